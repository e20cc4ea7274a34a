"""Device-side training augmentation against its numpy restatement, stage by stage, at the nuScenes-source sizes: a batch of 16 scenes of about
21 k points, 30 boxes and 15 GT-sampling candidates each.

    python tools/augment_micro.py [--scenes 16] [--points 21000] [--boxes 30] [--reps 20] > profiles/augment.txt

Device times are host-clock windows that end in a device synchronise, medians over --reps after a warm-up; the numpy times are one pass of
tests/augment_reference.py (the reference's statements, its BEV IoU through the oracle's C restatement) over the same 16 scenes, decisions
unchecked.  Library calls and host reads are the package's COUNTERS.  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CLASS_NAMES = ["car", "truck", "bus"]
RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
EXTRA = [0.0, 0.0, 0.0]


def make_inputs(args):
    import augment_reference as R
    rng = np.random.RandomState(0)
    db_boxes = R.make_boxes(rng, 60, extent=40.0, min_gap=0.5)
    infos = {n: [] for n in CLASS_NAMES}
    for k, bx in enumerate(db_boxes):
        n = 40 + 7 * (k % 9)
        name = CLASS_NAMES[k % 3]
        pts = np.concatenate([rng.uniform(-0.7, 0.7, (n, 3)), rng.uniform(0, 1, (n, 2))], axis=1).astype(np.float32)
        infos[name].append(dict(name=name, box3d_lidar=bx, points=pts, db_index=k, class_index=k % 3, num_points_in_gt=n, difficulty=0))
    scenes = []
    for b in range(args.scenes):
        boxes = R.make_boxes(rng, args.boxes, extent=46.0, min_gap=0.5)
        fg = R.make_points(rng, boxes, 0, 60, spread=0.55)
        pts = np.concatenate([fg, R.make_points(rng, boxes[:0], args.points - len(fg), 0, extent=54.0)])
        names = np.array(CLASS_NAMES + ["pedestrian"])[rng.randint(0, 4, args.boxes)]
        scenes.append(dict(points=pts, gt_boxes=boxes, gt_names=names))
    return scenes, infos, db_boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, default=21000)
    ap.add_argument("--boxes", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("augment_micro: needs a GPU")
    import augment_reference as R
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, BatchDataAugmentor, DeviceBatch, draw_params, reset_counters
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    from seevcn_amd.pcdet.datasets.augmentor.database_sampler import DataBaseSampler, GtDatabase
    from seevcn_amd.pcdet.datasets.processor import DataProcessor
    dev = torch.device("cuda:0")
    scenes, infos, db_boxes = make_inputs(args)
    flat = sorted((i for v in infos.values() for i in v), key=lambda i: i["db_index"])
    db = GtDatabase.from_arrays([i["points"] for i in flat], db_boxes, [i["class_index"] for i in flat], dev)
    gt_cfg = {"NAME": "gt_sampling", "PREPARE": {"filter_by_min_points": ["car:5", "truck:5", "bus:5"]}, "SAMPLE_GROUPS": ["car:5", "truck:5", "bus:5"],
              "NUM_POINT_FEATURES": 5, "REMOVE_EXTRA_WIDTH": EXTRA, "LIMIT_WHOLE_SCENE": False}
    aug_cfg = [{"NAME": "random_object_scaling", "SCALE_UNIFORM_NOISE": [0.75, 1.0]}, gt_cfg,
               {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x", "y"]}, {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.3925, 0.3925]},
               {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]
    dp = DataProcessor([{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True}], np.array(RANGE, np.float32), True, 5)
    min_points = 30
    cls = [np.array([CLASS_NAMES.index(n) if n in CLASS_NAMES else -1 for n in s["gt_names"]], np.int32) for s in scenes]
    d_scenes = [dict(points=torch.from_numpy(s["points"]).to(dev), gt_boxes=torch.from_numpy(s["gt_boxes"]).to(dev), gt_names=s["gt_names"]) for s in scenes]

    def sync_time(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))

    print(f"augment_micro: {args.scenes} scenes x {args.points} points, {args.boxes} boxes, 15 candidates per scene, {args.reps} reps, {torch.cuda.get_device_name(0)}")
    # ---- the whole path
    aug = BatchDataAugmentor(None, aug_cfg, CLASS_NAMES, min_points_of_gt=min_points, data_processor=dp, db_infos=infos, database=db)
    reset_counters()
    out = aug.forward(d_scenes, rng=np.random.RandomState(1))
    whole_counters = dict(COUNTERS)
    med, best = sync_time(lambda: aug.forward(d_scenes, rng=np.random.RandomState(1)), args.reps)
    print(f"device  forward (counts on the device)      median {med:8.3f} ms   min {best:8.3f} ms   calls {whole_counters['library_calls']} reads {whole_counters['host_reads']}"
          f"   -> {out['points'].shape[0]} points, max_gt {out['gt_boxes'].shape[1]}")
    # ---- stage by stage on the device
    counts = [R.points_in_boxes_count(s["points"], s["gt_boxes"])[0] for s in scenes]
    names = [s["gt_names"][c >= min_points] for s, c in zip(scenes, counts)]
    sampler = DataBaseSampler(None, gt_cfg, CLASS_NAMES, infos, db)
    draws = draw_params(np.random.RandomState(1), aug_cfg, [len(n) for n in names], sampler, names)
    cands = [d[1][1] for d in draws]
    slots = [int(sum(len(i["points"]) for _, i in c)) for c in cands]

    def fresh():
        b = DeviceBatch.from_scenes([s["points"] for s in d_scenes], [s["gt_boxes"] for s in d_scenes], cls, slots, [len(c) for c in cands])
        return b
    noises = np.zeros((sum(args.boxes + len(c) for c in cands), 50))
    row = 0
    for b, d in enumerate(draws):
        keep = np.nonzero(counts[b] >= min_points)[0]
        noises[row + keep] = d[0][1]
        row += args.boxes + len(cands[b])
    noises_d = torch.from_numpy(noises).to(dev)
    world = np.array([[float(v) for n, v in d[2:]] for d in draws])
    stages = [("build the stacked batch", lambda b: fresh()),
              ("points_in_boxes_count", lambda b: A.points_in_boxes_count(b)),
              ("scale_pre_object (plan + points)", lambda b: A.scale_pre_object(b, noises_d)),
              ("gt_sampling (select + paste)", lambda b: sampler(b, cands)),
              ("world transforms (4 ops, heading)", lambda b: A.world_transform(b, ["flip_x", "flip_y", "rotation", "scaling"], world, limit_heading=True)),
              ("compact + the one host read", lambda b: A.compact(b, **dp.tail_args()))]
    for label, fn in stages:
        batch = fresh()
        reset_counters()
        fn(batch)
        c = dict(COUNTERS)
        med, best = sync_time(lambda: fn(batch), args.reps)
        print(f"device  {label:38s}  median {med:8.3f} ms   min {best:8.3f} ms   calls {c['library_calls']} reads {c['host_reads']}")
    # ---- the numpy restatement, scene by scene
    t = {"points_in_boxes_count": 0.0, "scale_pre_object": 0.0, "gt_sampling": 0.0, "world transforms": 0.0, "tail": 0.0}
    for s, d, c, k in zip(scenes, draws, counts, cls):
        t0 = time.perf_counter()
        R.points_in_boxes_count(s["points"], s["gt_boxes"])
        t1 = time.perf_counter()
        keep = c >= min_points
        pts, boxes, alive, _, _, _ = R.scale_pre_object(s["gt_boxes"][keep], s["points"], k[keep] >= 0, d[0][1], check=False)
        t2 = time.perf_counter()
        groups = [(np.stack([i["box3d_lidar"] for g, i in d[1][1] if g == gid]), [i["points"] for g, i in d[1][1] if g == gid]) for gid in sorted({g for g, _ in d[1][1]})]
        pts, boxes, _, _, _ = R.gt_sampling(pts[alive], boxes, k[keep] >= 0, groups, EXTRA, check=False)
        t3 = time.perf_counter()
        boxes, pts, _, _ = R.world_transform(boxes, pts, d[2:])
        R.limit_period(boxes[:, 6])
        t4 = time.perf_counter()
        pts = pts[R.mask_points_by_range(pts, RANGE)]
        boxes[R.mask_boxes_outside_range(boxes, RANGE, 1)]
        t5 = time.perf_counter()
        for key, dt in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
            t[key] += dt
    for key, v in t.items():
        print(f"numpy   {key:38s}  {1e3 * v:10.3f} ms for the {args.scenes} scenes, one pass")
    print(f"numpy   {'all stages':38s}  {1e3 * sum(t.values()):10.3f} ms")


if __name__ == "__main__":
    main()
