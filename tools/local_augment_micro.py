"""The pointpillar_newaugs augmentor queue on the device against its numpy restatement: 16 scenes of about 20 k points and 40 boxes, every entry
of the YAML's AUG_CONFIG_LIST enabled (gt_sampling from a small device database; the world translation with the key the code reads).

    python tools/local_augment_micro.py [--scenes 16] [--points 20000] [--boxes 40] [--reps 20] > profiles/local_augment.txt

forward: host-clock windows that end in a device synchronise (the boundary reads block anyway), median / min / max over --reps after a warm-up,
with the package's COUNTERS.  Kernels: device events around the library calls of one run of local steps and of the world dropout, on the batch as
gt_sampling left it, buffers restored outside the window.  numpy: one pass of tests/local_augment_reference.prepare_scene over the same scenes and
draws on this host, decisions unchecked, its moved-decision bookkeeping off; it still carries the error bounds and gaps next to every statement,
so it is an upper estimate of the reference's own loop.  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CLASSES = ["Car", "Pedestrian", "Cyclist"]
RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


def make_inputs(args):
    import augment_reference as R
    rng = np.random.RandomState(0)
    db_boxes = R.make_boxes(rng, 60, extent=40.0, min_gap=0.5)
    infos = {n: [] for n in CLASSES}
    for k, bx in enumerate(db_boxes):
        n = 40 + 7 * (k % 9)
        pts = np.concatenate([rng.uniform(-0.6, 0.6, (n, 3)), rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)
        infos[CLASSES[k % 3]].append(dict(name=CLASSES[k % 3], box3d_lidar=bx, points=pts, db_index=k, class_index=k % 3, num_points_in_gt=n, difficulty=0))
    scenes = []
    for b in range(args.scenes):
        boxes = R.make_boxes(rng, args.boxes, extent=46.0, min_gap=0.5)
        fg = R.make_points(rng, boxes, 0, 60, C=4, spread=0.55)
        pts = np.concatenate([fg, R.make_points(rng, boxes[:0], args.points - len(fg), 0, C=4, extent=54.0)])
        names = np.array(CLASSES + ["Van"])[rng.randint(0, 4, args.boxes)]
        scenes.append(dict(points=pts, gt_boxes=boxes, gt_names=names, num_points_in_gt=np.full(args.boxes, 99)))
    return scenes, infos, db_boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--boxes", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("local_augment_micro: needs a GPU")
    import local_augment_reference as LR
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, BatchDataAugmentor, reset_counters
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    from seevcn_amd.pcdet.datasets.augmentor.database_sampler import GtDatabase
    from seevcn_amd.pcdet.datasets.processor import DataProcessor
    from seevcn_amd.pcdet.model_cfgs import pointpillar_newaugs_augmentor_cfg
    dev = torch.device("cuda:0")
    scenes, infos, db_boxes = make_inputs(args)
    flat = sorted((i for v in infos.values() for i in v), key=lambda i: i["db_index"])
    db = GtDatabase.from_arrays([i["points"] for i in flat], db_boxes, [i["class_index"] for i in flat], dev)
    cfg = pointpillar_newaugs_augmentor_cfg()
    cfg["DISABLE_AUG_LIST"] = []
    for entry in cfg["AUG_CONFIG_LIST"]:
        if entry["NAME"] == "random_world_translation":
            entry["NOISE_TRANSLATE_STD"] = 0.2
    dp = DataProcessor([{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True}], np.array(RANGE, np.float32), True, 4)
    d_scenes = [dict(points=torch.from_numpy(s["points"]).to(dev), gt_boxes=torch.from_numpy(s["gt_boxes"]).to(dev), gt_names=s["gt_names"],
                     num_points_in_gt=s["num_points_in_gt"]) for s in scenes]
    B = args.scenes

    def forward():
        aug = BatchDataAugmentor(None, cfg, CLASSES, data_processor=dp, db_infos=infos, database=db)   # a fresh sampler: the same draws every time
        return aug.forward(d_scenes, rng=[np.random.RandomState(100 + b) for b in range(B)])

    print(f"local_augment_micro: {B} scenes x {args.points} points, {args.boxes} boxes, {args.reps} reps, {torch.cuda.get_device_name(0)}")
    reset_counters()
    out = forward()
    torch.cuda.synchronize()
    counters = dict(COUNTERS)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        forward()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    print(f"device  forward, the whole queue            median {np.median(ts):8.3f} ms   min {np.min(ts):8.3f}   max {np.max(ts):8.3f}   "
          f"calls {counters['library_calls']} reads {counters['host_reads']}   -> {out['points'].shape[0]} points, max_gt {out['gt_boxes'].shape[1]}")
    per_box = [len(d[1][1]) for d in out["draws"]]
    print(f"        boxes per scene behind gt_sampling: {min(per_box)} .. {max(per_box)}")

    # ---- the kernels, event-timed, on a batch of the same scenes with the boxes gt_sampling left (their draws: the forward's own)
    cls = [np.array([CLASSES.index(n) if n in CLASSES else -1 for n in s["gt_names"]], np.int32) for s in scenes]
    batch = A.DeviceBatch.from_scenes([s["points"] for s in d_scenes], [s["gt_boxes"] for s in d_scenes], cls)
    rng = np.random.RandomState(7)
    N = batch.total_boxes
    runs = [("local rotation + scaling (2 steps)", ["local_rotation", "local_scaling"], [(-0.157, 0.157), (0.95, 1.05)]),
            ("local translation x, y, z (3 steps)", ["local_translation_x", "local_translation_y", "local_translation_z"], [(0.95, 1.05)] * 3),
            ("local dropout top (1 step)", ["local_dropout_top"], [(0.0, 0.2)]),
            ("all six steps in one run", ["local_rotation", "local_scaling", "local_translation_x", "local_translation_y", "local_translation_z",
                                          "local_dropout_top"], [(-0.157, 0.157), (0.95, 1.05)] + [(0.95, 1.05)] * 3 + [(0.0, 0.2)])]
    saved = (batch.points.clone(), batch.boxes.clone(), batch.keep.clone(), batch.box_cls.clone())

    def restore():
        batch.points.copy_(saved[0]), batch.boxes.copy_(saved[1]), batch.keep.copy_(saved[2]), batch.box_cls.copy_(saved[3])

    def event_time(fn):
        out = []
        for i in range(args.reps + 2):
            restore()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                out.append(a.elapsed_time(b))
        return np.median(out), np.min(out), np.max(out)

    for label, steps, ranges in runs:
        params = torch.from_numpy(np.stack([rng.uniform(lo, hi, N) for lo, hi in ranges], axis=1)).to(dev)
        med, lo, hi = event_time(lambda: A.local_transform(batch, steps, params))
        print(f"kernels {label:38s}  median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   (plan + walk, device events)")
    inten = torch.from_numpy(rng.uniform(0, 0.2, (B, 4))).to(dev)
    for label, dirs in (("world dropout top", ["world_dropout_top"]), ("world dropout, four directions", list(A.WORLD_DROPOUT))):
        med, lo, hi = event_time(lambda: A.world_frustum_dropout(batch, dirs, inten[:, :len(dirs)].contiguous()))
        print(f"kernels {label:38s}  median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   (memset + a launch pair per direction)")

    # ---- the numpy restatement on this host, scene by scene, the forward's draws
    LR.TRACK_MOVED = False
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for s, c, d in zip(scenes, cls, out["draws"]):
            LR.prepare_scene(s["points"], s["gt_boxes"], c, d, 1, RANGE, 1, num_points_in_gt=s["num_points_in_gt"], check=False)
        ts.append(1e3 * (time.perf_counter() - t0))
    print(f"numpy   the same queue, {B} scenes in turn        median {np.median(ts):8.3f} ms   min {np.min(ts):8.3f}   max {np.max(ts):8.3f}   (3 passes, one host thread)")


if __name__ == "__main__":
    main()
