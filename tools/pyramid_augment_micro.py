"""random_local_pyramid_aug on the device against its numpy restatement at pointpillar_pyramid_aug.yaml sizes: 16 scenes of about 20 k x 4 points,
10 .. 40 boxes a scene.

    python tools/pyramid_augment_micro.py [--scenes 16] [--points 20000] [--reps 20] > profiles/pyramid_augment.txt

forward: the queue [random_local_pyramid_aug] with the YAML's settings and, because those select few boxes, with every probability at 0.5;
host-clock windows that end in a device synchronise, median / min / max over --reps after a warm-up, with the package's COUNTERS.  Kernels: device
events around each library call on the same batch (every box dropping a face; the counts of all six faces of every box; a sparsify plan over every
box's fullest face; a swap plan with every box selected), buffers restored outside the window.  numpy: tests/pyramid_augment_reference's three
functions over the same scenes from the same seeds on this host (the scenes here are not filtered by the generator's 1e-6 m band, so a point count
may differ by a point; the time does not).  Needs a GPU: there is no fallback."""
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
YAML = {"DROP_PROB": 0.25, "SPARSIFY_PROB": 0.05, "SPARSIFY_MAX_NUM": 50, "SWAP_PROB": 0.1, "SWAP_MAX_NUM": 50}
BUSY = {"DROP_PROB": 0.5, "SPARSIFY_PROB": 0.5, "SPARSIFY_MAX_NUM": 50, "SWAP_PROB": 0.5, "SWAP_MAX_NUM": 50}


def make_inputs(args):
    import augment_reference as R
    rng = np.random.RandomState(0)
    scenes = []
    for b in range(args.scenes):
        n = 10 + (30 * b) // max(args.scenes - 1, 1)             # 10 .. 40 boxes
        boxes = R.make_boxes(rng, n, extent=46.0, min_gap=0.5)
        fg = R.make_points(rng, boxes, 0, 400, C=4, spread=0.55)
        pts = np.concatenate([fg, R.make_points(rng, boxes[:0], max(args.points - len(fg), 0), 0, C=4, extent=54.0)])
        scenes.append(dict(points=pts[rng.permutation(len(pts))], gt_boxes=boxes, gt_names=np.array(["Car"] * n), num_points_in_gt=np.full(n, 99)))
    return scenes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pyramid_augment_micro: needs a GPU")
    import pyramid_augment_reference as PR
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, BatchDataAugmentor, reset_counters
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    dev = torch.device("cuda:0")
    scenes = make_inputs(args)
    B = args.scenes
    d_scenes = [dict(points=torch.from_numpy(s["points"]).to(dev), gt_boxes=torch.from_numpy(s["gt_boxes"]).to(dev), gt_names=s["gt_names"],
                     num_points_in_gt=s["num_points_in_gt"]) for s in scenes]
    print(f"pyramid_augment_micro: {B} scenes x {args.points} points x 4, {len(scenes[0]['gt_boxes'])} .. {len(scenes[-1]['gt_boxes'])} boxes, "
          f"{args.reps} reps, {torch.cuda.get_device_name(0)}")
    for label, cfg in (("the YAML's settings", YAML), ("every probability 0.5", BUSY)):
        aug = BatchDataAugmentor(None, [dict(cfg, NAME="random_local_pyramid_aug")], CLASSES)
        forward = lambda: aug.forward(d_scenes, rng=[np.random.RandomState(100 + b) for b in range(B)])
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
        pairs = sum(len(dict(d)["pyramid_swap_face"]) for d in out["draws"])
        sparsified = sum(len(dict(d)["pyramid_sparsify_choice"]) for d in out["draws"])
        print(f"device  forward, {label:24s} median {np.median(ts):8.3f} ms   min {np.min(ts):8.3f}   max {np.max(ts):8.3f}   "
              f"calls {counters['library_calls']} reads {counters['host_reads']}   {sparsified} pyramids sparsified, {pairs} pairs swapped "
              f"-> {out['points'].shape[0]} points")
        ts, total = [], 0
        for _ in range(3):
            t0 = time.perf_counter()
            total = 0
            for b, s in enumerate(scenes):
                total += len(PR.random_local_pyramid_aug(s["gt_boxes"], s["points"], cfg, np.random.RandomState(100 + b))[0])
            ts.append(1e3 * (time.perf_counter() - t0))
        print(f"numpy   the same, {B} scenes in turn            median {np.median(ts):8.3f} ms   min {np.min(ts):8.3f}   max {np.max(ts):8.3f}   "
              f"(3 passes, one host thread) -> {total} points")

    # ---- the kernels, event-timed
    batch = A.DeviceBatch.from_scenes([s["points"] for s in d_scenes], [s["gt_boxes"] for s in d_scenes], [np.zeros(len(s["gt_boxes"]), np.int32) for s in scenes])
    N = batch.total_boxes
    rng = np.random.RandomState(7)
    counts = A.read(A.points_in_pyramids_mask(batch))
    rows = [batch.box_offsets[b] + np.arange(len(s["gt_boxes"])) for b, s in enumerate(scenes)]
    sp = A.plan_pyramid_sparsify(counts, [(r, counts[r].argmax(1)) for r in rows], 50, [np.random.RandomState(b) for b in range(B)])
    sw = A.plan_pyramid_swap(counts, rows, [np.ones(len(r), bool) for r in rows], 50, [np.random.RandomState(b) for b in range(B)])
    first = batch.add_room(sp["room"] + sw["room"])              # both plans' rows once, so that the timed calls do not re-stack
    ends = batch.pt_offsets + batch.pt_sizes                     # a plan without room counts its rows from the scene's end
    sp["pyr"][:, 4] += (first - ends)[sp["pyr"][:, 0]]
    sw["pairs"][:, 7] += (first + sp["room"] - ends)[sw["pairs"][:, 0]]
    sp, sw = dict(sp, room=0 * sp["room"]), dict(sw, room=0 * sw["room"])
    saved = (batch.points.clone(), batch.keep.clone())

    def event_time(fn):
        out = []
        for i in range(args.reps + 2):
            batch.points.copy_(saved[0]), batch.keep.copy_(saved[1])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                out.append(a.elapsed_time(b))
        return np.median(out), np.min(out), np.max(out)

    faces, u = rng.randint(0, 6, N), np.zeros(N)
    runs = [(f"dropout, a face of each of {N} boxes", lambda: A.local_pyramid_dropout(batch, faces, u, 1.0)),
            (f"counts, six faces of {N} boxes", lambda: A.points_in_pyramids_mask(batch)),
            (f"sparsify, {len(sp['pyr'])} pyramids to 50", lambda: A.local_pyramid_sparsify(batch, sp)),
            (f"swap, {len(sw['pairs'])} pairs", lambda: A.local_pyramid_swap(batch, sw))]
    for label, fn in runs:
        med, lo, hi = event_time(fn)
        print(f"kernels {label:40s} median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   (one library call with its uploads, device events)")
    A.read_checked(batch, batch.box_cls[:1])                     # a count mismatch in a timed plan would raise here


if __name__ == "__main__":
    main()
