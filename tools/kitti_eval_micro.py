"""KITTI AP evaluation at KITTI-val size: a synthetic set (3769 frames, about 10 ground truths and 50 detections a frame, three classes plus
DontCare) through one get_official_eval_result(['Car', 'Pedestrian', 'Cyclist']) -- three eval_class, one per metric, 18 combinations each.
Reports the wall time of the whole call (median of --repeats behind a warm-up), and from one further call with a device synchronisation around
every stage: the host stages (concatenation + clean_data tables), each library entry, the torch plumbing between them (uploads, fill, sort)
as the remainder, the library calls and the blocking host reads.  No ratio to anything: the reference's numba code cannot run on this hardware.
Needs a GPU.

    python tools/kitti_eval_micro.py [--out profiles/kitti_eval.txt] [--frames 3769] [--repeats 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = np.array(["Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Truck"])
DIMS = np.array([[3.9, 1.55, 1.6], [0.8, 1.75, 0.6], [1.75, 1.7, 0.6], [5.0, 2.2, 1.9], [0.8, 1.25, 0.6], [10.0, 3.2, 2.6]])


def synthetic_set(frames, seed=0):
    rng = np.random.RandomState(seed)
    gt_annos, dt_annos = [], []

    def boxes(n, cls):
        z = rng.uniform(5, 75, n)
        loc = np.stack([rng.uniform(-0.45, 0.45, n) * z, rng.uniform(1.4, 1.9, n), z], 1)
        dims = DIMS[cls] * (1 + 0.08 * rng.randn(n, 3))
        hp, wp = 720 * dims[:, 1] / z, 500 * np.maximum(dims[:, 0], dims[:, 2]) / z
        u = 620 + 720 * loc[:, 0] / z
        bbox = np.stack([u - wp / 2, 190 - hp / 2, u + wp / 2, 190 + hp / 2], 1)
        return loc, dims, bbox

    for _ in range(frames):
        n_gt, n_dc, n_fp = rng.poisson(8) + 1, rng.poisson(2), rng.poisson(42)
        cls = rng.choice(6, n_gt, p=[0.5, 0.2, 0.12, 0.08, 0.04, 0.06])
        loc, dims, bbox = boxes(n_gt, cls)
        ry = rng.uniform(-np.pi, np.pi, n_gt)
        dc_u, dc_v = rng.uniform(50, 1100, n_dc), rng.uniform(150, 220, n_dc)
        gt_annos.append(dict(
            name=np.concatenate([CLASSES[cls], np.full(n_dc, "DontCare")]), truncated=np.concatenate([rng.choice([0, 0.2, 0.4, 0.6], n_gt), -np.ones(n_dc)]),
            occluded=np.concatenate([rng.choice(4, n_gt, p=[0.5, 0.2, 0.2, 0.1]), -np.ones(n_dc)]), alpha=np.concatenate([ry, np.full(n_dc, -10.0)]),
            bbox=np.concatenate([bbox, np.stack([dc_u, dc_v, dc_u + rng.uniform(40, 160, n_dc), dc_v + rng.uniform(25, 70, n_dc)], 1).reshape(-1, 4)]),
            dimensions=np.concatenate([dims, -np.ones((n_dc, 3))]), location=np.concatenate([loc, np.full((n_dc, 3), -1000.0)]),
            rotation_y=np.concatenate([ry, np.full(n_dc, -10.0)])))
        hit = rng.rand(n_gt) < 0.85
        fcls = rng.choice(3, n_fp)
        floc, fdims, fbbox = boxes(n_fp, fcls)
        n_hit = int(hit.sum())
        dt_annos.append(dict(
            name=np.concatenate([CLASSES[cls[hit]], CLASSES[fcls]]), truncated=np.zeros(n_hit + n_fp), occluded=np.zeros(n_hit + n_fp),
            alpha=np.concatenate([ry[hit] + 0.2 * rng.randn(n_hit), rng.uniform(-np.pi, np.pi, n_fp)]),
            bbox=np.concatenate([bbox[hit] + 2.5 * rng.randn(n_hit, 4), fbbox]),
            dimensions=np.concatenate([dims[hit] * (1 + 0.05 * rng.randn(n_hit, 3)), fdims]),
            location=np.concatenate([loc[hit] + rng.randn(n_hit, 3) * [0.15, 0.05, 0.15], floc]),
            rotation_y=np.concatenate([ry[hit] + 0.08 * rng.randn(n_hit), rng.uniform(-np.pi, np.pi, n_fp)]),
            score=np.concatenate([rng.beta(4, 2, n_hit), rng.beta(1.5, 4, n_fp)])))
    return gt_annos, dt_annos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from seevcn_amd.pcdet.datasets.kitti.kitti_object_eval_python import eval as E, rotate_iou as R

    gt_annos, dt_annos = synthetic_set(args.frames)
    n_gt, n_dt = sum(len(a["name"]) for a in gt_annos), sum(len(a["name"]) for a in dt_annos)
    pairs = sum(len(g["name"]) * len(d["name"]) for g, d in zip(gt_annos, dt_annos))
    classes = ["Car", "Pedestrian", "Cyclist"]
    lines = ["KITTI AP evaluation, synthetic KITTI-val-sized set: %d frames, %d ground truths (%.1f a frame), %d detections (%.1f a frame), %d (detection, "
             "ground truth) pairs; get_official_eval_result(%s): 3 metrics x 18 combinations x up to 41 thresholds"
             % (args.frames, n_gt, n_gt / args.frames, n_dt, n_dt / args.frames, pairs, classes),
             "measured once, on one MI355X, by tools/kitti_eval_micro.py; no ratio is claimed: the reference's numba evaluation cannot run on this hardware"]
    result, _ = E.get_official_eval_result(gt_annos, dt_annos, classes)          # warm-up
    walls = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.get_official_eval_result(gt_annos, dt_annos, classes)
        walls.append(time.perf_counter() - t0)
    walls.sort()
    lines.append("whole call, wall: median %.1f ms (min %.1f, max %.1f) over %d calls" % (1e3 * walls[len(walls) // 2], 1e3 * walls[0], 1e3 * walls[-1], len(walls)))

    stages = {}

    def timed(name, fn):
        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
            return out
        return wrapper

    call, read, frames_init, tables = R.call, R.read, E._Frames.__init__, E._Frames.tables
    R.call = lambda name, *a: timed(name, call)(name, *a)
    R.read = timed("host read (table + threshold counts)", read)
    E._Frames.__init__ = timed("host: concatenate annotations, name codes, offsets", frames_init)
    E._Frames.tables = timed("host: clean_data tables (9 class x difficulty rows)", tables)
    try:
        R.reset_counters()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.get_official_eval_result(gt_annos, dt_annos, classes)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        counters = dict(R.COUNTERS)
    finally:
        R.call, R.read, E._Frames.__init__, E._Frames.tables = call, read, frames_init, tables
    lines.append("one call with a device synchronisation around every stage: %.1f ms, of which (summed over the three metrics)" % (1e3 * total))
    for name, t in stages.items():
        lines.append("    %-58s %8.2f ms" % (name, 1e3 * t))
    lines.append("    %-58s %8.2f ms" % ("rest: uploads, torch fill / sort / cat, metric box columns, host AP", 1e3 * (total - sum(stages.values()))))
    lines.append("library calls %d (4 per eval_class), blocking host reads %d (1 per eval_class); the same for any number of frames" %
                 (counters["library_calls"], counters["host_reads"]))
    lines.append("first lines of the result:")
    lines += ["    " + l for l in result.splitlines()[:4]]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
