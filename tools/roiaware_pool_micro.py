"""RoI-aware pooling at PartA2.yaml sizes (4 scenes, 128 RoIs a scene, 12^3 cells, at most 127 points a cell, about 20 k points a scene from a
synthetic scene): the assignment, the two poolings the head runs (avg C = 4, max C = 16) and their backwards (atomic and order-fixed), each as
ONE call over the whole batch (box_pt_range) and as the per-scene loop over the same entries, alternating in one process.  Device events around
windows of calls behind a warm-up; medians with the spread over the windows.  Bytes per call are computed from the shapes and the lists' counts.
Needs a GPU (--rehearse: build the inputs, print the byte counts, stop).

    python tools/roiaware_pool_micro.py [--out profiles/roiaware_pool.txt] [--windows 15] [--calls 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seevcn_amd.synth as synth  # noqa: E402
from seevcn_amd.pcdet import model_cfgs as C  # noqa: E402

SCENES, ROIS, POOL, CAP = 4, 128, 12, 128
VOXEL = np.array([0.05, 0.05, 0.1])


def make_inputs(n_az):
    """Points: the centres of the occupied voxels (what UNetV2 hands the head), stacked scene after scene.  RoIs: jittered ground truth and
    random boxes on the ground, 128 a scene."""
    rng = np.random.default_rng(5)
    pts, gt = synth.make_scene_batch(SCENES, seed=2000, n_az=n_az)
    rg = np.array(C.KITTI_RANGE[:3])
    cells = np.unique(np.concatenate([pts[:, 0:1], np.floor((pts[:, 1:4] - rg) / VOXEL)], 1).astype(np.int64), axis=0)
    cells = cells[np.argsort(cells[:, 0], kind='stable')]
    xyz = ((cells[:, 1:4] + 0.5) * VOXEL + rg).astype(np.float32)
    counts = np.bincount(cells[:, 0], minlength=SCENES)
    rois = []
    for b in range(SCENES):
        g = gt[b][gt[b, :, 3] > 0][:, :7]
        rep = np.repeat(g, 8, axis=0) + rng.normal(0, 1, (len(g) * 8, 7)).astype(np.float32) * np.array([0.3, 0.3, 0.1, 0.1, 0.05, 0.05, 0.2], np.float32)
        rnd = np.concatenate([rng.uniform([0, -40, -2], [70, 40, 0], (ROIS, 3)), rng.uniform([1.5, 0.6, 1.2], [4.5, 2, 2], (ROIS, 3)),
                              rng.uniform(-3, 3, (ROIS, 1))], 1).astype(np.float32)
        rois.append(np.concatenate([rep, rnd])[:ROIS])
    return xyz, counts, np.concatenate(rois).astype(np.float32)


def timed(fn, windows, calls):
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return sorted(ms)


def fmt(name, ms, nbytes=None):
    med = ms[len(ms) // 2]
    rate = f"   {nbytes / 1e6:9.2f} MB -> {nbytes / med / 1e6:8.1f} GB/s" if nbytes else ""
    return f"{name:<50s} median {med:8.3f} ms   min {ms[0]:8.3f}   max {ms[-1]:8.3f}   ({len(ms)} windows){rate}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-az", type=int, default=900)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    xyz, counts, rois = make_inputs(a.n_az)
    n_pts, n_boxes, cells = len(xyz), len(rois), POOL ** 3
    starts = np.concatenate([[0], np.cumsum(counts)])
    ranges = np.repeat(np.stack([starts[:-1], starts[1:]], 1), ROIS, axis=0).astype(np.int32)
    lines = [f"RoI-aware pooling: {SCENES} scenes, points per scene {counts.tolist()}, {ROIS} RoIs a scene, {POOL}^3 cells, cap {CAP}"]
    # what the calls must move (bytes), from the shapes: the assignment reads every point of a box's scene once per box (L2 serves the re-reads: a
    # scene is 12 B x 20 k = 240 KB) and writes the counts; listed points are known after the run
    lines.append(f"assignment: point reads issued {int((ranges[:, 1] - ranges[:, 0]).sum()) * 12 / 1e6:.1f} MB (distinct {n_pts * 12 / 1e6:.2f} MB), "
                 f"counts written {n_boxes * cells * 4 / 1e6:.2f} MB; the list tensor spans {n_boxes * cells * CAP * 4 / 1e6:.1f} MB and is never zero-filled")
    if a.rehearse or not torch.cuda.is_available():
        print("\n".join(lines))
        if not a.rehearse:
            raise SystemExit("roiaware_pool_micro: no GPU visible; timings are not produced anywhere else")
        return
    from seevcn_amd import set_ordered_gradients
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as U
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(x).to(dev)
    pts, boxes, rng_d = t(xyz), t(rois), t(ranges)
    g = torch.Generator().manual_seed(3)
    f4, f16 = torch.rand((n_pts, 4), generator=g).to(dev), torch.randn((n_pts, 16), generator=g).to(dev)
    go4, go16 = torch.randn((n_boxes, POOL, POOL, POOL, 4), generator=g).to(dev), torch.randn((n_boxes, POOL, POOL, POOL, 16), generator=g).to(dev)
    scene = [(boxes[b * ROIS:(b + 1) * ROIS].contiguous(), pts[starts[b]:starts[b + 1]].contiguous(), f4[starts[b]:starts[b + 1]].contiguous(),
              f16[starts[b]:starts[b + 1]].contiguous()) for b in range(SCENES)]

    lists = U.assign_points_to_cells(boxes, pts, POOL, CAP, rng_d)
    cnt = lists[..., 0]
    listed, nonempty = int(cnt.sum()), int((cnt > 0).sum())
    lines.append(f"lists: {listed} listed points in {nonempty} non-empty cells of {n_boxes * cells}; fullest cell {int(cnt.max())}")
    # same lists from the per-scene calls (rows relative to the scene)
    for b in range(SCENES):
        single = U.assign_points_to_cells(scene[b][0], scene[b][1], POOL, CAP)
        part = lists[b * ROIS:(b + 1) * ROIS]
        live = torch.arange(CAP, device=dev) <= part[..., :1]
        shifted = torch.where(live, part - int(starts[b]), part)
        shifted[..., 0] = part[..., 0]
        assert torch.equal(torch.where(live, shifted, 0), torch.where(live, single, 0)), "batched and per-scene lists differ"

    def pool_bytes(c):
        return n_boxes * cells * 4 + listed * 4 + listed * c * 4 + n_boxes * cells * c * 4 * (2 if c == 16 else 1)

    def fwd(feat, method):
        return lambda: U.RoIAwarePoolFromListsFunction.apply(feat, lists, method)

    def loop_assign():
        for s in scene:
            U.assign_points_to_cells(s[0], s[1], POOL, CAP)

    scene_lists = [U.assign_points_to_cells(s[0], s[1], POOL, CAP) for s in scene]

    def loop_pool(k, method):
        def run():
            for s, l in zip(scene, scene_lists):
                U.RoIAwarePoolFromListsFunction.apply(s[k], l, method)
        return run

    def head_batched():
        pool = U.RoIAwarePool3d(POOL, CAP)
        return lambda: pool.forward_multi(boxes, pts, [f4, f16], ['avg', 'max'], rng_d)

    def head_loop():
        pool = U.RoIAwarePool3d(POOL, CAP)

        def run():
            for s in scene:
                pool(s[0], s[1], s[2], 'avg')
                pool(s[0], s[1], s[3], 'max')
        return run

    def bwd(feat, method, grad):
        f = feat.clone().requires_grad_(True)
        out = U.RoIAwarePoolFromListsFunction.apply(f, lists, method)

        def run():
            f.grad = None
            out.backward(grad, retain_graph=True)
        return run

    jobs = [("assign, one launch for the batch", lambda: U.assign_points_to_cells(boxes, pts, POOL, CAP, rng_d), None),
            ("assign, one call per scene", loop_assign, None),
            ("pool avg C=4, batch", fwd(f4, 'avg'), pool_bytes(4)),
            ("pool avg C=4, per scene", loop_pool(2, 'avg'), pool_bytes(4)),
            ("pool max C=16, batch", fwd(f16, 'max'), pool_bytes(16)),
            ("pool max C=16, per scene", loop_pool(3, 'max'), pool_bytes(16)),
            ("head's pooling (assign + avg + max), batch", head_batched(), None),
            ("head's pooling (2 x (assign + pool)), per scene", head_loop(), None),
            ("backward avg C=4, atomics", bwd(f4, 'avg', go4), None),
            ("backward max C=16, atomics", bwd(f16, 'max', go16), None)]
    for _, fn, _ in jobs:                                   # warm-up of every shape the windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in jobs}
    for w in range(a.windows):                              # alternating: every window of every job sees the same neighbours
        for name, fn, _ in jobs:
            res[name] += timed(fn, 1, a.calls)
    for name, _, nbytes in jobs:
        lines.append(fmt(name, sorted(res[name]), nbytes))
    with set_ordered_gradients(True):
        ordered = [("backward avg C=4, order-fixed", bwd(f4, 'avg', go4)), ("backward max C=16, order-fixed", bwd(f16, 'max', go16))]
        for name, fn in ordered:
            for _ in range(2):
                fn()
            lines.append(fmt(name, timed(fn, max(a.windows // 3, 3), max(a.calls // 5, 1))))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
