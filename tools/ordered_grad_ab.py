#!/usr/bin/env python3
"""What the opt-in order-fixed gradients cost: the atomic route against seevcn_amd.set_ordered_gradients(True) for the three entries, at the
workloads' own shapes --
  chamfer      VCN training loss, 64 objects x 1024 points each way                          (chamfer.backward)
  group        stacked grouping gradient, the raw-points source of PV-RCNN's set abstraction (group_points_grad_wrapper; C = 1, the intensity)
  sa ...       one scale of the PV-RCNN side mode's SA layers, backward of SAScaleTrain: x_conv1 (C 16, 16/16), x_conv3 (C 64, 64/64, 32 slots),
               RoI-grid pool (C 128, 64/64, 2 x 128 RoIs x 216 grid points over 2 x 2048 keypoints: lists of ~200 keys)
on synthetic clouds (points uniform in a ground slab of the KITTI range, queries on jittered points).  One process; the two routes alternate
call by call, HIP events around every call, the median of REPS calls after WARMUP of each.  No pass / fail: the ordered route is opt-in and
its price is information.
  python tools/ordered_grad_ab.py [--out profiles/ordered_grad_ab.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS = 5, 30


def slab(rng, n):
    import numpy as np
    return np.stack([rng.uniform(0, 70.4, n), rng.uniform(-40, 40, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import seevcn_amd
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as raw
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    from seevcn_amd.vcn.extensions.chamfer_dist import chamfer
    assert torch.cuda.is_available(), "tools/ordered_grad_ab.py needs a GPU"
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cases = []

    rng = np.random.default_rng(0)
    x1, x2 = t(rng.normal(0, 1, (64, 1024, 3)).astype(np.float32)), t(rng.normal(0, 1, (64, 1024, 3)).astype(np.float32))
    _, _, i1, i2 = chamfer.forward(x1, x2)
    g1, g2 = torch.full((64, 1024), 1 / 1024, device=dev), torch.full((64, 1024), 1 / 1024, device=dev)
    cases.append(("chamfer 64 x 1024 x 1024", lambda: chamfer.backward(x1, x2, i1, i2, g1, g2)))

    def scene_pair(n_per, m_per, jitter, around=None):
        """two scenes: support points, queries, their counts"""
        xyz = np.concatenate([slab(rng, n_per), slab(rng, n_per)])
        q = []
        for b in range(2):
            base = xyz[b * n_per:(b + 1) * n_per]
            centres = base[rng.integers(0, n_per, m_per if around is None else m_per // around)]
            if around is not None:
                centres = np.repeat(centres, around, axis=0)
            q.append(centres + rng.uniform(-jitter, jitter, centres.shape).astype(np.float32))
        cnt = torch.tensor([n_per, n_per], dtype=torch.int32, device=dev)
        qcnt = torch.tensor([len(q[0]), len(q[1])], dtype=torch.int32, device=dev)
        return t(xyz), t(np.concatenate(q)), cnt, qcnt

    def ball(xyz, new, cnt, qcnt, radius, ns):
        idx = torch.zeros((new.shape[0], ns), dtype=torch.int32, device=dev)
        raw.ball_query_wrapper(2, new.shape[0], radius, ns, new, qcnt, xyz, cnt, idx)
        return idx

    xyz, new, cnt, qcnt = scene_pair(16384, 2048, 0.2)
    idx = ball(xyz, new, cnt, qcnt, 0.8, 16)
    idx[idx[:, 0] < 0] = 0                                                        # as BallQuery.forward hands it to the grouping
    go = torch.randn((new.shape[0], 1, 16), device=dev)
    gf = torch.empty((xyz.shape[0], 1), device=dev)
    cases.append(("group raw_points M 4096 N 32768 C 1",
                  lambda: raw.group_points_grad_wrapper(2, new.shape[0], 1, xyz.shape[0], 16, go, idx, qcnt, cnt, gf)))

    def sa_case(name, n_per, m_per, C, C1, C2, ns, radius, jitter, around=None):
        xyz, new, cnt, qcnt = scene_pair(n_per, m_per, jitter, around)
        idx = ball(xyz, new, cnt, qcnt, radius, ns)
        row_start = raw._row_start(qcnt, cnt, new.shape[0])
        feats = torch.randn((xyz.shape[0], C), device=dev).requires_grad_(True)
        w1, w2 = (0.2 * torch.randn((C1, C + 3, 1, 1), device=dev)).requires_grad_(True), (0.2 * torch.randn((C2, C1, 1, 1), device=dev)).requires_grad_(True)
        bn = [torch.ones(C1, device=dev).requires_grad_(True), torch.zeros(C1, device=dev).requires_grad_(True),
              torch.ones(C2, device=dev).requires_grad_(True), torch.zeros(C2, device=dev).requires_grad_(True)]
        stats = [torch.zeros(C1, device=dev), torch.ones(C1, device=dev), torch.zeros((), dtype=torch.int64, device=dev),
                 torch.zeros(C2, device=dev), torch.ones(C2, device=dev), torch.zeros((), dtype=torch.int64, device=dev)]
        out = pu.sa_scale_train(xyz, feats, new, idx, row_start, w1, bn[0], bn[1], w2, bn[2], bn[3], *stats, 0.1, 1e-5)
        g = torch.randn_like(out)
        leaves = [feats, w1, w2] + bn
        keys = int((idx[:, 0] >= 0).sum()) * ns
        cases.append((f"sa {name} M {new.shape[0]} N {xyz.shape[0]} C {C} {C1}/{C2} ns {ns} ({keys / xyz.shape[0]:.0f} keys a point)",
                      lambda: torch.autograd.grad(out, leaves, g, retain_graph=True)))

    sa_case("x_conv1", 20000, 2048, 16, 16, 16, 16, 0.8, 0.2)
    sa_case("x_conv3", 8000, 2048, 64, 64, 64, 32, 2.4, 0.5)
    sa_case("roi_grid", 2048, 128 * 216, 128, 64, 64, 16, 1.6, 1.2, around=216)

    lines = [f"Order-fixed gradients (seevcn_amd.set_ordered_gradients) against the default float-atomic route; us per call, HIP events, median of {REPS} calls",
             f"after {WARMUP} warm-up calls of each route, one process, the routes alternating call by call; synthetic clouds (see tools/ordered_grad_ab.py)",
             "", f"{'entry':86s} {'atomic':>9s} {'ordered':>9s}   ordered / atomic"]
    for name, call in cases:
        times = {False: [], True: []}
        for rep in range(WARMUP + REPS):
            for flag in (False, True):
                with seevcn_amd.set_ordered_gradients(flag):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    call()
                    e.record()
                    torch.cuda.synchronize()
                if rep >= WARMUP:
                    times[flag].append(s.elapsed_time(e) * 1e3)
        a, o = float(np.median(times[False])), float(np.median(times[True]))
        lines.append(f"{name:86s} {a:9.1f} {o:9.1f}   {o / a:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
