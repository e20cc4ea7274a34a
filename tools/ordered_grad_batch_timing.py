"""Device time of the three dense-batch gradient entries alone, atomic against order-fixed, at the shapes pointrcnn.yaml produces (2 scenes x
16 384 points): the groupings of SA_modules.0 (c = 1, the intensity channel; 4096 queries, nsample 16 / 32) and SA_modules.1 (c = 96; 1024
queries over 4096 points -- the first grouping whose gradient a train step takes, the input features of SA_modules.0 need none), the gather of
SA_modules.0's sampling (c = 3) and the interpolation of FP_modules.0 (c = 256, 16 384 unknown points over 4096 known ones).  Indices come
from this library's own farthest point sampling, ball query and three_nn on the synthetic scenes of tools/pointrcnn_step.py.  Every call is
bracketed by device events; the two routes alternate call by call behind a warm-up; median, min .. max over the timed calls.  The ordered
output is compared with the atomic one at the timed size, and two ordered calls bit for bit.  Needs a GPU (--rehearse: build the inputs'
shapes on the CPU, print them, stop).

    python tools/ordered_grad_batch_timing.py [--out profiles/ordered_grad_batch.txt] [--calls 200] [--warmup 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENES, POINTS = 2, 16384
# name, entry, channels, (support points, queries, radius, nsample)
GROUPS = [("SA_modules.0 scale 0", 1, (16384, 4096, 0.1, 16)), ("SA_modules.0 scale 1", 1, (16384, 4096, 0.5, 32)),
          ("SA_modules.1 scale 0", 96, (4096, 1024, 0.5, 16)), ("SA_modules.1 scale 1", 96, (4096, 1024, 1.0, 32))]
GATHER = ("SA_modules.0 sampling", 3, (16384, 4096))
INTERP = ("FP_modules.0", 256, (16384, 4096))


def time_pair(run, calls, warmup):
    """run(ordered) enqueues one call -> per-route list of ms, the routes alternating"""
    for _ in range(warmup):
        run(False), run(True)
    torch.cuda.synchronize()
    spans = {False: [], True: []}
    for _ in range(calls):
        for ordered in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(ordered)
            b.record()
            spans[ordered].append((a, b))
    torch.cuda.synchronize()
    return {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in spans.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    lines = [f"dense-batch gradient entries, atomic against order-fixed: {SCENES} scenes x {POINTS} points, {a.calls} calls a route behind {a.warmup} "
             f"warm-up calls, the routes alternating; device events around every call (ms: median, min .. max)"]
    if a.rehearse or not torch.cuda.is_available():
        for name, c, shape in GROUPS + [GATHER, INTERP]:
            lines.append(f"{name}: c {c}, {shape}")
        print("\n".join(lines))
        if not a.rehearse:
            raise SystemExit("ordered_grad_batch_timing: no GPU visible; timings are not produced anywhere else")
        return
    import pointrcnn_step
    import seevcn_amd._lib as L
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pu
    dev = torch.device("cuda:0")
    lib = L.load()
    p = L.ptr
    pts, _ = pointrcnn_step.make_inputs()
    xyz0 = torch.from_numpy(pts[:, 1:4].reshape(SCENES, POINTS, 3)).to(dev).contiguous()
    level = {16384: xyz0}
    level[4096] = pu.gather_operation(xyz0.transpose(1, 2).contiguous(), pu.farthest_point_sample(xyz0, 4096)).transpose(1, 2).contiguous()
    level[1024] = pu.gather_operation(level[4096].transpose(1, 2).contiguous(), pu.farthest_point_sample(level[4096], 1024)).transpose(1, 2).contiguous()
    gen = torch.Generator(device=dev).manual_seed(3)
    B = SCENES

    def report(name, c, what, run, out, rows_named):
        t = time_pair(run, a.calls, a.warmup)
        run(True)
        first = out.clone()
        run(True)
        same = bool((first.view(torch.int32) == out.view(torch.int32)).all())
        run(False)
        diff = float((first - out).abs().max())
        lines.append(f"{name}: c {c}, {what}; rows named {rows_named}; ordered twice: {'same bits' if same else 'DIFFERENT BITS'}; "
                     f"largest |ordered - atomic| {diff:.3e}")
        for ordered in (False, True):
            v = t[ordered]
            lines.append(f"    {'ordered' if ordered else 'atomic ':<8s} {v[len(v) // 2]:8.4f}   {v[0]:8.4f} .. {v[-1]:8.4f}")

    def named(idx, rows):
        """share of the destination rows that some key names, and the longest list"""
        flat = (idx.reshape(B, -1).long() + torch.arange(B, device=dev)[:, None] * rows).reshape(-1)
        cnt = torch.bincount(flat, minlength=B * rows)
        return f"{int((cnt > 0).sum())} of {B * rows}, longest list {int(cnt.max())}"

    for name, c, (n, npoint, radius, nsample) in GROUPS:
        idx = pu.ball_query(radius, nsample, level[n], level[npoint])
        grad_out = torch.randn((B, c, npoint, nsample), device=dev, generator=gen)
        out = torch.empty((B, c, n), device=dev)
        scratch = torch.empty(lib.sv_group_points_grad_batch_ordered_scratch_bytes(B, n, npoint, nsample), dtype=torch.uint8, device=dev)

        def run(ordered, c=c, n=n, npoint=npoint, nsample=nsample, grad_out=grad_out, idx=idx, out=out, scratch=scratch):
            if ordered:
                L.check(lib.sv_group_points_grad_batch_ordered(B, c, n, npoint, nsample, p(grad_out), p(idx), p(scratch), p(out), L.stream()), "ordered")
            else:
                L.check(lib.sv_group_points_grad_batch(B, c, n, npoint, nsample, p(grad_out), p(idx), p(out), L.stream()), "atomic")
        report("group_points_grad_batch, " + name, c, f"n {n}, npoint {npoint}, nsample {nsample}, radius {radius}", run, out, named(idx, n))

    name, c, (n, npoint) = GATHER
    idx = pu.farthest_point_sample(xyz0, npoint)
    grad_out = torch.randn((B, c, npoint), device=dev, generator=gen)
    out = torch.empty((B, c, n), device=dev)
    scratch = torch.empty(lib.sv_gather_points_grad_batch_ordered_scratch_bytes(B, n, npoint), dtype=torch.uint8, device=dev)

    def run_gather(ordered):
        if ordered:
            L.check(lib.sv_gather_points_grad_batch_ordered(B, c, n, npoint, p(grad_out), p(idx), p(scratch), p(out), L.stream()), "ordered")
        else:
            L.check(lib.sv_gather_points_grad_batch(B, c, n, npoint, p(grad_out), p(idx), p(out), L.stream()), "atomic")
    report("gather_points_grad_batch, " + name, c, f"n {n}, npoint {npoint}", run_gather, out, named(idx, n))

    name, c, (n, m) = INTERP
    dist, idx = pu.three_nn(level[n], level[m])
    w = 1.0 / (dist + 1e-8)
    weight = (w / w.sum(dim=2, keepdim=True)).contiguous()
    grad_out = torch.randn((B, c, n), device=dev, generator=gen)
    out = torch.empty((B, c, m), device=dev)
    scratch = torch.empty(lib.sv_three_interpolate_grad_batch_ordered_scratch_bytes(B, n, m), dtype=torch.uint8, device=dev)

    def run_interp(ordered):
        if ordered:
            L.check(lib.sv_three_interpolate_grad_batch_ordered(B, c, n, m, p(grad_out), p(idx), p(weight), p(scratch), p(out), L.stream()), "ordered")
        else:
            L.check(lib.sv_three_interpolate_grad_batch(B, c, n, m, p(grad_out), p(idx), p(weight), p(out), L.stream()), "atomic")
    report("three_interpolate_grad_batch, " + name, c, f"n {n}, m {m}", run_interp, out, named(idx, m))

    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
