"""Vector-pool aggregation at pv_rcnn_plusplus.yaml sizes, 2 scenes: time per call of the choice kernel (sv_vector_pool_choice), the local 3-NN
(sv_vector_pool_three_nn), the stacked interpolation (sv_three_interpolate_stack) and of one VectorPoolAggregationModuleMSG eval forward, each
beside a plain-torch statement of the same result written the way one would write it without the kernels (broadcast masks over (queries, support),
scatter-min of the first row per cell, chunked top-3).  The statements are compared with the kernels, element for element, before anything is timed; a difference is written into the record and fails the run.

  RoI-grid side   2 x 27 648 queries (128 RoIs x 216 grid points) over 2 x 4 096 keypoints, 90 -> 30 channels, [3, 3, 3] cells, R 0.8 / 1.6, nsample 32
  keypoint side   2 x 4 096 queries over an x_conv3-sized support (2 x 30 000 voxel centres), 64 -> 32 channels, 27 centres, R 1.2 x 2, nsample -1

Device events around windows of calls behind a warm-up, medians with their range; kernel time and launch count of ONE call from torch.profiler.
Needs a GPU (--rehearse: small sizes on the CPU, the torch statements against the numpy restatement of tests/vector_pool_reference.py, stop).

    python tools/vector_pool_micro.py [--out profiles/vector_pool.txt] [--windows 15] [--calls 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = dict(roi=dict(queries=27648, support=4096, c_in=90, c_each=30, grid=(3, 3, 3), R=0.8, nsample=32),
             kp=dict(queries=4096, support=30000, c_in=64, c_each=32, grid=(3, 3, 3), R=1.2, mult=2.0, nsample=-1))


def make_inputs(kind, scale=1.0, seed=3):
    """Two scenes: support points LiDAR-like (a ground sheet 70 x 80 m plus clusters), queries drawn near support points."""
    s = SIZES[kind]
    n, m = max(64, int(s["support"] * scale)), max(8, int(s["queries"] * scale))
    rng = np.random.default_rng(seed)
    xyz, new_xyz = [], []
    for b in range(2):
        spots = rng.uniform([5, -30, -1.0], [60, 30, 0.0], (40, 3))
        near = spots[rng.integers(0, len(spots), n // 2)] + rng.normal(0, 1.5, (n // 2, 3)) * np.array([1.0, 1.0, 0.3])
        far = rng.uniform([0, -40, -2.0], [70, 40, 0.5], (n - len(near), 3))
        p = np.concatenate([near, far])[rng.permutation(n)].astype(np.float32)
        q = (p[rng.integers(0, n, m)] + rng.normal(0, 0.4, (m, 3))).astype(np.float32)
        xyz.append(p)
        new_xyz.append(q)
    feats = rng.standard_normal((2 * n, s["c_in"])).astype(np.float32)
    return np.concatenate(xyz), np.array([n, n], np.int32), np.concatenate(new_xyz), np.array([m, m], np.int32), feats


def _in_range(loc, R):
    return ~((loc.abs() > R).any(-1))


def torch_choice(xyz, xyz_cnt, feats, new_xyz, new_cnt, grid, R, nsample, c_each, chunk=2048):
    """choice (M, G) int32 and new_features (M, G * c_each), plain torch; per scene, `chunk` queries at a time."""
    nx, ny, nz = grid
    G = nx * ny * nz
    dev = xyz.device
    Rt = torch.tensor(R, dtype=torch.float32, device=dev)
    gs = torch.stack([Rt * 2 / n for n in grid])
    out = []
    ps = qs = 0
    for n, m in zip(xyz_cnt, new_cnt):
        p = xyz[ps:ps + n]
        rows = torch.arange(n, device=dev)
        for q0 in range(qs, qs + m, chunk):
            q = new_xyz[q0:min(q0 + chunk, qs + m)]
            loc = p[None] - q[:, None]                                                            # (m, n, 3)
            ok = _in_range(loc, Rt)
            i = torch.floor((loc + Rt) / gs).to(torch.int64)
            cell = (i[..., 0] * ny * nz + i[..., 1] * nz + i[..., 2]).clamp(0, G - 1)
            first = torch.full((len(q), G + 1), n, dtype=torch.int64, device=dev)
            first.scatter_reduce_(1, torch.where(ok, cell, G), rows.expand(len(q), n), reduce="amin")
            first = first[:, :G]                                                                  # the first in-range row of every cell, n = none
            if 0 < nsample < G:                                                                   # the walk stops after nsample taken rows
                kth = first.sort(1).values[:, nsample - 1:nsample]
                first = torch.where(first <= kth, first, n)
            out.append(torch.where(first < n, first + ps, -1))
        ps, qs = ps + n, qs + m
    choice = torch.cat(out).to(torch.int32)
    got = feats[choice.clamp(min=0).long()][..., feats.shape[1] - c_each:]
    return choice, torch.where((choice >= 0)[..., None], got, 0).reshape(len(choice), -1)


def torch_three_nn(xyz, xyz_cnt, new_xyz, centers, new_cnt, R, nsample, chunk=128):
    """dist2 (M, G, 3) over the first min(1000, nsample) in-range rows, plain torch (the indices of tied distances are not compared)."""
    dev = xyz.device
    cap = min(1000, nsample) if nsample > 0 else 1000
    out = []
    ps = qs = 0
    for n, m in zip(xyz_cnt, new_cnt):
        p = xyz[ps:ps + n]
        for q0 in range(qs, qs + m, chunk):
            q, c = new_xyz[q0:min(q0 + chunk, qs + m)], centers[q0:min(q0 + chunk, qs + m)]
            ok = _in_range(p[None] - q[:, None], torch.tensor(R, dtype=torch.float32, device=dev))
            ok &= torch.cumsum(ok, 1) <= cap
            d = c[:, :, None, :] - p[None, None]                                                  # (m, G, n, 3)
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            d2 = torch.where(ok[:, None, :], d2, float("inf"))
            best = torch.topk(d2, 3, dim=-1, largest=False).values
            cnt = ok.sum(1)[:, None]
            best[..., 1] = torch.where(cnt < 2, best[..., 0], best[..., 1])
            best[..., 2] = torch.where(cnt < 3, best[..., 0], best[..., 2])
            out.append(best)
        ps, qs = ps + n, qs + m
    return torch.cat(out)


def torch_interpolate(feats, idx, weight):
    f = feats[idx.long()]                                                                         # (rows, 3, C)
    return weight[:, 0:1] * f[:, 0] + weight[:, 1:2] * f[:, 1] + weight[:, 2:3] * f[:, 2]


def centres(new_xyz, R, grid):
    offs = [torch.arange(-R + R / n, R - R / n + 1e-5, 2 * R / n, device=new_xyz.device) for n in grid]
    off = torch.stack(torch.meshgrid(*offs, indexing="ij"), -1).reshape(-1, 3)
    return (new_xyz[:, None, :] + off[None]).contiguous()


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


def kernels_of_one_call(fn):
    """(launches, summed kernel time in ms) of one call, from torch.profiler; (None, None) where the profiler gives nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        if not ev:
            return None, None
        return len(ev), sum(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) for e in ev) / 1e3
    except Exception as e:                                                                        # the record says so instead of guessing
        print("profiler:", repr(e), file=sys.stderr)
        return None, None


def rehearse():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vector_pool_reference as VR
    lines = []
    for kind in ("roi", "kp"):
        s = SIZES[kind]
        xyz, xc, q, qc, feats = make_inputs(kind, scale=0.01)
        t = [torch.from_numpy(a) for a in (xyz, feats, q)]
        if kind == "roi":
            for nsample in (s["nsample"], 5, -1):
                ch, nf = torch_choice(t[0], xc.tolist(), t[1], t[2], qc.tolist(), s["grid"], s["R"], nsample, s["c_each"], chunk=100)
                want = VR.choice(xyz, xc, feats, q, qc, s["grid"], s["R"], nsample, 0, s["c_each"])
                assert np.array_equal(ch.numpy(), want[0]) and np.array_equal(nf.numpy(), want[3]), "torch statement of the choice differs"
            lines.append(f"rehearsal choice: {len(q)} queries over {len(xyz)} rows, {int((want[0] >= 0).sum())} cells filled: torch statement == restatement")
        else:
            R = np.float32(s["R"] * s["mult"])
            cen = centres(t[2], s["R"], s["grid"])
            for nsample in (-1, 4):
                d2 = torch_three_nn(t[0], xc.tolist(), t[2], cen, qc.tolist(), float(R), nsample, chunk=16)
                idx, want = VR.three_nn(xyz, xc, q, cen.numpy(), qc, R, nsample, 0)
                assert np.array_equal(d2.numpy(), want), "torch statement of the 3-NN differs"
            w = torch.rand(idx.reshape(-1, 3).shape)
            i0 = torch.from_numpy(idx.reshape(-1, 3)).clamp(min=0)
            assert np.array_equal(torch_interpolate(t[1], i0, w).numpy(), VR.interpolate(feats, i0.numpy(), w.numpy()))
            lines.append(f"rehearsal 3-NN + interpolate: {len(q)} queries x 27 centres over {len(xyz)} rows: torch statements == restatement")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        return rehearse()
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm, pointnet2_stack_cuda as ext
    from seevcn_amd.seeding import seeded_state_dict
    assert torch.cuda.is_available(), "vector_pool_micro needs a GPU (--rehearse runs the statements on the CPU)"
    dev = torch.device("cuda:0")
    lines = ["vector pool at pv_rcnn_plusplus.yaml sizes, 2 scenes; per call: median of windows (min .. max), launches and kernel time of one call"]

    differ = []

    def agree(name, got, want):
        n = int((got != want).sum()) if got.shape == want.shape else -1
        if n:
            differ.append(f"{name}: kernel and torch statement differ in {n} of {got.numel()} elements")
            lines.append("!! " + differ[-1])

    def report(name, fn, note="", slow=False):
        windows, calls = (5, 2) if slow else (a.windows, a.calls)                # the chunked torch 3-NN takes a good fraction of a second a call
        for _ in range(1 if slow else 3):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, windows, calls)
        launches, kernel_ms = kernels_of_one_call(fn)
        k = "profiler: not measured" if launches is None else f"{launches} launches, kernel time {kernel_ms:.3f} ms"
        lines.append(f"{name:<58s} median {ms[len(ms) // 2]:9.3f} ms   min {ms[0]:9.3f}   max {ms[-1]:9.3f}   ({len(ms)} x {calls} calls)   {k}   {note}")
        print(lines[-1], flush=True)

    with torch.no_grad():
        # ---- RoI-grid side
        s = SIZES["roi"]
        xyz, xc, q, qc, feats = make_inputs("roi")
        d_xyz, d_xc, d_q, d_qc = (torch.from_numpy(v).to(dev) for v in (xyz, xc, q, qc))
        red = torch.from_numpy(feats).to(dev).view(len(xyz), -1, s["c_each"]).sum(1).contiguous()      # the module's channel-group sum: 90 -> 30
        args = (d_xyz, d_xc, red, d_q, d_qc, *s["grid"], s["R"], s["c_each"], s["nsample"], 0)
        ch, cnt, loc, nf = ext.vector_pool_choice(*args)
        t_ch, t_nf = torch_choice(d_xyz, xc.tolist(), red, d_q, qc.tolist(), s["grid"], s["R"], s["nsample"], s["c_each"])
        agree("choice", ch, t_ch)
        agree("choice features", nf, t_nf)
        filled = float(cnt.float().mean())
        out_mb = (ch.numel() * 8 + loc.numel() * 4 + nf.numel() * 4) / 1e6
        note = f"[{filled * 27:.1f} of 27 cells filled per query; outputs {out_mb:.0f} MB]"
        report("choice   sv_vector_pool_choice (RoI grid, 30 ch)", lambda: ext.vector_pool_choice(*args), note)
        report("choice   plain-torch statement", lambda: torch_choice(d_xyz, xc.tolist(), red, d_q, qc.tolist(), s["grid"], s["R"], s["nsample"], s["c_each"]))
        layer, _ = pm.build_local_aggregation_module(input_channels=s["c_in"], config=C.PVRCNNPP_ROI_GRID_POOL)
        layer.load_state_dict(seeded_state_dict(layer, seed=1))
        layer = layer.to(dev).eval()
        d_feats = torch.from_numpy(feats).to(dev)
        report("module   VectorPoolAggregationModuleMSG ROI_GRID_POOL, eval", lambda: layer(xyz=d_xyz, xyz_batch_cnt=d_xc, new_xyz=d_q, new_xyz_batch_cnt=d_qc,
                                                                                          features=d_feats))
        del layer, t_ch, t_nf, ch, cnt, loc, nf
        # ---- keypoint side
        s = SIZES["kp"]
        xyz, xc, q, qc, feats = make_inputs("kp")
        d_xyz, d_xc, d_q, d_qc = (torch.from_numpy(v).to(dev) for v in (xyz, xc, q, qc))
        for R in (s["R"], 2 * s["R"]):                                                                 # the yaml's two groups of x_conv3: 1.2 and 2.4
            cen = centres(d_q, R, s["grid"])
            Rq = float(np.float32(R * s["mult"]))
            idx, d2 = ext.vector_pool_three_nn(d_xyz, d_xc, d_q, cen, d_qc, Rq, s["nsample"], 0)
            t_d2 = torch_three_nn(d_xyz, xc.tolist(), d_q, cen, qc.tolist(), Rq, s["nsample"])
            agree(f"3-NN dist2 R {R}", d2, t_d2)
            full = float((idx[:, 0, 0] >= 0).float().mean())
            report(f"3-NN     sv_vector_pool_three_nn (R {R} x 2, 27 centres)", lambda: ext.vector_pool_three_nn(d_xyz, d_xc, d_q, cen, d_qc, Rq, s["nsample"], 0),
                   f"[{full * 100:.0f}% of the queries have neighbours]")
            report(f"3-NN     plain-torch statement (R {R} x 2)", lambda: torch_three_nn(d_xyz, xc.tolist(), d_q, cen, qc.tolist(), Rq, s["nsample"]), slow=True)
        red = torch.from_numpy(feats).to(dev).view(len(xyz), -1, s["c_each"]).sum(1).contiguous()      # 64 -> 32
        i3 = idx.view(-1, 3).clamp(min=0).contiguous()
        w = torch.rand(i3.shape, device=dev)
        out = torch.empty((len(i3), s["c_each"]), device=dev)
        ext.three_interpolate_wrapper(red, i3, w, out)
        agree("interpolate", out, torch_interpolate(red, i3, w))
        report("interp   sv_three_interpolate_stack (221 184 rows x 32 ch)", lambda: ext.three_interpolate_wrapper(red, i3, w, out),
               f"[reads + writes {(i3.numel() * 8 + 4 * out.numel() * 4) / 1e6:.0f} MB]")
        report("interp   plain-torch statement", lambda: torch_interpolate(red, i3, w))
        layer, _ = pm.build_local_aggregation_module(input_channels=s["c_in"], config=C.PVRCNNPP_SA_LAYER["x_conv3"])
        layer.load_state_dict(seeded_state_dict(layer, seed=2))
        layer = layer.to(dev).eval()
        d_feats = torch.from_numpy(feats).to(dev)
        report("module   VectorPoolAggregationModuleMSG x_conv3, eval", lambda: layer(xyz=d_xyz, xyz_batch_cnt=d_xc, new_xyz=d_q, new_xyz_batch_cnt=d_qc,
                                                                                    features=d_feats))
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if differ:
        raise SystemExit("\n".join(differ))


if __name__ == "__main__":
    main()
