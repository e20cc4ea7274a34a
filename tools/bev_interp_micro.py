#!/usr/bin/env python3
"""Micro-benchmark of VoxelSetAbstraction's BEV source (forward + backward of _BevInterp) on a channels_last map, the layout HeightCompression hands
over from 8 scenes on: 8 and 16 KITTI-shaped scenes (200 x 176 cells, C = 256), 2048 and 4096 keypoints per scene.

Two arms on the same input:
  nhwc  the channel-last entries (SEEVCN_BEV_INTERP_NHWC=1): one pass each way, the gradient written in channels_last strides
  nchw  the route before them (SEEVCN_BEV_INTERP_NHWC=0), its layout copies included: channels_last -> NCHW copy, NCHW entries (memset, float
        atomics, transpose), NCHW gradient
In both arms the leaf already holds a channels_last gradient (the 2-D backbone's, in the detector), so the backward ends in autograd's accumulation
into it -- for the nchw arm that is where the second layout conversion is paid.

The arms run in alternating child processes, their order rotated from round to round; each child times every size (HIP events around REPS
forward + backward pairs after WARMUP pairs, the per-pair median).  The parent process never touches the GPU.
  python tools/bev_interp_micro.py [--rounds 3] [--out profiles/bev_interp_nhwc.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(8, 2048), (8, 4096), (16, 2048), (16, 4096)]           # (scenes, keypoints per scene)
C, H, W = 256, 200, 176
RANGE, VOXEL, STRIDE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], [0.05, 0.05, 0.1], 8
WARMUP, REPS = 5, 20


def child():
    import numpy as np
    import torch
    from seevcn_amd.pcdet.models.backbones_3d.pfe import voxel_set_abstraction as vsa_mod
    assert torch.cuda.is_available(), "tools/bev_interp_micro.py needs a GPU"
    dev = torch.device("cuda:0")
    want = "nhwc" if vsa_mod.BEV_INTERP_NHWC else "nchw"
    res = {}
    for scenes, nkp in SIZES:
        rng = np.random.RandomState(scenes * 10000 + nkp)
        m = scenes * nkp
        kps = np.stack([np.repeat(np.arange(scenes), nkp), rng.uniform(RANGE[0], RANGE[3], m), rng.uniform(RANGE[1], RANGE[4], m),
                        rng.uniform(RANGE[2], RANGE[5], m)], axis=1).astype(np.float32)
        kps = torch.from_numpy(kps).to(dev)
        leaf = torch.randn((scenes, C, H, W), device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        leaf.grad = torch.randn((scenes, C, H, W), device=dev).contiguous(memory_format=torch.channels_last)
        gout = torch.randn((m, C), device=dev)

        def pair():
            out = vsa_mod._BevInterp.apply(leaf, kps, RANGE[0], RANGE[1], VOXEL[0], VOXEL[1], STRIDE)
            out.backward(gout)

        for _ in range(WARMUP):
            pair()
        assert vsa_mod.VoxelSetAbstraction.last_bev_layout == want and leaf.grad.is_contiguous(memory_format=torch.channels_last)
        times = []
        for _ in range(REPS):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            pair()
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e) * 1e3)
        res[f"{scenes}x{nkp}"] = {"median_us": float(np.median(times)), "min_us": float(np.min(times))}
        del leaf, gout, kps
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps({"arm": want, "sizes": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    arms = ["nhwc", "nchw"]
    runs = {a: [] for a in arms}
    order_log = []
    for r in range(args.rounds):
        order = arms[r % 2:] + arms[:r % 2]
        order_log.append(" ".join(order))
        for arm in order:
            env = dict(os.environ, SEEVCN_BEV_INTERP_NHWC="1" if arm == "nhwc" else "0")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:                         # a failed arm ends the run: nothing more is started on the device
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"arm {arm} round {r} failed with exit status {p.returncode}")
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            assert got["arm"] == arm
            runs[arm].append(got["sizes"])
    lines = [f"VoxelSetAbstraction BEV source, forward + backward on a channels_last map (B, {C}, {H}, {W}), fp32; us per pair, HIP events, median of {REPS}",
             f"after {WARMUP} warm-up pairs; one child process per arm and round, order per round: " + " | ".join(order_log),
             "nhwc = channel-last entries; nchw = SEEVCN_BEV_INTERP_NHWC=0 (copy to NCHW, NCHW entries, NCHW gradient accumulated into the channels_last one)",
             "", f"{'scenes x keypoints':20s} {'arm':5s} " + " ".join(f"round{r:<3d}" for r in range(args.rounds)) + "   spread    nchw / nhwc (medians of rounds)"]
    for scenes, nkp in SIZES:
        key = f"{scenes}x{nkp}"
        med = {}
        for arm in arms:
            t = [run[key]["median_us"] for run in runs[arm]]
            med[arm] = sorted(t)[len(t) // 2]
            tail = f"   {med['nchw'] / med['nhwc']:.2f}x" if arm == "nchw" else ""
            lines.append(f"{key:20s} {arm:5s} " + " ".join(f"{x:8.1f}" for x in t) + f"   {max(t) - min(t):6.1f}" + tail)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
