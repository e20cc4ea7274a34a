#!/usr/bin/env python3
"""Micro-benchmark of CaDDN's frustum -> voxel sampling at kitti_models/CaDDN.yaml's sizes: C = 64, D = 80 (+1 bin), a 94 x 311 feature map of a
376 x 1244 image, a 280 x 376 x 25 grid over [2, -30.08, -3, 46.8, 30.08, 1], LID bins, B = 1 and 2.

Two routes through FrustumToVoxel on the same inputs, in this one process:
  fused   sv_frustum_to_voxel / sv_frustum_to_voxel_grad on image_features and depth_probs
  tree    SEEVCN_FUSED_FRUSTUM=0: the (B, C, D, H, W) volume (depth_probs[:, :-1] * image_features, as DepthFFN.create_frustum_features builds it),
          sv_frustum_grid, the 5-D F.grid_sample and autograd's backward of both
Per route and size: HIP events around forward and around backward (median of REPS after WARMUP), torch.cuda.max_memory_allocated above the inputs,
kernel launches per forward + backward (torch.profiler; "n/a" where it is not available), and for the fused gradient the longest and the median
key list of a pixel.
  python tools/frustum_sample_micro.py [--out profiles/frustum_sample.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, D, H, W = 64, 80, 94, 311
IMAGE = (376, 1244)
GRID, RANGE = (280, 376, 25), (2.0, -30.08, -3.0, 46.8, 30.08, 1.0)
DISC = dict(mode="LID", num_bins=D, depth_min=2.0, depth_max=46.8)
WARMUP, REPS = 3, 10


def calibration(B, dev):
    """a KITTI-like camera: the LiDAR -> camera axis swap with the sensor offset, P2 with fx = fy = 721.5"""
    import torch
    l2c = torch.tensor([[0., -1., 0., 0.0], [0., 0., -1., -0.08], [1., 0., 0., -0.27], [0., 0., 0., 1.]], device=dev)
    c2i = torch.tensor([[721.5, 0., 609.6, 44.9], [0., 721.5, 172.9, 0.22], [0., 0., 1., 0.0027]], device=dev)
    return l2c.repeat(B, 1, 1), c2i.repeat(B, 1, 1), torch.tensor([IMAGE] * B, dtype=torch.int32, device=dev)


def list_lengths(l2c, c2i, ishape):
    """keys per pixel of the fused gradient, from the sampling grid: a key per pixel tap inside the map of a voxel with a depth tap inside"""
    import torch
    from seevcn_amd.pcdet.ops import frustum_ops
    g = frustum_ops.frustum_grid(l2c, c2i, ishape, GRID, RANGE, DISC)
    B = g.shape[0]
    ix, iy, iz = ((g[..., k] + 1) / 2 * (n - 1) for k, n in enumerate((W, H, D)))
    x0, y0, z0 = torch.floor(ix), torch.floor(iy), torch.floor(iz)
    depth_in = ((z0 >= 0) & (z0 <= D - 1)) | ((z0 >= -1) & (z0 <= D - 2))
    counts = torch.zeros(B * H * W, dtype=torch.int64, device=g.device)
    base = (torch.arange(B, device=g.device) * H * W).view(B, 1, 1, 1)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = depth_in & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
            pix = (base + y.clamp(0, H - 1).long() * W + x.clamp(0, W - 1).long())[ok]
            counts += torch.bincount(pix, minlength=B * H * W)
    return int(counts.max()), int(counts.median()), int(counts.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from seevcn_amd.pcdet.models.backbones_3d.vfe.image_vfe_modules.f2v import FrustumToVoxel
    assert torch.cuda.is_available(), "tools/frustum_sample_micro.py needs a GPU"
    dev = torch.device("cuda:0")
    m = FrustumToVoxel(dict(NAME="FrustumToVoxel", SAMPLER=dict(mode="bilinear", padding_mode="zeros")), grid_size=GRID, pc_range=RANGE, disc_cfg=DISC).to(dev)
    lines = [f"CaDDN frustum -> voxel sampling, C = {C}, D = {D} (+1), map {H} x {W}, grid {GRID[0]} x {GRID[1]} x {GRID[2]}, LID, fp32; ms, HIP events, median of "
             f"{REPS} after {WARMUP} warm-ups; both routes in one process",
             "fused = sv_frustum_to_voxel(+_grad); tree = SEEVCN_FUSED_FRUSTUM=0: volume + sv_frustum_grid + 5-D grid_sample + autograd", "",
             f"{'B':>2s} {'route':6s} {'forward':>9s} {'backward':>9s} {'peak above inputs':>18s} {'launches fwd+bwd':>17s}"]
    for B in (1, 2):
        torch.manual_seed(B)
        l2c, c2i, ishape = calibration(B, dev)
        feats0 = torch.randn((B, C, H, W), device=dev).contiguous(memory_format=torch.channels_last)
        probs0 = torch.softmax(torch.randn((B, D + 1, H, W), device=dev), dim=1).contiguous(memory_format=torch.channels_last)
        gout = torch.randn((B, GRID[1], GRID[0], C, GRID[2]), device=dev).permute(0, 3, 4, 1, 2)       # in the fused output's storage order
        kmax, kmed, ktot = list_lengths(l2c, c2i, ishape)
        outs = {}
        for route in ("fused", "tree"):
            os.environ["SEEVCN_FUSED_FRUSTUM"] = "1" if route == "fused" else "0"
            feats, probs = feats0.clone().requires_grad_(True), probs0.clone().requires_grad_(True)

            def forward():
                d = dict(trans_lidar_to_cam=l2c, trans_cam_to_img=c2i, image_shape=ishape)
                if route == "fused":
                    d.update(image_features=feats, depth_probs=probs)
                else:
                    d.update(frustum_features=probs.unsqueeze(1)[:, :, :-1] * feats.unsqueeze(2))
                return m(d)["voxel_features"]

            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tf, tb = [], []
            for it in range(WARMUP + REPS):
                feats.grad = probs.grad = None
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                out = forward()
                e[1].record()
                out.backward(gout)
                e[2].record()
                torch.cuda.synchronize()
                if it >= WARMUP:
                    tf.append(e[0].elapsed_time(e[1]))
                    tb.append(e[1].elapsed_time(e[2]))
                if it + 1 < WARMUP + REPS:
                    del out                                                # or the next forward's output is allocated beside this one
            peak = torch.cuda.max_memory_allocated() - base
            outs[route] = (out.detach().clone(), feats.grad.clone(), probs.grad.clone())
            try:
                from torch.profiler import ProfilerActivity, profile
                feats.grad = probs.grad = None
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    forward().backward(gout)
                    torch.cuda.synchronize()
                from torch.autograd import DeviceType
                launches = str(sum(ev.count for ev in prof.key_averages() if ev.device_type == DeviceType.CUDA))      # kernels, memsets and copies
            except Exception as ex:                                        # the profiler is an extra here, not the measurement
                launches = "n/a"
                print("profiler unavailable:", type(ex).__name__, ex, file=sys.stderr)
            lines.append(f"{B:2d} {route:6s} {np.median(tf):9.3f} {np.median(tb):9.3f} {peak / 1e6:15.1f} MB {launches:>17s}")
            del out, feats, probs
            torch.cuda.empty_cache()
        diff = [float((a - b).abs().max()) for a, b in zip(outs["fused"], outs["tree"])]
        lines.append(f"   B = {B}: keys per pixel list max {kmax}, median {kmed}, total {ktot} of {4 * B * GRID[0] * GRID[1] * GRID[2]} possible; "
                     f"max |fused - tree|: out {diff[0]:.2e}, grad features {diff[1]:.2e}, grad probs {diff[2]:.2e}")
        del outs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
