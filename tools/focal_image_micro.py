#!/usr/bin/env python3
"""Micro-benchmark of the focal image branch's construct_multimodal_features at kitti_models/voxel_rcnn_car_focal_multimodal.yaml's sizes: 2 scenes,
a 375 x 1242 image, 94 x 311 x 16 layer1 features, 16 voxel channels, and the voxels of a KITTI-shaped synthetic scene batch at the input
resolution (the coordinates conv1's submanifold blocks keep; its focal layer adds to them).

Two routes on the same inputs, in this one process, each as the layer calls it -- once as a concat in front of conv_imp, once as a sum behind conv:
  fused       sv_focal_image_pixels + sv_focal_image_sample, backward sv_focal_image_sample_grad (spconv/focal.py)
  reference   a plain-torch statement of focal_sparse_conv.py:50-113: F.interpolate to the image size, then per scene a boolean mask, the voxel
              centres to the host, Calibration.lidar_to_img in numpy float32, the pixels uploaded, indexing, cat; autograd's backward
Per route and call: HIP events around forward and around backward (median of REPS after WARMUP; the reference's host work lies between its
events, as it lies in a training step), torch.cuda.max_memory_allocated above the inputs, and for the fused gradient the longest and the median
key list of a low-resolution pixel.
  python tools/focal_image_micro.py [--out profiles/focal_image.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, IMAGE, FEAT = 2, 16, (375, 1242), (94, 311)
RANGE_ZYX, VOXEL_ZYX = [-3.0, -40.0, 0.0], [0.1, 0.05, 0.05]
WARMUP, REPS = 3, 10
# KITTI object benchmark, calib/000000.txt
P2 = [[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01], [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01], [0.0, 0.0, 1.0, 2.745884e-03]]
R0 = [[9.999239e-01, 9.837760e-03, -7.445048e-03], [-9.869795e-03, 9.999421e-01, -4.278459e-03], [7.402527e-03, 4.351614e-03, 9.999631e-01]]
V2C = [[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03], [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
       [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]]


def reference_route(f, x_rgb, indices, calibs, batch_dict, fuse_sum, consts):
    """focal_sparse_conv.py:62-113, statement for statement, on the device where the reference is and on the host where it is"""
    import torch
    import torch.nn.functional as F
    from seevcn_amd.pcdet.utils import common_utils
    dev = f.device
    inv_idx, voxel_size, origin = consts                     # attributes of the reference's layer (:46-48)
    batch_index = indices[:, 0]
    voxels_3d = indices[:, 1:] * voxel_size + origin
    h, w = IMAGE
    if tuple(x_rgb.shape[2:]) != (h, w):
        x_rgb = F.interpolate(x_rgb, (h, w), mode='bilinear')
    rows = []
    for b in range(B):
        mask = batch_index == b
        v3 = voxels_3d[mask]
        fb = f[mask]
        v3 = v3 / batch_dict['noise_scale'][b]
        v3 = common_utils.rotate_points_along_z(v3[:, inv_idx].unsqueeze(0), -batch_dict['noise_rot'][b].unsqueeze(0))[0, :, inv_idx]
        v3[:, 1] *= -1 if batch_dict['flip_x'][b] else 1
        v3[:, 2] *= -1 if batch_dict['flip_y'][b] else 1
        v2, _ = calibs[b].lidar_to_img(v3[:, inv_idx].cpu().numpy())
        v2 = torch.Tensor(v2).to(dev).long()
        keep = (0 <= v2[:, 1]) * (v2[:, 1] < h) * (0 <= v2[:, 0]) * (v2[:, 0] < w)
        v2 = v2[keep]
        img = torch.zeros((fb.shape[0], x_rgb.shape[1]), device=dev)
        img[keep] = x_rgb[b][:, v2[:, 1], v2[:, 0]].permute(1, 0)
        rows.append(img + fb if fuse_sum else torch.cat([img, fb], dim=1))
    return torch.cat(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.ops import voxel_ops
    from seevcn_amd.pcdet.utils import calibration_kitti
    from seevcn_amd.spconv import focal
    assert torch.cuda.is_available(), "tools/focal_image_micro.py needs a GPU"
    dev = torch.device("cuda:0")
    pts, _ = synth.make_scene_batch(B, seed=2000)
    _, coords, _ = voxel_ops.voxelize_dynamic(torch.from_numpy(pts).to(dev).contiguous(), [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1], [1408, 1600, 40], B)
    coords = coords.int().contiguous()
    n = coords.shape[0]
    calib = calibration_kitti.Calibration({"P2": np.array(P2, np.float32), "R0": np.array(R0, np.float32), "Tr_velo2cam": np.array(V2C, np.float32)})
    calibs = [calib] * B
    batch_dict = {"noise_scale": torch.tensor([0.97, 1.04], device=dev), "noise_rot": torch.tensor([0.31, -0.52], device=dev),
                  "flip_x": torch.tensor([True, False], device=dev), "flip_y": torch.tensor([False, False], device=dev)}
    torch.manual_seed(0)
    f0 = torch.randn((n, C), device=dev)
    rgb0 = torch.randn((B, C) + FEAT, device=dev)
    # in scene order the two routes give the same rows (the reference concatenates scene after scene)
    order = torch.argsort(coords[:, 0].long(), stable=True)
    coords, f0 = coords[order].contiguous(), f0[order].contiguous()
    calib_table = calibration_kitti.pack_calib(calibs, dev)
    aug_table = focal.image_aug_table(batch_dict, B, dev)
    consts = (torch.tensor([2, 1, 0], device=dev), torch.tensor(VOXEL_ZYX, device=dev), torch.tensor(RANGE_ZYX, device=dev))

    def fused_route(f, x_rgb, fuse_sum):
        pix = focal.focal_image_pixels(coords, B, 1, VOXEL_ZYX, RANGE_ZYX, calib_table, aug_table, IMAGE)
        return focal.focal_image_fuse(f, x_rgb.permute(0, 2, 3, 1).contiguous(), coords, pix, IMAGE, fuse_sum)

    pix = focal.focal_image_pixels(coords, B, 1, VOXEL_ZYX, RANGE_ZYX, calib_table, aug_table, IMAGE).long()
    ok = pix >= 0
    v, u = pix[ok] // IMAGE[1], pix[ok] % IMAGE[1]
    scene = coords[ok, 0].long()
    counts = torch.zeros(B * FEAT[0] * FEAT[1], dtype=torch.int64, device=dev)
    for dy in (0, 1):
        for dx in (0, 1):
            sy = (FEAT[0] * (2 * v + 1) - IMAGE[0]).clamp(min=0) // (2 * IMAGE[0])
            sx = (FEAT[1] * (2 * u + 1) - IMAGE[1]).clamp(min=0) // (2 * IMAGE[1])
            y, x = sy + dy * (sy < FEAT[0] - 1), sx + dx * (sx < FEAT[1] - 1)
            counts += torch.bincount((scene * FEAT[0] + y) * FEAT[1] + x, minlength=counts.numel())
    lines = [f"focal image branch, construct_multimodal_features: {B} scenes, image {IMAGE[0]} x {IMAGE[1]}, features {FEAT[0]} x {FEAT[1]} x {C}, "
             f"{C} voxel channels, n = {n} voxels ({int(ok.sum())} project into the image), fp32; ms, HIP events, median of {REPS} after {WARMUP} warm-ups; "
             f"both routes in one process",
             "fused = sv_focal_image_pixels + sv_focal_image_sample (+ _sample_grad); reference = F.interpolate + per-scene host projection + indexing + "
             "autograd", "",
             f"{'call':7s} {'route':10s} {'forward':>9s} {'backward':>9s} {'peak above inputs':>18s}"]
    for fuse_sum in (False, True):
        outs = {}
        gout = torch.randn((n, C if fuse_sum else 2 * C), device=dev)
        for route in ("fused", "reference"):
            f, x_rgb = f0.clone().requires_grad_(True), rgb0.clone().requires_grad_(True)

            def forward():
                if route == "fused":
                    return fused_route(f, x_rgb, fuse_sum)
                return reference_route(f, x_rgb, coords, calibs, batch_dict, fuse_sum, consts)

            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tf, tb = [], []
            for it in range(WARMUP + REPS):
                f.grad = x_rgb.grad = None
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
                    del out
            peak = torch.cuda.max_memory_allocated() - base
            outs[route] = (out.detach().clone(), f.grad.clone(), x_rgb.grad.clone())
            lines.append(f"{'sum' if fuse_sum else 'concat':7s} {route:10s} {np.median(tf):9.3f} {np.median(tb):9.3f} {peak / 1e6:15.1f} MB")
            del out, f, x_rgb
            torch.cuda.empty_cache()
        same_pixels = (outs["fused"][0] - outs["reference"][0]).abs().amax(dim=1) < 1e-3
        diff = [float((a - b).abs().max()) for a, b in ((outs["fused"][0][same_pixels], outs["reference"][0][same_pixels]), (outs["fused"][1], outs["reference"][1]))]
        lines.append(f"   {'sum' if fuse_sum else 'concat'}: rows whose two routes agree to 1e-3 (the same pixel) {int(same_pixels.sum())} of {n}; on them max |fused - "
                     f"reference| {diff[0]:.2e}; grad f {diff[1]:.2e}; grad features, relative to its largest entry "
                     f"{float((outs['fused'][2] - outs['reference'][2]).abs().max() / outs['reference'][2].abs().max()):.2e}")
        del outs
        torch.cuda.empty_cache()
    lines.append(f"keys per low-resolution pixel list of the fused gradient: max {int(counts.max())}, median {int(counts.median())}, "
                 f"pixels without a key {int((counts == 0).sum())} of {counts.numel()}, keys {int(counts.sum())}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
