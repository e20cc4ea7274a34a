"""VoxelRCNNHead eval forward at voxel_rcnn_car.yaml sizes (2 scenes, 100 RoIs a scene, x_conv2 / x_conv3 / x_conv4): the fused route against the
module tree (what SEEVCN_FUSED_VOXEL_POOL=0 selects), alternating in one process, and the voxel query kernel alone per source.  Device events
around batches of calls behind a warm-up; medians with the spread over the batches.  Needs a GPU (--rehearse: build the inputs and the head, stop).

    python tools/voxel_rcnn_head_micro.py [--out profiles/voxel_rcnn_head.txt] [--n-az 400] [--batches 15] [--calls 10]
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seevcn_amd.synth as synth  # noqa: E402
from seevcn_amd.pcdet import model_cfgs as C  # noqa: E402
from seevcn_amd.seeding import seeded_state_dict  # noqa: E402

TAPS = {'x_conv2': (2, 32, [21, 800, 704]), 'x_conv3': (4, 64, [11, 400, 352]), 'x_conv4': (8, 64, [5, 200, 176])}
VOXEL_SIZE = [0.05, 0.05, 0.1]


def make_inputs(n_az):
    rng = np.random.default_rng(5)
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=n_az)
    out = {}
    vs, rg = np.array(VOXEL_SIZE), np.array(C.KITTI_RANGE[:3])
    for name, (factor, ch, shape) in TAPS.items():
        c = np.floor((pts[:, 1:4] - rg) / (vs * factor)).astype(np.int32)
        ok = (c >= 0).all(1) & (c[:, 0] < shape[2]) & (c[:, 1] < shape[1]) & (c[:, 2] < shape[0])
        idx = np.unique(np.concatenate([pts[ok, 0:1].astype(np.int32), c[ok][:, [2, 1, 0]]], 1), axis=0)
        out[name] = (idx.astype(np.int32), rng.normal(size=(len(idx), ch)).astype(np.float32))
    boxes = []
    for b in range(2):
        g = gt[b][gt[b, :, 3] > 0][:, :7]
        rep = np.repeat(g, 40, axis=0) + rng.normal(0, 1, (len(g) * 40, 7)).astype(np.float32) * np.array([0.5, 0.5, 0.1, 0.1, 0.05, 0.05, 0.3], np.float32)
        rnd = np.concatenate([rng.uniform([0, -40, -2], [70, 40, 0], (400, 3)), rng.uniform([1.5, 0.6, 1.2], [4.5, 2, 2], (400, 3)),
                              rng.uniform(-3, 3, (400, 1))], 1).astype(np.float32)
        boxes.append(np.concatenate([rep, rnd])[:800])
    n = min(len(b) for b in boxes)
    out['batch_box_preds'] = np.stack([b[:n] for b in boxes]).astype(np.float32)
    out['batch_cls_preds'] = rng.normal(size=(2, n, 1)).astype(np.float32)
    return out


def timed(fn, batches, calls):
    """ms per call of fn(): `batches` windows of `calls` calls each between two device events -> sorted list"""
    ms = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return sorted(ms)


def fmt(name, ms):
    return f"{name:<44s} median {ms[len(ms) // 2]:8.3f} ms   min {ms[0]:8.3f}   max {ms[-1]:8.3f}   ({len(ms)} windows)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-az", type=int, default=400)
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    from seevcn_amd.pcdet.models import roi_heads
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda, voxel_pool_modules
    from seevcn_amd.pcdet.utils import common_utils
    inp = make_inputs(a.n_az)
    rh = roi_heads.__all__["VoxelRCNNHead"](backbone_channels={k: v[1] for k, v in TAPS.items()}, model_cfg=C.voxelrcnn_cfg(),
                                            point_cloud_range=np.array(C.KITTI_RANGE, np.float32), voxel_size=VOXEL_SIZE, num_class=1)
    rh.load_state_dict(seeded_state_dict(rh, seed=13))
    lines = [f"VoxelRCNNHead eval forward, voxel_rcnn_car.yaml sizes: 2 scenes, 100 RoIs a scene (2 x 100 x 216 = 43200 grid points), proposals {inp['batch_box_preds'].shape[1]} a scene",
             "support voxels: " + ", ".join(f"{k} {len(inp[k][0])}" for k in TAPS)]
    if a.rehearse:
        print("\n".join(lines))
        return
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    rh = rh.to(dev).eval()
    t = lambda x: torch.from_numpy(x).to(dev)
    taps = {k: SimpleNamespace(indices=t(inp[k][0]), features=t(inp[k][1]), spatial_shape=TAPS[k][2], batch_size=2) for k in TAPS}
    box, cls = t(inp['batch_box_preds']), t(inp['batch_cls_preds'])

    def forward(off):
        voxel_pool_modules.FUSED_VOXEL_POOL_OFF = off
        bd = {"batch_size": 2, "multi_scale_3d_features": taps, "multi_scale_3d_strides": {k: v[0] for k, v in TAPS.items()}, "batch_cls_preds": cls,
              "batch_box_preds": box, "cls_preds_normalized": False}
        with torch.no_grad():
            return rh(bd)

    out_f, out_t = forward(False)["batch_box_preds"].clone(), forward(True)["batch_box_preds"].clone()
    lines.append(f"fused vs module tree, batch_box_preds: max |diff| {float((out_f - out_t).abs().max()):.3e} (largest value {float(out_t.abs().max()):.3e})")
    for _ in range(5):
        forward(False), forward(True)
    torch.cuda.synchronize()
    fused, tree = [], []
    for _ in range(a.batches):                                    # alternating windows: both routes see the same machine
        fused += timed(lambda: forward(False), 1, a.calls)
        tree += timed(lambda: forward(True), 1, a.calls)
    lines += [fmt("head eval forward, fused route", sorted(fused)), fmt("head eval forward, module tree (switch = 0)", sorted(tree))]
    # the query kernel alone, per source, on the RoIs the head pooled
    rois = forward(False)["rois"]
    grid, _ = rh.get_global_grid_points_of_roi(rois, grid_size=6)
    grid = grid.view(2, -1, 3)
    coords = torch.cat([(grid[:, :, k:k + 1] - float(C.KITTI_RANGE[k])) // VOXEL_SIZE[k] for k in range(3)], dim=-1)
    bcol = torch.arange(2, device=dev, dtype=grid.dtype).view(-1, 1, 1).expand(-1, grid.shape[1], 1)
    new_xyz = grid.contiguous().view(-1, 3)
    for k, (factor, _, shape) in TAPS.items():
        cur = torch.cat([bcol, (coords // factor).flip(-1)], dim=-1).int().view(-1, 4).contiguous()            # [b, z, y, x]
        xyz = common_utils.get_voxel_centers(taps[k].indices[:, 1:4], factor, VOXEL_SIZE, np.array(C.KITTI_RANGE, np.float32)).contiguous()
        vol = common_utils.generate_voxel2pinds(taps[k])
        radius = {2: 0.4, 4: 0.8, 8: 1.6}[factor]
        idx = torch.zeros((new_xyz.shape[0], 16), dtype=torch.int32, device=dev)
        call = lambda: pointnet2_stack_cuda.voxel_query_wrapper(new_xyz.shape[0], *shape, 16, radius, 4, 4, 4, new_xyz, xyz, cur, vol, idx)
        for _ in range(5):
            call()
        ms = timed(call, a.batches, a.calls * 5)
        empty = float((idx[:, 0] < 0).float().mean())
        lines.append(fmt(f"voxel query alone, {k} (range 4, nsample 16)", ms) + f"   empty queries {100 * empty:.1f} %")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
