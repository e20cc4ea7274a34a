"""BASELINE configs 4 and 5 at their full size (inputs: tests/config_inputs.py), each run through the registered detector and checked against
the oracle where the oracle can follow (indices bit-exact, features element-wise per channel, tests/tolerances.py) and through size-independent
properties elsewhere.  The reference cannot run these (spconv and the CUDA ops are absent): parity for the sparse stages is
against oracle/spconv.py (unpinned restatement, cross-checked against torch conv3d in tests/test_spconv.py)."""
import numpy as np
import pytest
import torch

import config_inputs as ci
from oracle import boxes as ob, hard_voxelize as ohv, pointnet2 as op2, spconv as osp
from seeding import seeded_state_dict
from tolerances import assert_close_per_channel
from seevcn_amd.pcdet import model_cfgs as C


# ------------------------------------------------------------------------------------------ config 5: CenterPoint, VoxelResBackBone8x, 300 k points
@pytest.mark.gpu
def test_hip_centerpoint_res_backbone_at_config5_size(cuda, hip_lib):
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.pcdet.ops import voxel_ops
    pts, gt = ci.centerpoint_scene(n_az=1200)
    assert 280_000 <= len(pts) <= 330_000, len(pts)
    pts = pts[np.random.default_rng(0).permutation(len(pts))]                      # DataProcessor.shuffle_points (data_processor.py:146-154)
    grid = np.round((np.array(ci.NUSC_RANGE[3:]) - np.array(ci.NUSC_RANGE[:3])) / np.array(ci.NUSC_VOXEL)).astype(np.int64)
    assert list(grid) == [1440, 1440, 40]
    # D1 at full size: GPU hard voxeliser == sequential first-come oracle, bit-exact (coords, slot order, counts)
    vox, crd, nmp, nv = voxel_ops.voxelize_hard(torch.from_numpy(pts).to(cuda), 0, 3, [len(pts)], ci.NUSC_RANGE, ci.NUSC_VOXEL, grid, 10, 120000)
    ov, oc, on = ohv.points_to_voxel(pts, ci.NUSC_VOXEL, ci.NUSC_RANGE, 10, 120000)
    n = int(nv[0])
    assert n == len(oc) and np.array_equal(crd[0, :n].cpu().numpy(), oc) and np.array_equal(nmp[0, :n].cpu().numpy(), on)
    assert np.array_equal(vox[0, :n].cpu().numpy(), ov) and int(on.max()) == 10            # the 10-points-per-voxel cap is exercised
    coords = torch.cat([torch.zeros((n, 1), dtype=torch.int32, device=cuda), crd[0, :n]], dim=1)

    ds = C.SyntheticDatasetInfo(class_names=C.NUSC_CLASS_NAMES, point_cloud_range=ci.NUSC_RANGE, voxel_size=ci.NUSC_VOXEL, num_point_features=3)
    net = detectors.build_detector(C.centerpoint_model_cfg(), num_class=10, dataset=ds)
    assert type(net.backbone_3d).__name__ == "VoxelResBackBone8x" and type(net.dense_head).__name__ == "CenterHead"
    sd = seeded_state_dict(net, seed=21)
    net.load_state_dict(sd)
    net = net.to(cuda)
    gt10 = np.concatenate([gt[:, :7], np.zeros((len(gt), 2), np.float32), gt[:, 7:8]], axis=1)[None]          # [box7, vx, vy, class]
    batch = {"batch_size": 1, "voxels": vox[0, :n].contiguous(), "voxel_coords": coords, "voxel_num_points": nmp[0, :n].contiguous(),
             "gt_boxes": torch.from_numpy(gt10).to(cuda)}

    # eval: every level of the residual backbone against the oracle chain (eval-mode BN), coordinates bit-exact
    net.eval()
    with torch.no_grad():
        bd = dict(batch)
        for m in net.module_list[:2]:                                              # MeanVFE, VoxelResBackBone8x
            bd = m(bd)
    feats = (ov.astype(np.float64).sum(1) / np.maximum(on, 1)[:, None]).astype(np.float32)
    np.testing.assert_allclose(bd["voxel_features"].cpu().numpy(), feats, rtol=1e-6, atol=1e-6)
    bsd = {k[len("backbone_3d."):]: v.numpy() for k, v in sd.items() if k.startswith("backbone_3d.")}
    ref = osp.voxel_res_backbone8x_forward(bsd, bd["voxel_features"].cpu().numpy(), coords.cpu().numpy(), 1, net.backbone_3d.sparse_shape)
    for name in ("x_conv1", "x_conv2", "x_conv3", "x_conv4"):
        t = bd["multi_scale_3d_features"][name]
        f, c, shape = ref[name]
        assert list(t.spatial_shape) == list(shape) and np.array_equal(t.indices.cpu().numpy(), c), name
        assert_close_per_channel(t.features.cpu().numpy(), f, name=name)
    t = bd["encoded_spconv_tensor"]
    f, c, shape = ref["out"]
    assert list(t.spatial_shape) == [2, 180, 180] == list(shape) and np.array_equal(t.indices.cpu().numpy(), c)
    assert_close_per_channel(t.features.cpu().numpy(), f, name="conv_out")
    assert bd["multi_scale_3d_features"]["x_conv4"].features.shape[1] == 128           # the 128 -> 128 residual layers ran

    # whole detector: train step (targets, losses, backward through the residual blocks) and eval decode.  The backward of the residual backbone is held to
    # the float64 oracle for the sampled stages below (tests/test_spconv.py holds ALL of it on 2 scenes); the other layers are checked for finite, non-zero gradients.
    from oracle import spconv_train as ost
    from test_spconv import HINT_BAND, HINT_CAP, _check_conv_bias_gradients, _res_branch_hooks
    net.train()
    taps, branches = {}, {}

    def keep_taps(_m, _i, out):                                                  # the stage boundaries of THIS step, their gradients retained
        taps.update(out["multi_scale_3d_features"])
        taps["out"] = out["encoded_spconv_tensor"]
        for name in ("x_conv3", "x_conv4", "out"):
            taps[name].features.retain_grad()

    hooks = _res_branch_hooks(net.backbone_3d, branches, only=("conv4", "conv_out")) + [net.backbone_3d.register_forward_hook(keep_taps)]
    ret, tb, _ = net(dict(batch))
    for h in hooks:
        h.remove()
    assert torch.isfinite(ret["loss"]) and "rpn_loss" in tb
    ret["loss"].backward()
    grads = {k: p.grad for k, p in net.backbone_3d.named_parameters()}
    for key in ("conv4.1.conv1.weight", "conv4.2.conv2.weight", "conv1.0.conv1.bias", "conv_out.0.weight"):
        g = grads[key]
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, key
    # sampled stages at this size, the step's own tensors on both sides (as test_hip_train_step_gradients_of_sampled_stages_at_16_scenes does for the plain
    # backbone): x_conv3 -> x_conv4 = the 64 -> 128 strided block + two 128-channel SparseBasicBlocks, x_conv4 -> out = conv_out.  Stage output, input gradient and
    # every conv weight / BatchNorm gradient per channel; the conv biases by the rounding-noise bound of tests/test_spconv.py; ReLU branches as hints within 1e-4.
    import time
    stages = [("x_conv3", "x_conv4", [("conv4.0.0.weight", "conv4.0.1", "sparse", 3, 2, (0, 1, 1)), ("basic", "conv4.1"), ("basic", "conv4.2")], 3 + 2 * 6),
              ("x_conv4", "out", [("conv_out.0.weight", "conv_out.1", "sparse", (3, 1, 1), (2, 1, 1), 0)], 3)]
    for src, dst, layers, n_params in stages:
        t0 = time.time()
        xin, yout = taps[src], taps[dst]
        assert xin.features.grad is not None and yout.features.grad is not None, (src, dst)
        prefixes = tuple(l[1] if l[0] == "basic" else l[0].rsplit(".0.weight", 1)[0] for l in layers)
        hints = {k: v for k, v in branches.items() if k.startswith(prefixes)}
        assert len(hints) == sum(2 if l[0] == "basic" else 1 for l in layers), sorted(hints)
        ref, leaves, oc, oshape, info = ost.res_stage_train_chain(bsd, layers, xin.features.detach().cpu().numpy(), xin.indices.cpu().numpy(), xin.spatial_shape,
                                                                  branch_hints=hints, hint_band=HINT_BAND)
        assert info["hinted"] == sum(h.size for h in hints.values()) and info["overridden"] <= HINT_CAP * info["hinted"], (dst, info["overridden"], info["hinted"])
        assert np.array_equal(yout.indices.cpu().numpy(), oc) and list(yout.spatial_shape) == list(oshape), dst
        assert_close_per_channel(yout.features.detach().cpu().numpy(), ref.detach().numpy(), name=f"res {dst} features (config 5, train)")
        ref.backward(yout.features.grad.detach().cpu().double())
        assert_close_per_channel(xin.features.grad.cpu().numpy(), leaves["input"].grad.numpy(), rtol=2e-3, atol_frac=2e-4, name=f"res d loss / d {src} (config 5)")
        checked, bias_grads = 0, {}
        for k in leaves:
            if k == "input":
                continue
            got = grads[k].detach().cpu().numpy()
            if k.endswith(".bias") and ".conv" in k:
                bias_grads[k] = got
                continue
            assert_close_per_channel(osp.weight_to_kio(got) if got.ndim == 5 else got, leaves[k].grad.numpy(), rtol=2e-3, atol_frac=2e-3, name=f"res grad {k} (config 5)")
            checked += 1
        needed = []
        assert checked + _check_conv_bias_gradients(bias_grads, info, needed) == n_params + (4 if n_params > 3 else 0), (dst, checked)
        print(f"config 5 stage {src} -> {dst}: {xin.features.shape[0]} -> {yout.features.shape[0]} rows, branches from the device {info['overridden']} of {info['hinted']}, "
              f"bias f needed {max(needed) if needed else 0:.3f}, oracle {time.time() - t0:.1f} s")
    net.eval()
    with torch.no_grad():
        preds, recall = net(dict(batch))
    assert len(preds) == 1 and preds[0]["pred_boxes"].shape[1] >= 7 and "gt" in recall
    # linearity of one 128 -> 128 submanifold layer at this size (size-independent property): conv(a x + b y) = a conv(x) + b conv(y)
    import seevcn_amd.spconv as spconv
    x4 = bd["multi_scale_3d_features"]["x_conv4"]
    conv = net.backbone_3d.conv4[1].conv1
    xa, xb = torch.randn_like(x4.features), torch.randn_like(x4.features)
    with torch.no_grad():
        mk = lambda ft: spconv.SparseConvTensor(ft, x4.indices, x4.spatial_shape, 1)
        ya, yb, yc = conv(mk(xa)).features, conv(mk(xb)).features, conv(mk(2.0 * xa - 3.0 * xb)).features
        bias = conv.bias.detach()
    np.testing.assert_allclose((yc - bias).cpu().numpy(), (2.0 * (ya - bias) - 3.0 * (yb - bias)).cpu().numpy(), rtol=1e-3, atol=2e-3)


# ------------------------------------------------------------------------------------------ config 4: PV-RCNN train step, DA geometry, 4096 keypoints
@pytest.mark.gpu
def test_hip_pvrcnn_train_step_at_config4_size(cuda, hip_lib):
    """4 scenes per GPU, 360-degree clouds with VCN-completed objects pasted in, sparse shape [41,1504,1504], NUM_KEYPOINTS 4096, sources
    bev / x_conv3 / x_conv4 / raw_points, 9000 -> 512 proposals, 128 RoIs x 216 grid points (source-nuscenes/pvrcnn.yaml)."""
    import seevcn_amd.synth as synth
    import seevcn_amd.vcn as V
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as raw
    from seevcn_amd.vcn.scene_merge import complete_scene_batch_device
    from seevcn_amd.vcn.utils import sampling
    B = 4
    pts, gt = ci.pvrcnn_scene_batch(B, n_az=350)
    per_scene = np.bincount(pts[:, 0].astype(int), minlength=B)
    assert per_scene.min() > 15000, per_scene
    # stage A feeds stage B: 16 cropped objects completed by VCN_VC (+ surface select + largest cluster), pasted into their scenes
    objs, _ = synth.make_object_batch(16, seed=1000)
    objs[:, :, 2] += 1.8                                                                 # SHIFT_COOR
    vcn = V.MODELS.build({"NAME": "VCN_VC"})
    vcn.load_state_dict(seeded_state_dict(vcn, seed=0))
    vcn = vcn.to(cuda).eval()
    with torch.no_grad():
        x = torch.from_numpy(objs).to(cuda)
        coarse = vcn({"input": x})["coarse"]
        surface, _ = sampling.get_partial_mesh_batch_device(x, coarse, k=30)
        clustered, _ = sampling.get_largest_cluster_batch_device(surface, eps=0.4, min_points=2)
        merged = complete_scene_batch_device(torch.from_numpy(pts).to(cuda), clustered, torch.arange(16, device=cuda).float() // 4, 0.1, compact=True)
    order = torch.argsort(merged[:, 0], stable=True)                                   # collate layout: stacked scene by scene
    points = merged[order].contiguous()
    assert points.shape[0] > pts.shape[0] - 16 * 1024

    ds = C.SyntheticDatasetInfo(class_names=["car"], point_cloud_range=C.DA_RANGE, voxel_size=C.DA_VOXEL, num_point_features=3)
    assert list(ds.grid_size) == [1504, 1504, 40]
    net = detectors.build_detector(C.see_pvrcnn_model_cfg(), num_class=1, dataset=ds)
    net.load_state_dict(seeded_state_dict(net, seed=6))
    net = net.to(cuda).train()
    assert net.backbone_3d.sparse_shape == [41, 1504, 1504]
    gtb = gt.copy()
    gtb[:, :, 7] = (gtb[:, :, 3] > 0)                                                   # one class
    batch = {"batch_size": B, "points": points, "gt_boxes": torch.from_numpy(gtb).to(cuda)}
    np.random.seed(0)
    torch.manual_seed(0)
    bd = dict(batch)
    for m in net.module_list:
        bd = m(bd)
    ret, tb, _ = net.get_training_loss()
    assert torch.isfinite(ret) and {"rpn_loss", "point_loss_cls", "rcnn_loss"} <= set(tb) | set(_)

    # D14 at size: 4096 keypoints per scene, index-exact against the oracle's restatement of the CUDA kernel (tie rule included)
    P = points.cpu().numpy()
    cnt = np.bincount(P[:, 0].astype(int), minlength=B)
    kp = bd["point_coords"].cpu().numpy()
    assert kp.shape == (B * 4096, 4)
    starts = np.cumsum(cnt) - cnt
    for b in (0, B - 1):                                                                # two scenes: the oracle takes ~10 s each
        want = op2.farthest_point_sampling(P[starts[b]:starts[b] + cnt[b], 1:4], 4096)
        assert np.array_equal(kp[b * 4096:(b + 1) * 4096, 1:4], P[starts[b] + want, 1:4]), b
    # D16 at size: ball query of the x_conv3 source (r 1.2 / 2.4, ns 16 / 32) vs oracle on a slice of the queries
    from seevcn_amd.pcdet.utils import common_utils
    t3 = bd["multi_scale_3d_features"]["x_conv3"]
    xyz3 = common_utils.get_voxel_centers(t3.indices[:, 1:4], downsample_times=4, voxel_size=C.DA_VOXEL, point_cloud_range=C.DA_RANGE).contiguous()
    c3 = torch.bincount(t3.indices[:, 0].long(), minlength=B).int()
    new_xyz = bd["point_coords"][:, 1:4].contiguous()
    qcnt = torch.full((B,), 4096, dtype=torch.int32, device=cuda)
    for radius, ns in ((1.2, 16), (2.4, 32)):
        idx = torch.zeros((new_xyz.shape[0], ns), dtype=torch.int32, device=cuda)
        raw.ball_query_wrapper(B, new_xyz.shape[0], radius, ns, new_xyz, qcnt, xyz3, c3, idx)
        sl = slice(4096, 4096 + 300)                                                    # 300 queries of scene 1
        c3n = c3.cpu().numpy()
        s1 = int(c3n[0])
        want = op2.ball_query(radius, ns, xyz3[s1:s1 + int(c3n[1])].cpu().numpy(), [int(c3n[1])], new_xyz[sl].cpu().numpy(), [300])
        assert np.array_equal(idx[sl].cpu().numpy(), want), radius
        # D16 features at size: the training-mode set-abstraction kernels (gather, MFMA MLP, batch-statistics BatchNorm, max) of this scale,
        # ALL 16 384 queries, against the float64 oracle on the same neighbour lists (the statistics need every row)
        k = 0 if ns == 16 else 1
        conv1, bn1, _, conv2, bn2, _ = list(net.pfe.SA_layers[0].mlps[k])
        n = lambda p: p.detach().cpu().numpy()
        row_start = torch.repeat_interleave(torch.cumsum(c3, 0) - c3, 4096).int().cpu().numpy()
        want_f = op2.sa_scale_train(xyz3.cpu().numpy(), t3.features.detach().cpu().numpy(), new_xyz.cpu().numpy(), idx.cpu().numpy(), row_start,
                                    n(conv1.weight).reshape(64, 67), n(bn1.weight), n(bn1.bias), n(conv2.weight).reshape(64, 64), n(bn2.weight), n(bn2.bias),
                                    eps=bn1.eps)
        got_f = bd["point_features_before_fusion"][:, 288 + 64 * k:288 + 64 * (k + 1)].detach().cpu().numpy()
        assert_close_per_channel(got_f, want_f, rtol=1e-3, atol_frac=1e-4, name=f"x_conv3 set-abstraction features, radius {radius}")
    # D19 at size: the 9000 -> 512 proposal NMS of scene 0 against the oracle sweep
    scores = bd["batch_cls_preds"][0].detach().max(dim=1)[0]
    boxes = bd["batch_box_preds"][0].detach()
    top = torch.topk(scores, k=9000)[1]
    keep, _ = iou3d_nms_utils.nms_gpu(boxes[top], scores[top], 0.8)
    sb, ss = boxes[top].cpu().numpy(), scores[top].cpu().numpy()
    o = np.argsort(-ss, kind="stable")
    if len(np.unique(ss)) == len(ss):
        assert np.array_equal(keep.cpu().numpy(), o[ob.nms(sb[o], 0.8)])
    assert tuple(net.roi_head.forward_ret_dict["rois"].shape) == (B, 128, 7)
    assert bd["point_features"].shape == (B * 4096, 128) and bd["point_features_before_fusion"].shape[1] == 256 + 128 + 128 + 32
    ret.backward()
    for name in ("backbone_3d.conv3.1.0.weight", "pfe.SA_layers.0.mlps.1.0.weight", "pfe.SA_rawpoints.mlps.0.0.weight", "roi_head.shared_fc_layer.0.weight",
                 "roi_head.roi_grid_pool_layer.mlps.0.0.weight", "dense_head.conv_box.weight"):
        g = dict(net.named_parameters())[name].grad
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, name
    net.eval()
    with torch.no_grad():
        preds, recall = net(dict(batch))
    assert len(preds) == B and all(p["pred_boxes"].shape[1] == 7 for p in preds) and "gt" in recall


# ------------------------------------------------------------------------------------------ headline size: gradients of sampled stages, 16 scenes
@pytest.mark.gpu
def test_hip_train_step_gradients_of_sampled_stages_at_16_scenes(cuda, hip_lib):
    """The benchmarked batch (16 scenes x 20.9 k returns, bench.py make_inputs) through DynMeanVFE -> VoxelBackBone8x (train mode, the chained
    launch-list path) -> HeightCompression -> loss -> backward.  tests/test_spconv.py checks the WHOLE chain against the float64 oracle on 2
    scenes; here, at full size, three sampled stages are checked with the step's own tensors on both sides of each: the stage's input features
    and the gradient arriving at its output are read from the GPU step, the float64 oracle (oracle/spconv_train.py stage_train_chain) recomputes
    the stage, and its output, its input gradient and every weight / BatchNorm gradient of its layers must match the step's, per channel."""
    import seevcn_amd.synth as synth
    from oracle import spconv_train as ost
    from seevcn_amd.pcdet.models import backbones_3d
    from seevcn_amd.pcdet.models.backbones_2d import map_to_bev
    from seevcn_amd.pcdet.models.backbones_3d import vfe
    B = 16
    pts, _ = synth.make_scene_batch(B, seed=2000, n_az=384)
    pc_range, vs, grid = [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1], [1408, 1600, 40]
    import seevcn_amd.spconv.chain as chain
    from seevcn_amd.spconv import norm
    m = backbones_3d.__all__["VoxelBackBone8x"]({}, 3, grid)
    sd = seeded_state_dict(m, seed=1)
    m.load_state_dict(sd)
    m = m.to(cuda).train()
    dyn_vfe = vfe.__all__["DynMeanVFE"](model_cfg={}, num_point_features=3, voxel_size=vs, grid_size=grid, point_cloud_range=pc_range)
    to_bev = map_to_bev.__all__["HeightCompression"]({"NUM_BEV_FEATURES": 256})

    with torch.no_grad():                                                  # voxelised once (the mean's float atomics are not bit-reproducible)
        voxels = dyn_vfe({"batch_size": B, "points": torch.from_numpy(pts).to(cuda)})
    assert voxels["voxel_features"].shape[0] > 200_000
    recorded = {}

    def step(chain_off, stats_in_conv=None, bwd_in_conv=False):
        """one forward + backward; the stage boundaries (multi_scale_3d_features) with the gradient that reached them, and the parameter gradients"""
        m.zero_grad(set_to_none=True)
        was, chain.CHAIN_OFF = chain.CHAIN_OFF, chain_off
        was_stats, was_bwd = norm.STATS_IN_CONV, chain.BWD_SUMS_IN_CONV
        chain.BWD_SUMS_IN_CONV = bwd_in_conv
        if stats_in_conv is not None:
            norm.STATS_IN_CONV = stats_in_conv
        try:
            bd = {"batch_size": B, "voxel_features": voxels["voxel_features"].clone(), "voxel_coords": voxels["voxel_coords"].clone()}
            hooks = []
            if chain_off:                                                  # the ReLU branches every block of the sampled stages took
                for name, blk in (("conv2", m.conv2), ("conv4", m.conv4)):
                    for i in range(3):
                        hooks.append(blk[i].register_forward_hook(lambda _m, _i, out, k=f"{name}.{i}.0.weight": recorded.__setitem__(k, out.features.detach() > 0)))
                hooks.append(m.conv_out.register_forward_hook(lambda _m, _i, out: recorded.__setitem__("conv_out.0.weight", out.features.detach() > 0)))
            bd = to_bev(m(bd))
            for h in hooks:
                h.remove()
            taps = dict(bd["multi_scale_3d_features"])
            taps["out"] = bd["encoded_spconv_tensor"]
            for t in taps.values():
                if t.features.requires_grad:
                    t.features.retain_grad()
            dense = bd["spatial_features"]
            G = torch.randn(dense.shape, generator=torch.Generator(device=cuda).manual_seed(5), device=cuda)
            (dense * G).sum().backward()
        finally:
            chain.CHAIN_OFF, norm.STATS_IN_CONV, chain.BWD_SUMS_IN_CONV = was, was_stats, was_bwd
        return taps, {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    # The layer-by-layer module path exposes the gradient at every stage boundary: it is the run held to the oracle element by element.  The
    # chained path (the default: one autograd node for the whole backbone) shows only parameter gradients and boundary features.  A ReLU branch
    # that flips moves a BatchNorm / weight gradient by O(1); since round 4 a rulebook table has exactly ONE plan (plan_region_body_stable), so the
    # batch statistics summed in the conv epilogues are the same in every run and the chain is BIT-IDENTICAL to the module path at this size in
    # its DEFAULT forward configuration (and with the statistics from their own reduction pass) -- it is held to the oracle at the module path's tolerance.
    # Round 5: by default the chain's BatchNorm BACKWARD sums come out of the data-gradient epilogues (plan order, not row order): that run (grads_default)
    # is deterministic but not bit-identical with the modules; it equals them to 1e-5 of each tensor's largest entry and is held to the oracle as well.
    taps, grads_modules = step(chain_off=True)
    branches = dict(recorded)                                              # the branches of THIS run (the later module-path run records its own)
    taps_chain, grads_chain = step(chain_off=False)
    for k in grads_modules:
        assert torch.equal(grads_modules[k], grads_chain[k]), (k, "backward sums in their own passes")
    for k in taps:
        assert torch.equal(taps[k].features, taps_chain[k].features), (k, "default forward configuration")
    taps_default, grads_default = step(chain_off=False, bwd_in_conv=True)
    _, grads_default2 = step(chain_off=False, bwd_in_conv=True)
    for k in grads_modules:
        assert torch.equal(grads_default[k], grads_default2[k]), (k, "the default configuration is reproducible run to run")
        assert float((grads_default[k] - grads_modules[k]).abs().max()) <= 1e-5 * float(grads_modules[k].abs().max()) + 1e-7, (k, "default configuration vs modules")
    for k in taps:
        assert torch.equal(taps[k].features, taps_default[k].features), (k, "default configuration")
    del taps_default, grads_default2
    taps_b, grads_b = step(chain_off=True, stats_in_conv=False)
    taps_c, grads_c = step(chain_off=False, stats_in_conv=False)
    for k in grads_b:
        assert torch.equal(grads_b[k], grads_c[k]), k
    for k in taps_b:
        assert torch.equal(taps_b[k].features, taps_c[k].features), k
    del taps_b, taps_c, grads_b, grads_c
    sdn = {k: v.numpy() for k, v in sd.items()}

    def block(name, i, kind, ksize=3, stride=1, pad=1):
        return (f"{name}.{i}.0.weight" if name != "conv_out" else "conv_out.0.weight", f"{name}.{i}.1" if name != "conv_out" else "conv_out.1",
                kind, ksize, stride, pad)

    stages = [("x_conv1", "x_conv2", [block("conv2", 0, "sparse", 3, 2, 1), block("conv2", 1, "subm"), block("conv2", 2, "subm")]),
              ("x_conv3", "x_conv4", [block("conv4", 0, "sparse", 3, 2, (0, 1, 1)), block("conv4", 1, "subm"), block("conv4", 2, "subm")]),
              ("x_conv4", "out", [block("conv_out", 0, "sparse", (3, 1, 1), (2, 1, 1), 0)])]
    for src, dst, layers in stages:
        xin, yout = taps[src], taps[dst]
        assert xin.features.grad is not None and yout.features.grad is not None, (src, dst)
        # The ReLU's derivative jumps at zero: the oracle follows the branch the device took wherever its own pre-activation is closer to zero than
        # 1e-4 (oracle/spconv_train.py stage_train_chain), its own sign everywhere else; at most 1e-4 of the activations may be decided that way.
        x_np, c_np, dy = xin.features.detach().cpu().numpy(), xin.indices.cpu().numpy(), yout.features.grad.detach().cpu().double()
        hints = {key: branches[key].cpu().numpy() for key, *_ in layers}
        ref, leaves, oc, oshape, overridden = ost.stage_train_chain(sdn, layers, x_np, c_np, xin.spatial_shape, branch_hints=hints, hint_band=1e-4)
        assert overridden <= 1e-4 * sum(h.size for h in hints.values()), (dst, overridden)
        assert np.array_equal(yout.indices.cpu().numpy(), oc) and list(yout.spatial_shape) == list(oshape), dst
        assert_close_per_channel(yout.features.detach().cpu().numpy(), ref.detach().numpy(), name=f"{dst} features (16 scenes)")
        ref.backward(dy)
        assert_close_per_channel(xin.features.grad.cpu().numpy(), leaves["input"].grad.numpy(), rtol=2e-3, atol_frac=2e-4, name=f"d loss / d {src}")
        assert_close_per_channel(taps_chain[dst].features.detach().cpu().numpy(), ref.detach().numpy(), name=f"{dst} features (16 scenes, chained path)")
        for key, _bn, *_ in layers:
            for k in (key, _bn + ".weight", _bn + ".bias"):
                for path, grads in (("modules", grads_modules), ("chain", grads_chain), ("chain, default backward sums", grads_default)):
                    got = grads[k].cpu().numpy()
                    if got.ndim == 5:
                        got = osp.weight_to_kio(got)
                    # sums over 10^5 rows of products of O(1) terms in fp32: 2e-3 of each output channel's own largest value (as in the 2-scene test)
                    assert_close_per_channel(got, leaves[k].grad.numpy(), rtol=2e-3, atol_frac=2e-3, name=f"grad {k} (16 scenes, {path})")
