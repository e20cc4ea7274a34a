"""The sv_focal_image_* entries (csrc/focal_image.hip), their autograd function (spconv/focal.py) and FocalSparseConvMultimodal on the GPU against
tests/focal_image_reference.py: pixels against the reference's own lidar_to_img (tests/golden/focal_image.npz) on every unmasked voxel,
forward values within a derived fp32 bound of the float64 restatement, the feature gradient bit for bit against the fp32 ascending-key loop,
and the layer against itself with the image features taken by a plain-torch statement."""
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

import focal_image_reference as FI
from seeding import seeded_state_dict

_cache = {}


def _case(name):
    """the case, its pixels by the float64 restatement and by the golden, and the mask -- computed once and shared"""
    if name not in _cache:
        case = FI.make_case(name)
        gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focal_image.npz"))
        assert np.array_equal(case["coords"], gold[name + "_coords"])
        u, v, rz, bu, bv = FI.project64(case, case["calibs"], case["coords"])
        img = gold[name + "_img"]
        case.update(mask=FI.pixel_mask(u, v, rz, bu, bv), pix64=FI.pixels(u, v, case["image"]), pix_gold=FI.pixels(img[:, 0], img[:, 1], case["image"]))
        _cache[name] = case
    return _cache[name]


def _device_pixels(case, cuda, batch_dict=None):
    from seevcn_amd.pcdet.utils import calibration_kitti
    from seevcn_amd.spconv import focal
    coords = torch.from_numpy(case["coords"]).to(cuda)
    aug = focal.image_aug_table(FI.batch_dict_aug(case, cuda) if batch_dict is None else batch_dict, case["B"], cuda)
    calib = calibration_kitti.pack_calib(case["calibs"], cuda)
    return coords, focal.focal_image_pixels(coords, case["B"], 1, FI.VOXEL_ZYX, FI.RANGE_ZYX, calib, aug, case["image"])


# ---------------------------------------------------------------------------------------------------------------- pixels
@pytest.mark.gpu
@pytest.mark.parametrize("name", FI.CASE_NAMES)
def test_hip_pixels_match_reference_projection(cuda, hip_lib, name):
    case = _case(name)
    _, pix = _device_pixels(case, cuda)
    pix = pix.cpu().numpy()
    H, W = case["image"]
    keep = ~case["mask"]
    assert pix.dtype == np.int32 and pix.min() >= -1 and pix.max() < H * W
    wrong = np.flatnonzero((pix != case["pix_gold"]) & keep)
    print(name, "rows", len(pix), "masked", int(case["mask"].sum()), "inside", int((pix >= 0).sum()), "differ from the golden", len(wrong),
          "differ on masked rows", int(((pix != case["pix_gold"]) & ~keep).sum()))
    assert len(wrong) == 0, (wrong[:10], pix[wrong[:10]], case["pix_gold"][wrong[:10]])
    assert np.array_equal(pix[keep] < 0, case["pix_gold"][keep] < 0) and np.array_equal(pix[keep], case["pix64"][keep])
    if name == "tiny":                                           # absent keys and explicit identity values give the same pixels
        identity = dict(noise_scale=torch.ones(2, device=cuda), noise_rot=torch.zeros(2, device=cuda), flip_x=torch.zeros(2, dtype=torch.bool, device=cuda),
                        flip_y=torch.zeros(2, dtype=torch.bool, device=cuda))
        assert np.array_equal(_device_pixels(case, cuda, identity)[1].cpu().numpy(), pix)


@pytest.mark.gpu
def test_hip_pixels_refuse_nonfinite_and_foreign_scenes(cuda, hip_lib):
    """a non-finite u or v and a scene index outside the batch give -1"""
    from seevcn_amd.pcdet.utils import calibration_kitti
    from seevcn_amd.spconv import focal
    case = _case("tiny")
    coords = torch.from_numpy(case["coords"][:64].copy()).to(cuda)
    coords[5, 0], coords[6, 0] = 2, -1
    calib = calibration_kitti.pack_calib(case["calibs"], cuda)
    aug = focal.image_aug_table({}, 2, cuda)
    pix = focal.focal_image_pixels(coords, 2, 1, FI.VOXEL_ZYX, FI.RANGE_ZYX, calib, aug, case["image"]).cpu().numpy()
    assert pix[5] == -1 and pix[6] == -1 and (pix >= 0).any()
    aug[0, 0] = 0.0                                               # noise_scale 0: every centre becomes infinite or NaN
    assert (focal.focal_image_pixels(coords, 2, 1, FI.VOXEL_ZYX, FI.RANGE_ZYX, calib, aug, case["image"]) == -1).all()


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.gpu
@pytest.mark.parametrize("fuse_sum", [False, True], ids=["concat", "sum"])
@pytest.mark.parametrize("name", FI.CASE_NAMES)
def test_hip_fused_rows_within_fp32_bound_of_float64(cuda, hip_lib, name, fuse_sum):
    from seevcn_amd.spconv import focal
    case = _case(name)
    coords, pix = _device_pixels(case, cuda)
    C = case["C"]
    out = focal.focal_image_fuse(torch.from_numpy(case["f"]).to(cuda), torch.from_numpy(case["features"]).to(cuda), coords, pix, case["image"], fuse_sum)
    out = out.cpu().numpy()
    pix = pix.cpu().numpy()
    want, bound = FI.forward64(case, pix, fuse_sum), FI.forward_bound(case, pix, fuse_sum)
    assert out.shape == want.shape == ((len(pix), C) if fuse_sum else (len(pix), 2 * C)) and out.dtype == np.float32
    err = np.abs(out.astype(np.float64) - want)
    print(name, "sum" if fuse_sum else "concat", "largest error", err.max(), "largest bound", bound.max(), "largest error / bound",
          (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0)
    assert (err <= bound).all()
    if not fuse_sum:                                              # the layout: [img | f], f copied, rows without a pixel zero
        assert np.array_equal(out[:, C:], case["f"]) and (out[pix < 0, :C] == 0).all() and (pix < 0).any()
        assert np.abs(out[pix >= 0, :C]).sum(axis=1).min() > 0
    else:
        assert np.array_equal(out[pix < 0], case["f"][pix < 0])


# ---------------------------------------------------------------------------------------------------------------- gradient
def _raw_grad(lib, L, case, coords, pix, g, cuda, n=None):
    """sv_focal_image_sample_grad on a map poisoned with NaN and a scratch poisoned with 0xA5"""
    B, h, w, C = case["features"].shape
    H, W = case["image"]
    n = len(case["coords"]) if n is None else n
    nbytes = lib.sv_focal_image_sample_grad_scratch_bytes(n, B, h, w, H, W)
    assert nbytes > 0
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=cuda)
    out = torch.full((B, h, w, C), float("nan"), dtype=torch.float32, device=cuda)
    rc = lib.sv_focal_image_sample_grad(L.ptr(g), g.shape[1], L.ptr(coords), L.ptr(pix), n, B, h, w, C, H, W, L.ptr(scratch), L.ptr(out), L.stream())
    L.check(rc, "sv_focal_image_sample_grad")
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_sum", [False, True], ids=["concat", "sum"])
@pytest.mark.parametrize("name", FI.CASE_NAMES)
def test_hip_feature_gradient_equals_ascending_key_loop_bit_for_bit(cuda, hip_lib, name, fuse_sum):
    import seevcn_amd._lib as L
    from seevcn_amd.spconv import focal
    case = _case(name)
    coords, pix = _device_pixels(case, cuda)
    g_host = case["g_sum"] if fuse_sum else case["g_concat"]
    g = torch.from_numpy(g_host).to(cuda)
    want, longest = FI.grad_loop32(case, pix.cpu().numpy(), g_host)
    got = _raw_grad(hip_lib, L, case, coords, pix, g, cuda)
    again = _raw_grad(hip_lib, L, case, coords, pix, g, cuda)
    print(name, "sum" if fuse_sum else "concat", "longest list", longest, "pixels without a key", int((np.abs(want).sum(axis=-1) == 0).sum()))
    assert not np.isnan(got).any()                                # every element written
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == again.tobytes()
    # through autograd: the same map, and the voxel features' gradient a slice (concat) or the identity (sum)
    f = torch.from_numpy(case["f"]).to(cuda).requires_grad_(True)
    feats = torch.from_numpy(case["features"]).to(cuda).requires_grad_(True)
    focal.focal_image_fuse(f, feats, coords, pix, case["image"], fuse_sum).backward(g)
    assert feats.grad.cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(f.grad.cpu().numpy(), g_host if fuse_sum else g_host[:, case["C"]:])


@pytest.mark.gpu
def test_hip_no_rows_give_the_zero_map_and_empty_output(cuda, hip_lib):
    import seevcn_amd._lib as L
    from seevcn_amd.spconv import focal
    case = _case("ratio")
    coords = torch.zeros((0, 4), dtype=torch.int32, device=cuda)
    pix = torch.zeros((0,), dtype=torch.int32, device=cuda)
    g = torch.zeros((0, 2 * case["C"]), dtype=torch.float32, device=cuda)
    got = _raw_grad(hip_lib, L, case, coords, pix, g, cuda, n=0)
    assert got.tobytes() == np.zeros_like(case["features"]).tobytes()                       # +0.0f everywhere
    feats = torch.from_numpy(case["features"]).to(cuda)
    f = torch.zeros((0, case["C"]), dtype=torch.float32, device=cuda)
    assert tuple(focal.focal_image_fuse(f, feats, coords, pix, case["image"], False).shape) == (0, 2 * case["C"])
    assert tuple(focal.focal_image_fuse(f, feats, coords, pix, case["image"], True).shape) == (0, case["C"])
    with pytest.raises(L.SeevcnHipError, match="as many image channels"):
        focal.focal_image_fuse(torch.zeros((0, 8), device=cuda), feats, coords, pix, case["image"], True)


# ---------------------------------------------------------------------------------------------------------------- no host read, constant calls
@pytest.mark.gpu
def test_hip_fused_route_reads_nothing_back_and_calls_do_not_grow_with_the_batch(cuda, hip_lib, monkeypatch):
    from seevcn_amd.pcdet.utils import calibration_kitti
    from seevcn_amd.spconv import focal
    case = _case("ratio")
    calls = {}

    def counted(name, fn):
        def call(*args):
            calls[name] = calls.get(name, 0) + 1
            return fn(*args)
        return call

    for name in ("sv_focal_image_pixels", "sv_focal_image_sample", "sv_focal_image_sample_grad_scratch_bytes", "sv_focal_image_sample_grad"):
        monkeypatch.setattr(hip_lib, name, counted(name, getattr(hip_lib, name)))
    seen = []
    for B in (1, 3):
        coords = case["coords"].copy()
        coords[:, 0] = np.arange(len(coords)) % B
        coords = torch.from_numpy(coords).to(cuda)
        calibs = [FI.make_calib(case["image"], b) for b in range(B)]
        batch_dict = {"noise_rot": torch.linspace(-0.3, 0.3, B, device=cuda), "flip_x": torch.arange(B, device=cuda) % 2 == 1}
        f = torch.from_numpy(case["f"]).to(cuda).requires_grad_(True)
        feats = torch.randn((B,) + case["features"].shape[1:], device=cuda).requires_grad_(True)
        g = torch.from_numpy(case["g_concat"]).to(cuda)
        torch.cuda.synchronize()
        calls.clear()
        previous = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            aug = focal.image_aug_table(batch_dict, B, cuda)
            calib = calibration_kitti.pack_calib(calibs, cuda)
            pix = focal.focal_image_pixels(coords, B, 1, FI.VOXEL_ZYX, FI.RANGE_ZYX, calib, aug, case["image"])
            focal.focal_image_fuse(f, feats, coords, pix, case["image"], False).backward(g)
        finally:
            torch.cuda.set_sync_debug_mode(previous)
        assert torch.isfinite(feats.grad).all() and bool((pix >= 0).any())
        seen.append(dict(calls))
    assert seen[0] == seen[1] == {"sv_focal_image_pixels": 1, "sv_focal_image_sample": 1, "sv_focal_image_sample_grad_scratch_bytes": 1,
                                   "sv_focal_image_sample_grad": 1}, seen


# ---------------------------------------------------------------------------------------------------------------- the layer
def _plain_torch_fuse(layer, x, image_ctx, fuse_sum=False):
    """construct_multimodal_features with the image features taken as the reference takes them -- F.interpolate to the image size, then indexing --
    in plain torch; the pixels are the kernel's (held to the reference above)."""
    from seevcn_amd.spconv import focal
    features_nhwc, calib_table, aug_table, (H, W) = image_ctx
    pix = focal.focal_image_pixels(x.indices, x.batch_size, layer.voxel_stride, layer.voxel_size, layer.point_cloud_range[:3], calib_table, aug_table,
                                   (H, W))
    x_rgb = features_nhwc.permute(0, 3, 1, 2)
    if tuple(x_rgb.shape[2:]) != (H, W):
        x_rgb = TF.interpolate(x_rgb, (H, W), mode="bilinear")
    flat = x_rgb.permute(0, 2, 3, 1).reshape(-1, x_rgb.shape[1])
    inside = pix >= 0
    img = flat[x.indices[:, 0].long() * (H * W) + pix.clamp(min=0).long()] * inside[:, None]
    return x.features + img if fuse_sum else torch.cat([img, x.features], dim=1)


@pytest.mark.gpu
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_hip_multimodal_layer_matches_plain_torch_image_features(cuda, hip_lib, train):
    import seevcn_amd.spconv as spconv
    from oracle.tolerances import assert_close_per_channel
    from seevcn_amd.pcdet.models.backbones_3d.focal_sparse_conv.focal_sparse_conv import FocalSparseConvMultimodal
    case = _case("ratio")
    C = case["C"]
    norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    # one box per scene in metres [x, y, z, dx, dy, dz, heading, class], faces off the voxel positions
    gt = np.array([[[30.013, 0.017, -1.003, 24.0, 30.0, 3.0, 0.0, 1.0]], [[45.011, -9.987, -0.997, 30.0, 24.0, 3.0, 0.0, 1.0]]], np.float32)
    results = []
    sd = None
    for plain in (False, True):
        m = FocalSparseConvMultimodal(C, C, voxel_stride=1, norm_fn=norm_fn, indice_key="spconv_focal_multimodal", image_channel=C, topk=True,
                                      threshold=0.5)
        sd = seeded_state_dict(m, seed=17) if sd is None else sd
        m.load_state_dict(sd)
        m = m.to(cuda).train(train)
        if plain:
            m.construct_multimodal_features = partial(_plain_torch_fuse, m)
        f = torch.from_numpy(case["f"]).to(cuda).requires_grad_(True)
        x_rgb = torch.from_numpy(case["features"]).to(cuda).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        batch_dict = dict(batch_size=case["B"], gt_boxes=torch.from_numpy(gt).to(cuda), calib=case["calibs"],
                          images=torch.zeros((case["B"], 3) + tuple(case["image"]), device=cuda), **FI.batch_dict_aug(case, cuda))
        out, bd, loss = m(spconv.SparseConvTensor(f, torch.from_numpy(case["coords"]).to(cuda), list(FI.GRID_ZYX), case["B"]), batch_dict, x_rgb)
        assert bd is batch_dict
        g = torch.from_numpy(np.random.RandomState(9).randn(*out.features.shape).astype(np.float32)).to(cuda)
        ((out.features * g).sum() + loss).backward()
        results.append(dict(indices=out.indices.cpu().numpy(), features=out.features.detach().cpu().numpy(), loss=float(loss), f_grad=f.grad.cpu().numpy(),
                            rgb_grad=x_rgb.grad.cpu().numpy(), params={k: p.grad.cpu().numpy() for k, p in m.named_parameters()},
                            buffers={k: b.cpu().numpy() for k, b in m.named_buffers()}))
    mine, want = results
    assert tuple(sd["conv_imp.weight"].shape) == (27, 3, 3, 3, 2 * C)
    assert len(mine["indices"]) > len(case["coords"]) and np.array_equal(mine["indices"], want["indices"])       # the same top-k: seeded continuous values
    assert_close_per_channel(mine["features"], want["features"], rtol=1e-3, atol_frac=1e-4, name="features")
    if train:
        assert mine["loss"] > 0 and abs(mine["loss"] - want["loss"]) <= 1e-5 * abs(want["loss"]), (mine["loss"], want["loss"])
    else:
        assert mine["loss"] == 0 and want["loss"] == 0
    assert_close_per_channel(mine["f_grad"], want["f_grad"], rtol=2e-3, atol_frac=2e-4, name="input gradient")
    assert_close_per_channel(mine["rgb_grad"].transpose(0, 2, 3, 1).reshape(-1, C), want["rgb_grad"].transpose(0, 2, 3, 1).reshape(-1, C), rtol=2e-3,
                             atol_frac=2e-4, name="image feature gradient")
    assert np.abs(mine["rgb_grad"]).sum() > 0
    for k in want["params"]:
        assert_close_per_channel(mine["params"][k], want["params"][k], rtol=2e-3, atol_frac=2e-3, name="grad " + k)
        assert np.abs(mine["params"][k]).sum() > 0, k
    for k in want["buffers"]:
        np.testing.assert_allclose(mine["buffers"][k], want["buffers"][k], rtol=1e-4, atol=1e-6, err_msg=k)
