"""Channel-last BEV keypoint features (sv_bev_interpolate_nhwc / sv_bev_interpolate_grad_nhwc and the dispatch in VoxelSetAbstraction).

Forward: bit-identical to the NCHW entry on the permuted map.  Gradient: bit-exact to the order the header defines (tests/bev_reference.py), which a
float-atomic sum cannot meet, and within (n + 1) * 2^-24 * sum |grad_out * w| of the float64 sum -- a bound the NCHW entry's atomic order meets too."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bev_reference as R
import seevcn_amd._lib as L

NEW_ENTRIES = {
    "sv_bev_interpolate_nhwc": ("int", ["const float*", "int64_t", "const float*", "int", "int", "int", "int", "float", "float", "float", "float", "float",
                                        "float*", "void*"]),
    "sv_bev_interpolate_grad_nhwc_scratch_bytes": ("size_t", ["int64_t", "int", "int", "int"]),
    "sv_bev_interpolate_grad_nhwc": ("int", ["const float*", "int64_t", "const float*", "int", "int", "int", "int", "float", "float", "float", "float",
                                             "float", "void*", "float*", "void*"]),
}
MAPS = [(5, 7), (16, 12)]
CHANNELS = [1, 3, 64, 130, 256]
KINDS = ["empty", "one", "mixed", "cluster"]
B = 2


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_and_binding_declare_the_new_entries():
    with open(L.HEADER_PATH) as f:
        protos = L.parse_declarations(f.read())
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name, (ret, params) in NEW_ENTRIES.items():
        assert name in protos, f"{name} is not declared in seevcn_hip.h"
        declared = [p.rsplit(" ", 1)[0] for p in protos[name][1]]                                # drop the parameter names
        assert protos[name][0] == ret and declared == params, (name, protos[name][0], declared)
        assert name in L.SIGNATURES, f"{name} has no prototype in _lib.py"
        restype, argtypes = L.SIGNATURES[name]
        assert restype == ctype[ret]
        assert argtypes == [ctypes.c_void_p if p.endswith("*") else ctype[p] for p in params], name


def _case(kind, H, W, C, geom=R.DYADIC, seed=0):
    kps = R.make_keypoints(kind, B, H, W, geom, seed=seed)
    grad_out = np.random.RandomState(seed + 100).standard_normal((kps.shape[0], C)).astype(np.float32)
    return kps, grad_out


@functools.lru_cache(maxsize=None)
def _references(kind, H, W, C):
    """(kps, grad_out, sequential fp32, float64, bound), computed once and shared; the arrays are read-only."""
    kps, grad_out = _case(kind, H, W, C)
    seq = R.grad_sequential_f32(kps, grad_out, R.DYADIC, B, C, H, W)
    exact, bound = R.grad_f64(kps, grad_out, R.DYADIC, B, C, H, W)
    for a in (kps, grad_out, seq, exact, bound):
        a.setflags(write=False)
    return kps, grad_out, seq, exact, bound


def test_reference_sequential_order_within_bound_of_float64():
    for kind in KINDS:
        kps, grad_out, seq, exact, bound = _references(kind, 5, 7, 3)
        keys, pix, w = R.tap_terms(kps, R.DYADIC, B, 5, 7)              # asserts finite weights, unique ascending keys
        assert len(keys) == 4 * int(((kps[:, 0] >= 0) & (kps[:, 0] < B)).sum())
        R.assert_within_bound(seq, exact, bound, name=kind)
        untouched = np.bincount(pix, minlength=B * 5 * 7).reshape(B, 5, 7) == 0
        assert not np.signbit(seq[untouched]).any() and (seq[untouched] == 0).all()
    cluster_pix = R.tap_terms(_references("cluster", 5, 7, 3)[0], R.DYADIC, B, 5, 7)[1]
    assert np.bincount(cluster_pix).max() >= 300                        # the long key lists are really there


def test_checker_rejects_a_dropped_tap():
    kps, grad_out, seq, exact, bound = _references("mixed", 5, 7, 3)
    keys, _, w = R.tap_terms(kps, R.DYADIC, B, 5, 7)
    drop = int(keys[np.argmax(np.abs(w))])                              # a tap that carries weight
    dropped = R.grad_sequential_f32(kps, grad_out, R.DYADIC, B, 3, 5, 7, drop_key=drop)
    with pytest.raises(AssertionError):
        R.assert_bit_equal(dropped, seq)
    with pytest.raises(AssertionError):
        R.assert_within_bound(dropped, exact, bound)


def test_checker_rejects_a_reversed_key_order():
    kps, grad_out = R.order_sensitive_case()
    fwd = R.grad_sequential_f32(kps, grad_out, R.DYADIC, 1, 1, 5, 7)
    rev = R.grad_sequential_f32(kps, grad_out, R.DYADIC, 1, 1, 5, 7, reverse=True)
    assert fwd[0, 1, 2, 0] == np.float32(1.0) and rev[0, 1, 2, 0] == np.float32(1.0) + np.float32(2.0 ** -23)
    with pytest.raises(AssertionError):
        R.assert_bit_equal(rev, fwd)
    exact, bound = R.grad_f64(kps, grad_out, R.DYADIC, 1, 1, 5, 7)
    R.assert_within_bound(fwd, exact, bound)                            # both orders are fair fp32 sums: only the bitwise check tells them apart
    R.assert_within_bound(rev, exact, bound)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _forward(lib, entry, kps, bev, Bn, C, H, W, geom):
    out = torch.full((kps.shape[0], C), float("nan"), dtype=torch.float32, device=kps.device)
    rc = getattr(lib, entry)(L.ptr(kps), kps.shape[0], L.ptr(bev), Bn, C, H, W, geom.x_min, geom.y_min, geom.voxel_x, geom.voxel_y, geom.stride,
                             L.ptr(out), L.stream())
    L.check(rc, entry)
    return out


def _grad_nhwc(lib, kps, grad_out, Bn, C, H, W, geom=R.DYADIC):
    gbev = torch.full((Bn, H, W, C), float("nan"), dtype=torch.float32, device=grad_out.device)
    nbytes = lib.sv_bev_interpolate_grad_nhwc_scratch_bytes(kps.shape[0], Bn, H, W)
    scratch = torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device=grad_out.device)     # uninitialised as far as the entry may assume
    rc = lib.sv_bev_interpolate_grad_nhwc(L.ptr(kps), kps.shape[0], L.ptr(grad_out), Bn, C, H, W, geom.x_min, geom.y_min, geom.voxel_x, geom.voxel_y,
                                          geom.stride, L.ptr(scratch), L.ptr(gbev), L.stream())
    L.check(rc, "sv_bev_interpolate_grad_nhwc")
    return gbev


def _grad_nchw(lib, kps, grad_out, Bn, C, H, W, geom=R.DYADIC):
    gbev = torch.full((Bn, C, H, W), float("nan"), dtype=torch.float32, device=grad_out.device)
    scratch = torch.empty((max(lib.sv_bev_interpolate_grad_scratch_bytes(Bn, C, H, W), 16),), dtype=torch.uint8, device=grad_out.device)
    rc = lib.sv_bev_interpolate_grad(L.ptr(kps), kps.shape[0], L.ptr(grad_out), Bn, C, H, W, geom.x_min, geom.y_min, geom.voxel_x, geom.voxel_y, geom.stride,
                                     L.ptr(scratch), L.ptr(gbev), L.stream())
    L.check(rc, "sv_bev_interpolate_grad")
    return gbev


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("H,W", MAPS)
def test_forward_bit_identical_to_nchw_entry(cuda, hip_lib, H, W, C):
    bev = torch.from_numpy(np.random.RandomState(C).standard_normal((B, C, H, W)).astype(np.float32)).to(cuda)
    bev_cl = bev.permute(0, 2, 3, 1).contiguous()
    for kind in KINDS:
        kps = torch.from_numpy(R.make_keypoints(kind, B, H, W, R.KITTI, seed=1)).to(cuda)
        want = _forward(hip_lib, "sv_bev_interpolate", kps, bev, B, C, H, W, R.KITTI)
        got = _forward(hip_lib, "sv_bev_interpolate_nhwc", kps, bev_cl, B, C, H, W, R.KITTI)
        assert not torch.isnan(got).any(), kind
        assert torch.equal(got, want), (kind, (got != want).sum().item())
        outside = (kps[:, 0] < 0) | (kps[:, 0] >= B)
        assert (got[outside] == 0).all()
    if C % 4 == 0:                                                      # a map that starts 4 bytes into an allocation: C % 4 == 0 but no 16-byte alignment
        flat = torch.empty(bev_cl.numel() + 1, dtype=torch.float32, device=cuda)
        shifted = flat[1:].view(bev_cl.shape).copy_(bev_cl)
        kps = torch.from_numpy(R.make_keypoints("mixed", B, H, W, R.KITTI, seed=1)).to(cuda)
        assert torch.equal(_forward(hip_lib, "sv_bev_interpolate_nhwc", kps, shifted, B, C, H, W, R.KITTI),
                           _forward(hip_lib, "sv_bev_interpolate", kps, bev, B, C, H, W, R.KITTI))


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("H,W", MAPS)
def test_gradient_bit_exact_to_defined_order(cuda, hip_lib, H, W, C):
    for kind in KINDS:
        kps_np, grad_np, seq, _, _ = _references(kind, H, W, C)
        kps, grad_out = torch.from_numpy(kps_np.copy()).to(cuda), torch.from_numpy(grad_np.copy()).to(cuda)
        first = _grad_nhwc(hip_lib, kps, grad_out, B, C, H, W).cpu().numpy()
        R.assert_bit_equal(first, seq, name=f"{kind} vs sequential fp32")          # untouched pixels +0.0: the sign bit is compared too
        second = _grad_nhwc(hip_lib, kps, grad_out, B, C, H, W).cpu().numpy()
        R.assert_bit_equal(second, first, name=f"{kind} second run")
        # one more (empty) scene changes B*H*W: other workgroups take the key-list segments, in another order
        padded = _grad_nhwc(hip_lib, kps, grad_out, B + 1, C, H, W).cpu().numpy()
        want = R.grad_sequential_f32(kps_np, grad_np, R.DYADIC, B + 1, C, H, W)      # rows with batch index B are valid on the padded map
        R.assert_bit_equal(padded, want, name=f"{kind} padded map")
        if not (kps_np[:, 0] == B).any():
            R.assert_bit_equal(padded[:B], first, name=f"{kind} padded map vs first run")


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("H,W", MAPS)
def test_gradient_within_bound_of_float64(cuda, hip_lib, H, W, C):
    for kind in KINDS:
        kps_np, grad_np, _, exact, bound = _references(kind, H, W, C)
        kps, grad_out = torch.from_numpy(kps_np.copy()).to(cuda), torch.from_numpy(grad_np.copy()).to(cuda)
        got = _grad_nhwc(hip_lib, kps, grad_out, B, C, H, W).cpu().numpy()
        R.assert_within_bound(got, exact, bound, name=f"{kind} nhwc entry")
        atomic = _grad_nchw(hip_lib, kps, grad_out, B, C, H, W).permute(0, 2, 3, 1).cpu().numpy()
        R.assert_within_bound(atomic, exact, bound, name=f"{kind} nchw entry (float atomics), permuted")


def _vsa_module():
    from seevcn_amd.pcdet.models.backbones_3d.pfe import voxel_set_abstraction as vsa_mod
    return vsa_mod


@pytest.mark.gpu
def test_autograd_takes_the_channels_last_route(cuda, hip_lib, monkeypatch):
    vsa_mod = _vsa_module()
    monkeypatch.setattr(vsa_mod, "BEV_INTERP_NHWC", True)              # whatever the environment of the run says
    H, W, C = 16, 12, 64
    kps_np, grad_np, seq, exact, bound = _references("mixed", H, W, C)
    kps, grad_out = torch.from_numpy(kps_np.copy()).to(cuda), torch.from_numpy(grad_np.copy()).to(cuda)
    values = torch.from_numpy(np.random.RandomState(5).standard_normal((B, C, H, W)).astype(np.float32)).to(cuda)
    g = R.DYADIC
    args = (g.x_min, g.y_min, g.voxel_x, g.voxel_y, g.stride)

    def run(leaf):
        out = vsa_mod._BevInterp.apply(leaf, kps, *args)
        layout = vsa_mod.VoxelSetAbstraction.last_bev_layout
        out.backward(grad_out)
        return out.detach(), leaf.grad, layout

    nchw_out, nchw_grad, layout = run(values.clone().requires_grad_(True))
    assert layout == "nchw" and nchw_grad.is_contiguous()
    leaf = values.contiguous(memory_format=torch.channels_last).detach().requires_grad_(True)
    assert leaf.is_contiguous(memory_format=torch.channels_last) and not leaf.is_contiguous()
    out, grad, layout = run(leaf)
    assert layout == "nhwc"
    assert torch.equal(out, nchw_out)
    assert grad.shape == (B, C, H, W) and grad.is_contiguous(memory_format=torch.channels_last) and not grad.is_contiguous()
    R.assert_bit_equal(grad.permute(0, 2, 3, 1).cpu().numpy(), seq, name="autograd gradient vs sequential fp32")

    monkeypatch.setattr(vsa_mod, "BEV_INTERP_NHWC", False)             # SEEVCN_BEV_INTERP_NHWC=0
    off_out, off_grad, layout = run(values.contiguous(memory_format=torch.channels_last).detach().requires_grad_(True))
    assert layout == "nchw"
    assert torch.equal(off_out, nchw_out)
    R.assert_within_bound(off_grad.permute(0, 2, 3, 1).cpu().numpy(), exact, bound, name="switched-off route (float atomics)")
    R.assert_within_bound(nchw_grad.permute(0, 2, 3, 1).cpu().numpy(), exact, bound, name="nchw leaf (float atomics)")


@pytest.mark.gpu
def test_vsa_channels_last_map_gives_the_same_point_features(cuda, hip_lib, monkeypatch):
    vsa_mod = _vsa_module()
    monkeypatch.setattr(vsa_mod, "BEV_INTERP_NHWC", True)              # whatever the environment of the run says
    from seeding import seeded_state_dict
    from seevcn_amd.pcdet import model_cfgs as C
    pc_range, voxel = [0.0, -8.0, -3.0, 16.0, 8.0, 1.0], [0.05, 0.05, 0.1]
    geom = R.Geom(pc_range[0], pc_range[1], voxel[0], voxel[1], 8.0)
    Cb, H, W, nkp = 32, 40, 40, 128
    pfe_cfg, _, _ = C.pvrcnn_cfg(num_keypoints=nkp, features_source=("bev", "raw_points"))
    vsa = vsa_mod.VoxelSetAbstraction(pfe_cfg, voxel_size=voxel, point_cloud_range=pc_range, num_bev_features=Cb, num_rawpoint_features=4)
    vsa.load_state_dict(seeded_state_dict(vsa, seed=21))
    vsa = vsa.to(cuda).train()
    rng = np.random.RandomState(3)
    pts = np.concatenate([np.stack([np.full(n, b), rng.uniform(0, 16, n), rng.uniform(-8, 8, n), rng.uniform(-3, 1, n), rng.uniform(0, 1, n)], axis=1)
                          for b, n in ((0, 700), (1, 500))]).astype(np.float32)
    points = torch.from_numpy(pts).to(cuda)
    values = torch.from_numpy(rng.standard_normal((2, Cb, H, W)).astype(np.float32)).to(cuda)
    probe = torch.from_numpy(rng.standard_normal((2 * nkp, vsa.num_point_features)).astype(np.float32)).to(cuda)

    def run(leaf):
        bd = vsa({"batch_size": 2, "points": points, "spatial_features": leaf, "spatial_features_stride": 8})
        before = bd["point_features_before_fusion"]
        before.retain_grad()
        (bd["point_features"] * probe).sum().backward()
        return (bd["point_features"].detach(), bd["point_coords"].detach(), before.grad[:, :Cb].contiguous(), leaf.grad,
                vsa_mod.VoxelSetAbstraction.last_bev_layout)

    feats_a, kp_a, gout_a, grad_a, layout_a = run(values.clone().requires_grad_(True))
    feats_b, kp_b, gout_b, grad_b, layout_b = run(values.contiguous(memory_format=torch.channels_last).detach().requires_grad_(True))
    assert (layout_a, layout_b) == ("nchw", "nhwc")
    assert torch.equal(kp_a, kp_b) and torch.equal(feats_a, feats_b)
    for name, gout, grad in (("nchw", gout_a, grad_a), ("channels_last", gout_b, grad_b)):
        exact, bound = R.grad_f64(kp_a.cpu().numpy(), gout.cpu().numpy(), geom, 2, Cb, H, W)
        R.assert_within_bound(grad.permute(0, 2, 3, 1).cpu().numpy(), exact, bound, name=f"map gradient, {name} feed")
    assert grad_b.is_contiguous(memory_format=torch.channels_last)
