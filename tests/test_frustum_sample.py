"""sv_frustum_grid, sv_frustum_to_voxel and sv_frustum_to_voxel_grad (csrc/frustum_sample.hip, ops/frustum_ops.py, f2v/FrustumToVoxel) against the
float64 run of the restatement in tests/caddn_reference.py, which also holds the cases, the allowance (a multiple of the float32 CPU run's own
error, per case) and the mask of voxels next to the NaN -> -2 jump."""
import ctypes
import functools

import pytest
import torch

import caddn_reference as R
import seevcn_amd._lib as L
from seevcn_amd.pcdet.ops import frustum_ops

pytestmark = pytest.mark.gpu
GRAD_CASES = [n for n, c in R.CASES.items() if c["grad"]]


def _geometry(case):
    return case["grid_size"], case["pc_range"], case["disc"]


def _device_inputs(case, cuda, flip=False):
    x = R.make_inputs(case, torch.float32)
    order = [1, 0] if flip else [0, 1]
    return [t[order].to(cuda).contiguous() for t in (x.feats, x.probs, x.gout, x.lidar_to_cam, x.cam_to_img, x.image_shape)]


def _fused(case, cuda, flip=False, grad=True):
    """out (B, C, Z, Y, X) [, grad feats, grad probs] of the fused route, on the CPU, batch order undone"""
    feats, probs, gout, l2c, c2i, ishape = _device_inputs(case, cuda, flip)
    feats.requires_grad_(grad), probs.requires_grad_(grad)
    out = frustum_ops.frustum_to_voxel(feats, probs, l2c, c2i, ishape, *_geometry(case))
    res = [out.detach()]
    if grad:
        (out * gout).sum().backward()
        res += [feats.grad, probs.grad]
    order = [1, 0] if flip else [0, 1]
    return [t[order].cpu() for t in res]


@functools.lru_cache(maxsize=None)
def _grid_e32(name):
    case = R.CASES[name]
    x = R.make_inputs(case, torch.float32)
    g32 = R.frustum_grid(x.lidar_to_cam, x.cam_to_img, x.image_shape, case["grid_size"], case["pc_range"], case["disc"], torch.float32)
    ref = R.reference(name)
    same = ((g32 == -2) == (ref.grid == -2)) | ref.near.unsqueeze(-1)
    assert same.all(), "the float32 CPU run disagrees with float64 about a non-finite component away from the jump"
    return float(((g32.double() - ref.grid).abs() * ~ref.near.unsqueeze(-1)).max())


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "chunked"])
def test_grid_against_float64(name, cuda):
    ref, case = R.reference(name), R.CASES[name]
    _, _, _, l2c, c2i, ishape = _device_inputs(case, cuda)
    grid = frustum_ops.frustum_grid(l2c, c2i, ishape, *_geometry(case)).cpu()
    assert tuple(grid.shape) == (2,) + tuple(case["grid_size"]) + (3,)
    keep = ~ref.near.unsqueeze(-1).expand_as(grid)
    replaced = ref.grid == -2
    assert torch.equal((grid == -2)[keep], replaced[keep]), "a non-finite component is not -2 (or a finite one is)"
    err = float(((grid.double() - ref.grid).abs() * keep).max())
    allow = R.FWD_FACTOR * _grid_e32(name)
    print(f"{name}: grid err {err:.3e} allowance {allow:.3e}")
    assert err <= allow


@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_against_float64(name, cuda):
    ref, case = R.reference(name), R.CASES[name]
    out, = _fused(case, cuda, grad=False)
    assert tuple(out.shape) == tuple(ref.out.shape)
    keep = ~ref.near.permute(0, 3, 2, 1).unsqueeze(1)
    err = float(((out.double() - ref.out).abs() * keep).max())
    print(f"{name}: forward err {err:.3e} E32 {ref.e_fwd:.3e} allowance {R.FWD_FACTOR * ref.e_fwd:.3e}")
    assert torch.isfinite(out).all()
    assert err <= R.FWD_FACTOR * ref.e_fwd
    if name == "outside":
        assert (out == 0).all()


def test_output_storage_order(cuda):
    case = R.CASES["base_LID"]
    feats, probs, _, l2c, c2i, ishape = _device_inputs(case, cuda)
    out = frustum_ops.frustum_to_voxel(feats, probs, l2c, c2i, ishape, *_geometry(case))
    B, C, (X, Y, Z) = 2, case["C"], case["grid_size"]
    assert tuple(out.shape) == (B, C, Z, Y, X) and out.permute(0, 3, 4, 1, 2).is_contiguous()
    bev = out.flatten(1, 2)
    assert bev.data_ptr() == out.data_ptr() and bev.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradients_against_float64_autograd(name, cuda):
    ref, case = R.reference(name), R.CASES[name]
    _, gf, gp = _fused(case, cuda)
    err_f, err_p = float((gf.double() - ref.grad_feats).abs().max()), float((gp.double() - ref.grad_probs).abs().max())
    print(f"{name}: grad feats err {err_f:.3e} E32 {ref.e_grad_feats:.3e}; grad probs err {err_p:.3e} E32 {ref.e_grad_probs:.3e} "
          f"(allowance {R.GRAD_FACTOR} x E32)")
    assert torch.isfinite(gf).all() and torch.isfinite(gp).all()
    assert err_f <= R.GRAD_FACTOR * ref.e_grad_feats
    assert err_p <= R.GRAD_FACTOR * ref.e_grad_probs
    assert (gp[:, -1] == 0).all() and not torch.signbit(gp[:, -1]).any(), "the ignored last bin must get +0.0f"
    if name == "outside":
        assert (gf == 0).all() and (gp == 0).all()


@pytest.mark.parametrize("name", ["base_LID", "c130", "shapes"])
def test_gradients_bit_equal_run_to_run_and_with_the_batch_swapped(name, cuda):
    case = R.CASES[name]
    first = _fused(case, cuda)
    for _ in range(2):
        again = _fused(case, cuda)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    swapped = _fused(case, cuda, flip=True)                                # another voxel / key order at launch, the same order within a pixel
    assert all(torch.equal(a, b) for a, b in zip(first, swapped))


def _raw_grad(case, cuda, fill):
    feats, probs, gout, l2c, c2i, ishape = _device_inputs(case, cuda)
    f = feats.permute(0, 2, 3, 1).contiguous()
    p = probs.permute(0, 2, 3, 1).contiguous()
    g = gout.permute(0, 3, 4, 1, 2).contiguous()
    B, H, W, C = f.shape
    X, Y, Z = case["grid_size"]
    lib = L.load()
    scratch = torch.full((lib.sv_frustum_to_voxel_grad_scratch_bytes(B, H, W, X, Y, Z),), 0xA5, dtype=torch.uint8, device=cuda)
    gf, gp = torch.full_like(f, fill), torch.full_like(p, fill)
    rng = L.host_array(ctypes.c_float, list(case["pc_range"]))
    d = case["disc"]
    rc = lib.sv_frustum_to_voxel_grad(L.ptr(f), L.ptr(p), L.ptr(l2c), L.ptr(c2i), L.ptr(ishape), L.ptr(g), B, C, d["num_bins"], H, W, X, Y, Z, rng,
                                      frustum_ops.MODES[d["mode"]], d["depth_min"], d["depth_max"], L.ptr(scratch), L.ptr(gf), L.ptr(gp), L.stream())
    L.check(rc, "sv_frustum_to_voxel_grad")
    return gf.permute(0, 3, 1, 2).cpu(), gp.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("name", ["base_LID", "outside", "d1"])
def test_every_gradient_element_is_written(name, cuda):
    case = R.CASES[name]
    gf, gp = _raw_grad(case, cuda, float("nan"))
    assert not torch.isnan(gf).any() and not torch.isnan(gp).any()
    _, want_f, want_p = _fused(case, cuda)
    assert torch.equal(gf, want_f) and torch.equal(gp, want_p)


def _module(case, cuda):
    from seevcn_amd.pcdet.models.backbones_3d.vfe.image_vfe_modules.f2v import FrustumToVoxel
    cfg = dict(NAME="FrustumToVoxel", SAMPLER=dict(mode="bilinear", padding_mode="zeros"))
    return FrustumToVoxel(cfg, grid_size=case["grid_size"], pc_range=case["pc_range"], disc_cfg=case["disc"]).to(cuda)


def _batch_dict(feats, probs, l2c, c2i, ishape, fused):
    d = dict(trans_lidar_to_cam=l2c, trans_cam_to_img=c2i, image_shape=ishape)
    if fused:
        d.update(image_features=feats, depth_probs=probs)
    else:
        d.update(frustum_features=R.frustum_from_probs(feats, probs))
    return d


@pytest.mark.parametrize("name", ["base_LID", "base_SID", "shapes", "c64"])
def test_fused_route_against_module_tree_route(name, cuda, monkeypatch):
    ref, case = R.reference(name), R.CASES[name]
    feats, probs, _, l2c, c2i, ishape = _device_inputs(case, cuda)
    m = _module(case, cuda)
    assert m.fused
    fused = m(_batch_dict(feats, probs, l2c, c2i, ishape, True))["voxel_features"]
    monkeypatch.setenv("SEEVCN_FUSED_FRUSTUM", "0")
    assert not m.fused
    tree = m(_batch_dict(feats, probs, l2c, c2i, ishape, False))["voxel_features"]
    assert fused.shape == tree.shape
    err = float((fused - tree).abs().max())
    print(f"{name}: fused vs module tree {err:.3e} allowance {R.FWD_FACTOR * ref.e_fwd:.3e}")
    assert err <= R.FWD_FACTOR * ref.e_fwd
    other = _module(dict(case), cuda)
    other.sampler.mode = "nearest"
    assert not other.fused


def test_incoming_gradient_layouts_give_the_same_bits(cuda):
    case = R.CASES["base_LID"]
    got = []
    for layout in ("storage", "reference", "strided"):
        feats, probs, gout, l2c, c2i, ishape = _device_inputs(case, cuda)
        feats.requires_grad_(True), probs.requires_grad_(True)
        out = frustum_ops.frustum_to_voxel(feats, probs, l2c, c2i, ishape, *_geometry(case))
        if layout == "storage":                                            # the gradient arrives with the output's own strides: no copy
            g = gout.permute(0, 3, 4, 1, 2).contiguous().permute(0, 3, 4, 1, 2)
            assert g.stride() == out.stride()
        elif layout == "reference":                                        # a plain contiguous (B, C, Z, Y, X) gradient
            g = gout
        else:                                                              # every other element of a wider buffer
            wide = torch.zeros(gout.shape[:-1] + (2 * gout.shape[-1],), device=cuda)
            wide[..., ::2] = gout
            g = wide[..., ::2]
            assert not g.is_contiguous()
        out.backward(g)
        got.append((feats.grad.cpu(), probs.grad.cpu()))
    for gf, gp in got[1:]:
        assert torch.equal(gf, got[0][0]) and torch.equal(gp, got[0][1])


def test_size_guard_and_cpu_tensors(cuda):
    lib = L.load()
    assert lib.sv_frustum_to_voxel_grad_scratch_bytes(1, 9, 13, 11, 10, 3) > 0
    assert lib.sv_frustum_to_voxel_grad_scratch_bytes(1, 1 << 16, 1 << 15, 11, 10, 3) == 0          # B * H * W = 2^31
    assert lib.sv_frustum_to_voxel_grad_scratch_bytes(1, 9, 13, 1 << 10, 1 << 10, 1 << 9) == 0       # 4 * X * Y * Z = 2^31
    assert lib.sv_frustum_to_voxel_grad_scratch_bytes(1, 9, 13, 1 << 10, 1 << 10, (1 << 9) - 1) > 0
    case = R.CASES["base_LID"]
    feats, probs, gout, l2c, c2i, ishape = _device_inputs(case, cuda)
    rng = L.host_array(ctypes.c_float, list(case["pc_range"]))
    small = torch.zeros(1024, device=cuda)
    for dims in [(1 << 16, 1 << 15, 11, 10, 3), (9, 13, 1 << 10, 1 << 10, 1 << 9)]:
        H, W, X, Y, Z = dims
        rc = lib.sv_frustum_to_voxel_grad(L.ptr(small), L.ptr(small), L.ptr(l2c), L.ptr(c2i), L.ptr(ishape), L.ptr(small), 1, 5, 7, H, W, X, Y, Z, rng, 1, 2.0,
                                          11.0, L.ptr(small), L.ptr(small), L.ptr(small), L.stream())
        assert rc != 0 and b"int32" in lib.sv_last_error()
        rc = lib.sv_frustum_to_voxel(L.ptr(small), L.ptr(small), L.ptr(l2c), L.ptr(c2i), L.ptr(ishape), 1, 5, 7, H, W, X, Y, Z, rng, 1, 2.0, 11.0,
                                     L.ptr(small), L.stream())
        assert rc != 0
    torch.cuda.synchronize()
    x = R.make_inputs(case, torch.float32)
    with pytest.raises(L.SeevcnHipError):
        frustum_ops.frustum_to_voxel(x.feats, x.probs, x.lidar_to_cam, x.cam_to_img, x.image_shape, *_geometry(case))
    with pytest.raises(L.SeevcnHipError):
        frustum_ops.frustum_to_voxel(feats, probs, x.lidar_to_cam, c2i, ishape, *_geometry(case))
    with pytest.raises(L.SeevcnHipError):
        frustum_ops.frustum_grid(x.lidar_to_cam, x.cam_to_img, x.image_shape, *_geometry(case))


def test_fused_route_never_holds_the_frustum_volume(cuda, monkeypatch):
    """B = 1, C = 64, D = 80, a 47 x 156 map, grid 70 x 94 x 6: the (B, C, D, H, W) volume is 150 MB.  A condition on memory, not a timing."""
    B, C, D, H, W = 1, 64, 80, 47, 156
    case = dict(grid_size=(70, 94, 6), pc_range=(2., -30.08, -3., 46.8, 30.08, 1.), disc=dict(mode="LID", num_bins=D, depth_min=2.0, depth_max=46.8))
    volume_bytes = B * C * D * H * W * 4
    g = torch.Generator().manual_seed(0)
    feats0 = torch.randn((B, C, H, W), generator=g).to(cuda)
    probs0 = torch.softmax(torch.randn((B, D + 1, H, W), generator=g), dim=1).to(cuda)
    l2c = R._l2c(t=(0., -0.08, -0.27)).float().unsqueeze(0).to(cuda)
    c2i = R._c2i(fx=360.0, fy=360.0, cx=312.0, cy=94.0, t=(22.0, 0.1, 0.003)).float().unsqueeze(0).to(cuda)
    ishape = torch.tensor([[188, 624]], dtype=torch.int32, device=cuda)
    m = _module(case, cuda)
    peaks = {}
    for fused in (True, False):
        monkeypatch.setenv("SEEVCN_FUSED_FRUSTUM", "1" if fused else "0")
        feats = feats0.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        probs = probs0.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = m(_batch_dict(feats, probs, l2c, c2i, ishape, fused))["voxel_features"]
        out.sum().backward()
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - base
        assert float(out.detach().abs().sum()) > 0
        del out
    print(f"peak above the inputs: fused {peaks[True] / 1e6:.1f} MB, module tree {peaks[False] / 1e6:.1f} MB, volume {volume_bytes / 1e6:.1f} MB")
    assert peaks[True] < volume_bytes / 2 < peaks[False]
