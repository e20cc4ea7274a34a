"""Half-precision inference of the 3-D sparse backbones: k_spconv_h16 (csrc/sparse_conv_half.hip), its fp16 weight fragments, the narrowing operation,
the two launch-list operations and the route from EVAL_DTYPE / set_eval_dtype down to them.  Every layer is held to tests/half_reference.py's derived
bound against float64 fed with the layer's own fp16 input; the narrowing operation and the fragments are bitwise torch.Tensor.half()."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import half_reference as H
from seeding import seeded_state_dict
from test_spconv import EPILOGUES, KITTI_GEOMETRY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPILOGUE_SETS = dict(EPILOGUES, none=())
TAPS = ("x_conv1", "x_conv2", "x_conv3", "x_conv4")


def _backbone(name, cfg=None, channels=3, grid=KITTI_GEOMETRY[2]):
    from seevcn_amd.pcdet.models import backbones_3d
    return backbones_3d.__all__[name]({} if cfg is None else cfg, channels, grid)


# ---------------------------------------------------------------------------------- CPU: the bound, on an emulation of the kernel's arithmetic
_CASES = {}


def _case(ti, cin, cout):
    """(table tag, nbr, x16, w, terms, z, p) of table ti at (cin, cout): operands and float64 products made once, shared and never written"""
    key = (ti, cin, cout)
    if key not in _CASES:
        t = H.tables()[ti]
        nbr, n_in = H.oracle_table(t)
        rng = np.random.default_rng(1000 * ti + cin + cout)
        x16, w, terms = H.operands(rng, n_in, nbr.shape[1], nbr.shape[0], cin, cout)
        _CASES[key] = (t[0], nbr, x16, w, terms) + H.products(x16, nbr, w)
    return _CASES[key]


@pytest.mark.parametrize("cin,cout", H.CHANNELS)
def test_fp32_emulation_meets_the_bound_on_every_case(cin, cout):
    for ti in range(len(H.tables())):
        tag, nbr, x16, w, terms, z, p = _case(ti, cin, cout)
        assert nbr.shape[1] >= 1 and (nbr >= 0).any(), tag
        for ename, names in EPILOGUE_SETS.items():
            for store in H.STORES:
                y64, tol = H.expected(z, p, cin, terms, names, store)
                got = H.emulate(x16, nbr, w, terms, names, store)
                H.assert_within(got, y64, tol, name=f"emulation {cin}->{cout} {tag} {ename} {store}")


@pytest.mark.parametrize("fault,names,store,channels", [
    # fp16 partial sums: 2^-12 |sum| per addition.  The sparse 300-site table gives a row two or three additions, and at C_in = 128 the bound's own
    # accumulation term, 3460 * 2^-23 * P = 2^-11.2 * P, is wider than that: the fault is seen up to C_in = 64
    ("acc16", ("relu",), "float32", H.CHANNELS[:5]),
    ("no_residual", EPILOGUES["all"], "float16", H.CHANNELS),
    ("swap", EPILOGUES["scale+shift"], "float16", H.CHANNELS),
    ("truncate", EPILOGUES["bias"], "float16", H.CHANNELS[:3])])       # up to 2^-10 |y| against 2^-11 |y| + E_acc: seen where E_acc (~ C_in) is small
def test_checker_rejects_seeded_faults(fault, names, store, channels):
    ti = H.SUBM_ROWS.index(300)
    for cin, cout in channels:
        tag, nbr, x16, w, terms, z, p = _case(ti, cin, cout)
        y64, tol = H.expected(z, p, cin, terms, names, store)
        assert H.excess(H.emulate(x16, nbr, w, terms, names, store), y64, tol) <= 1.0
        assert H.excess(H.emulate(x16, nbr, w, terms, names, store, fault=fault), y64, tol) > 1.0, (fault, cin, cout)


def test_truncate_half_is_truncation():
    v = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -20, -(1.0 + 2.0 ** -10 + 2.0 ** -11 + 2.0 ** -20), 1.0, 70000.0, -3.0e-8], dtype=torch.float32)
    got = H.truncate_half(v).float()
    assert got.tolist() == [1.0, -(1.0 + 2.0 ** -10), 1.0, 65504.0, -0.0] and bool((got.abs() <= v.abs()).all())


# ---------------------------------------------------------------------------------- CPU: ABI, row layout, public surface
NEW_SYMBOLS = {
    "sv_conv_h16_applies": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_int64]),
    "sv_conv_weight_fragments_h16": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int64] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2),
    "sv_conv_weight_fragments_h16_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]),
    "sv_sparse_conv_gather_gemm_planned_h16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int64] + [ctypes.c_int] * 3
                                               + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p]),
    "sv_narrow_h16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
}


def test_half_symbols_are_declared_exported_and_bound(hip_lib):
    from seevcn_amd import _lib
    header = open(os.path.join(ROOT, "include", "seevcn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, sig in NEW_SYMBOLS.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(hip_lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(sig[1])
    assert re.search(r"#define\s+SV_OP_CONV_PLANNED_H16\s+16\b", code) and re.search(r"#define\s+SV_OP_NARROW_H16\s+17\b", code)
    # the shape query and the empty calls touch no device
    for K, kd, nc, n, want in [(27, 16, 16, 10, 1), (3, 128, 128, 10, 1), (27, 64, 32, 0, 1), (28, 64, 64, 10, 0), (0, 64, 64, 10, 0), (27, 48, 64, 10, 0),
                               (27, 64, 48, 10, 0), (27, 64, 256, 10, 0), (27, 4, 16, 10, 0), (27, 128, 128, (1 << 24) - 1, 1), (27, 128, 128, 1 << 24, 0),
                               (27, 16, 16, -1, 0)]:
        assert hip_lib.sv_conv_h16_applies(K, kd, nc, n) == want, (K, kd, nc, n)
    assert hip_lib.sv_narrow_h16(None, 0, None, None) == 0
    assert hip_lib.sv_conv_weight_fragments_h16_batch(None, 0, 0, None) == 0
    assert hip_lib.sv_sparse_conv_gather_gemm_planned_h16(None, 0, None, None, None, None, None, 0, 0, 27, 64, 64, None, None, None, None, 0, None) == 0


def test_half_launch_rows_word_by_word():
    from seevcn_amd.spconv import chain
    plan = (101, 102, 103, 999, 2, False)                                           # table_rows, perm, masks_p; the deal (tile_of, tiles_per_wave) is not carried
    r = chain.CONV_PLANNED_H16(plan, X16=11, n_src=7, wfrag16=12, Y=13, y_is_f32=True, n_rows=9, K=27, Kd=64, Nc=128, relu=1, bias=14, scale=15, shift=16,
                               residual16=17)
    want = [0] * 32
    want[0] = 16
    want[1:6] = [27, 64, 128, 1, 1]                                                 # i: K, Kd, Nc, relu, y_is_f32
    want[9:11] = [7, 9]                                                             # n: n_src, n_rows
    want[17:27] = [11, 101, 102, 103, 12, 13, 14, 15, 16, 17]                       # p: X16, table_rows, perm, masks_p, wfrag16, Y, bias, scale, shift, residual16
    assert r == want and len(r) == chain.WORDS
    r = chain.CONV_PLANNED_H16(plan, X16=11, n_src=7, wfrag16=12, Y=13, y_is_f32=False, n_rows=9, K=3, Kd=16, Nc=16)
    assert r[1:6] == [3, 16, 16, 0, 0] and r[23:32] == [0] * 9
    r = chain.NARROW_H16(x_f32=21, n_elems=4099, y_f16=22)
    want = [0] * 32
    want[0], want[9], want[17], want[18] = 17, 4099, 21, 22
    assert r == want
    assert (chain.OP_CONV_PLANNED_H16, chain.OP_NARROW_H16) == (16, 17)


def test_eval_dtype_parsing_and_set_eval_dtype():
    for name in ("VoxelBackBone8x", "VoxelResBackBone8x"):
        m = _backbone(name)
        assert m._eval_dtype == torch.float32 and m.last_eval_route is None
        assert _backbone(name, {"EVAL_DTYPE": "float32"})._eval_dtype == torch.float32
        h = _backbone(name, {"EVAL_DTYPE": "float16"})
        assert h._eval_dtype == torch.float16
        assert all(p.dtype == torch.float32 for p in h.parameters()) and all(b.dtype in (torch.float32, torch.int64) for b in h.buffers())
        assert list(h.state_dict()) == list(m.state_dict())                         # the dtype is a property of the route, not of the module
        assert m.set_eval_dtype(torch.float16) is m and m._eval_dtype == torch.float16
        assert m.set_eval_dtype("float32")._eval_dtype == torch.float32
        for bad in ("bfloat16", torch.bfloat16, torch.float64, "half", None, 16, ["float16"]):
            with pytest.raises(ValueError):
                m.set_eval_dtype(bad)
        assert m._eval_dtype == torch.float32                                       # a rejected value changes nothing
        with pytest.raises(ValueError):
            _backbone(name, {"EVAL_DTYPE": "bfloat16"})


# ---------------------------------------------------------------------------------- GPU: narrowing and fragments, bitwise
def _bits16(t):
    return t.contiguous().view(torch.int16)


SPECIALS = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 6.0e-8, 1.0e-8,
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23, 65504.0, 65519.0, 65520.0, -65520.0, 70000.0, -1.0e6, 3.0e38]


@pytest.mark.gpu
def test_hip_narrow_h16_is_bitwise_half(cuda, hip_lib):
    from seevcn_amd.spconv import chain, functional as Fsp
    rng = np.random.default_rng(5)
    for n in (1, 7, 8, 4099):
        v = (rng.normal(size=n) * 10.0 ** rng.uniform(-9, 5, size=n)).astype(np.float32)
        v[:min(n, len(SPECIALS))] = np.array(SPECIALS, np.float32)[:n]
        if n == 4099:
            v[-len(SPECIALS):] = np.array(SPECIALS, np.float32)                     # the scalar tail sees them too
        x = torch.from_numpy(v)
        want = _bits16(x.half())
        got = Fsp.narrow_h16(x.to(cuda))
        assert torch.equal(_bits16(got).cpu(), want), n
        # unaligned source and destination (the scalar path), and the launch-list form
        src = torch.empty(n + 1, dtype=torch.float32, device=cuda)[1:]
        src.copy_(x)
        dst = torch.full((n + 3,), 7.0, dtype=torch.float16, device=cuda)
        out = dst[1:1 + n]
        assert src.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 2
        chain._run([chain.NARROW_H16(x_f32=src.data_ptr(), n_elems=n, y_f16=out.data_ptr())], "SV_OP_NARROW_H16")
        assert torch.equal(_bits16(out).cpu(), want) and float(dst[0]) == 7.0 and float(dst[n + 1]) == 7.0 and float(dst[n + 2]) == 7.0, n
    assert hip_lib.sv_narrow_h16(None, 5, None, None) == 1


def _fragment_order(w16):
    """(K, C_in, C_out) -> the flat order sv_conv_weight_fragments_h16 documents"""
    K, cin, cout = w16.shape
    E = 8 if cin >= 32 else 4
    KQ, NT = cin // (4 * E), cout // 16
    # [k][q][kk][j] x [t][li] -> [k][q][t][kk][li][j]
    return w16.reshape(K, KQ, 4, E, NT, 16).permute(0, 1, 4, 2, 5, 3).contiguous().reshape(-1)


@pytest.mark.gpu
def test_hip_weight_fragments_h16_are_bitwise_half(cuda, hip_lib):
    from seevcn_amd import _lib
    from seevcn_amd.spconv import functional as Fsp
    rng = np.random.default_rng(6)
    ws = []
    for q, (cin, cout, K) in enumerate([(16, 16, 27), (16, 32, 27), (32, 64, 27), (64, 64, 3), (64, 128, 27), (128, 128, 27), (32, 48, 2)]):
        w = (rng.normal(size=(cout, K, cin)) * 10.0 ** rng.uniform(-9, 5, size=(cout, K, cin))).astype(np.float32)      # the parameter's own layout
        w.reshape(-1)[:len(SPECIALS)] = np.array(SPECIALS, np.float32)
        ws.append(torch.from_numpy(w).to(cuda).permute(1, 2, 0))                    # a strided (K, C_in, C_out) view
    frags, rows, unit0 = [], [], 0
    for w in ws:
        K, cin, cout = w.shape
        assert not w.is_contiguous()
        want = _bits16(_fragment_order(w.cpu().half()))
        single = torch.full((K * cin * cout,), float("nan"), dtype=torch.float16, device=cuda)
        sk, si, so = w.stride()
        _lib.check(hip_lib.sv_conv_weight_fragments_h16(w.data_ptr(), sk, si, so, K, cin, cout, single.data_ptr(), _lib.stream()), "sv_conv_weight_fragments_h16")
        assert torch.equal(_bits16(single).cpu(), want), (cin, cout)
        batch = torch.full_like(single, float("nan"))
        frags.append((batch, want))
        rows.append([w.data_ptr(), sk, si, so, K, cin, cout, batch.data_ptr(), 0, unit0])
        unit0 += K * cin * cout // (8 if cin >= 32 else 4)
    table = torch.tensor(rows, dtype=torch.int64).to(cuda)
    _lib.check(hip_lib.sv_conv_weight_fragments_h16_batch(table.data_ptr(), len(rows), unit0, _lib.stream()), "sv_conv_weight_fragments_h16_batch")
    for batch, want in frags:
        assert torch.equal(_bits16(batch).cpu(), want)
    # the cache's half side: nothing until asked, the same bits, re-laid after an in-place change
    Fsp.fragment_cache.clear()
    w = ws[2]
    assert not Fsp.fragment_cache._h
    f = Fsp.fragment_cache.get_half(w)
    assert torch.equal(_bits16(f).cpu(), frags[2][1]) and len(Fsp.fragment_cache._h) == 1
    w._base.mul_(2.0)
    Fsp.fragment_cache.refresh_all_half(ws)
    f2 = Fsp.fragment_cache.get_half(w)
    assert f2.data_ptr() == f.data_ptr() and torch.equal(_bits16(f2).cpu(), _bits16(_fragment_order(w.cpu().half())))
    assert hip_lib.sv_conv_weight_fragments_h16(ws[0].data_ptr(), 1, 1, 1, 27, 48, 16, f.data_ptr(), None) == 1          # C_in 48: no layout


# ---------------------------------------------------------------------------------- GPU: one layer against float64
def _device_table(t, cuda):
    from seevcn_amd.spconv import functional as Fsp
    tag, coords, batch, shape, ksize, stride, padding, subm = t
    c = torch.from_numpy(coords).to(cuda)
    if subm:
        return Fsp.build_subm_rulebook(c, batch, list(shape), list(ksize))
    return Fsp.build_sparse_rulebook(c, batch, list(shape), list(ksize), list(stride), list(padding))


def _gpu_layer(Fsp, dev, plan, frag, n_out, K, cin, cout, names, store, out=None):
    kw = dict(bias=dev["bias"] if "bias" in names else None, scale=dev["scale"] if "scale" in names else None, shift=dev["shift"] if "scale" in names else None,
              residual16=dev["residual"] if "residual" in names else None, relu="relu" in names)
    return Fsp.gather_gemm_planned_h16(dev["x16"], plan, frag, n_out, K, cin, cout, out_dtype=getattr(torch, store), out=out, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", H.CHANNELS)
def test_hip_h16_layer_vs_float64(cuda, hip_lib, cin, cout):
    """sv_sparse_conv_gather_gemm_planned_h16 on every table of the shared list (1 .. 300 rows, K = 27 submanifold and stride 2, K = 3), every subset of the
    epilogue terms, both store types: each output element within the derived bound of float64 on the same fp16 operands; the device's table is the
    oracle's; a second run gives the same bits; an unaligned Y (single-element stores) gives the bits of the whole-row store."""
    from seevcn_amd.spconv import functional as Fsp
    worst = 0.0
    for ti, t in enumerate(H.tables()):
        tag, nbr, x16, w, terms, z, p = _case(ti, cin, cout)
        rb = _device_table(t, cuda)
        K, n_out = nbr.shape
        assert rb.n_out == n_out and np.array_equal(rb.nbr_out.cpu().numpy(), nbr), tag
        plan = rb.plan("fwd", cin, cout)
        assert plan is not None, tag
        wd = w.to(cuda)
        frag = Fsp.fragment_cache.get_half(wd)
        dev = {k: v.to(cuda) for k, v in terms.items()}
        dev["x16"] = x16.to(cuda)
        for ename, names in EPILOGUE_SETS.items():
            for store in H.STORES:
                y64, tol = H.expected(z, p, cin, terms, names, store)
                got = _gpu_layer(Fsp, dev, plan, frag, n_out, K, cin, cout, names, store)
                assert got.dtype == getattr(torch, store)
                e = H.excess(got.cpu(), y64, tol)
                worst = max(worst, e)
                assert e <= 1.0, (f"{cin}->{cout} {tag} {ename} {store}", "largest error / bound", e)
                if ename in ("all", "none"):
                    again = _gpu_layer(Fsp, dev, plan, frag, n_out, K, cin, cout, names, store)
                    assert torch.equal(again.view(torch.uint8), got.view(torch.uint8)), (tag, ename, store, "second run")
                    # Y one element off 16-byte alignment, sentinels around it: the narrow-store path, nothing written outside
                    buf = torch.full((n_out * cout + 2,), 123.0, dtype=got.dtype, device=cuda)
                    out = buf[1:1 + n_out * cout].view(n_out, cout)
                    assert out.data_ptr() % 16 != 0
                    _gpu_layer(Fsp, dev, plan, frag, n_out, K, cin, cout, names, store, out=out)
                    assert torch.equal(out.contiguous().view(torch.uint8), got.view(torch.uint8)), (tag, ename, store, "unaligned Y")
                    assert float(buf[0]) == 123.0 and float(buf[-1]) == 123.0
    print(f"h16 layer {cin}->{cout}: largest error / bound over all cases {worst:.3f}")


@pytest.mark.gpu
def test_hip_h16_layer_padding_and_argument_errors(cuda, hip_lib):
    """A 17-row table: the second tile holds one row and fifteen -1 -- none of them is written (Y beyond the rows keeps its sentinel) or read.  Bad channels,
    a null table and scale without shift return SV_ERR_ARG and launch nothing (Y untouched)."""
    from seevcn_amd import _lib
    from seevcn_amd.spconv import functional as Fsp
    ti = H.SUBM_ROWS.index(17)
    tag, nbr, x16, w, terms, z, p = _case(ti, 32, 64)
    rb = _device_table(H.tables()[ti], cuda)
    tp = rb.plan("fwd", 32, 64)[0]
    perm = tp.perm.cpu().numpy()
    assert len(perm) == 32 and (perm[17:] == -1).all() and sorted(perm[:17]) == list(range(17))
    frag = Fsp.fragment_cache.get_half(w.to(cuda))
    xd = x16.to(cuda)
    y = torch.full((17 + 15, 64), 9.0, dtype=torch.float16, device=cuda)
    args = lambda **o: [o.get("x", xd.data_ptr()), 17, o.get("tab", tp.rows.data_ptr()), tp.perm.data_ptr(), tp.masks_p.data_ptr(), frag.data_ptr(), y.data_ptr(), 0,
                        17, 27, o.get("kd", 32), o.get("nc", 64), None, o.get("scale"), None, None, 0, _lib.stream()]
    assert hip_lib.sv_sparse_conv_gather_gemm_planned_h16(*args()) == 0
    y64, tol = H.expected(z, p, 32, terms, (), "float16")
    H.assert_within(y[:17].cpu(), y64, tol, name="17 rows")
    assert bool((y[17:] == 9.0).all())
    y.fill_(9.0)
    for bad in (dict(kd=48), dict(nc=48), dict(nc=256), dict(tab=None), dict(x=None), dict(scale=frag.data_ptr())):
        assert hip_lib.sv_sparse_conv_gather_gemm_planned_h16(*args(**bad)) == 1, bad
    torch.cuda.synchronize()
    assert bool((y == 9.0).all())


# ---------------------------------------------------------------------------------- GPU: the backbones
def _kitti_batch(cuda, n_scenes=2, n_az=100, seed=2000):
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.models.backbones_3d import vfe
    pts, _ = synth.make_scene_batch(n_scenes, seed=seed, n_az=n_az)
    pc_range, vs, grid = KITTI_GEOMETRY
    bd = {"batch_size": n_scenes, "points": torch.from_numpy(pts).to(cuda)}
    return vfe.__all__["DynMeanVFE"](model_cfg={}, num_point_features=3, voxel_size=vs, grid_size=grid, point_cloud_range=pc_range)(bd)


def _built(name, cuda, cfg=None, seed=1):
    m = _backbone(name, cfg)
    m.load_state_dict(seeded_state_dict(m, seed=seed))
    return m.to(cuda).eval()


def _forward(m, bd, grad=False):
    with (torch.enable_grad() if grad else torch.no_grad()):
        out = m(dict(bd))
    taps = dict(out["multi_scale_3d_features"])
    taps["out"] = out["encoded_spconv_tensor"]
    return taps


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for name in a:
        fa, fb = a[name].features.detach(), b[name].features.detach()
        assert torch.equal(a[name].indices, b[name].indices) and fa.dtype == fb.dtype == torch.float32 and torch.equal(fa, fb), (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_convs", [("VoxelBackBone8x", 12), ("VoxelResBackBone8x", 21)])
def test_hip_half_backbone_every_layer_vs_float64(cuda, hip_lib, name, n_convs):
    """2 scenes on the KITTI geometry, seeded weights and running statistics, EVAL_DTYPE float16: the forward takes the half route; every entry's output
    (launch list with all outputs kept) is within the per-layer bound of float64 fed with the GPU's own fp16 output of the entry in front, the fp16-rounded
    weights and the GPU's own fp32 BatchNorm coefficients -- the residual entries of VoxelResBackBone8x included; entry 0 is the fp32 route's output narrowed
    bit for bit.  The last tap is fp32, the others widen on `.features` and keep the fp32 route's indices and shapes."""
    import seevcn_amd.spconv as spconv
    from seevcn_amd import _lib
    from seevcn_amd.spconv import chain
    bd = _kitti_batch(cuda)
    m = _built(name, cuda, {"EVAL_DTYPE": "float16"})
    before = {k: v.clone() for k, v in m.state_dict().items()}
    half = _forward(m, bd)
    assert m.last_eval_route == "half"
    m.set_eval_dtype("float32")
    full = _forward(m, bd)
    assert m.last_eval_route == "chain"
    assert all(torch.equal(v, before[k]) and v.dtype == before[k].dtype for k, v in m.state_dict().items())
    for tap in TAPS:
        assert isinstance(half[tap], chain.HalfTap) and half[tap].features_half.dtype == torch.float16
        f = half[tap].features
        assert f.dtype == torch.float32 and f is half[tap].features and torch.equal(f, half[tap].features_half.float())
        assert torch.equal(half[tap].indices, full[tap].indices) and f.shape == full[tap].features.shape and half[tap].spatial_shape == full[tap].spatial_shape
    assert type(half["out"]) is spconv.SparseConvTensor and half["out"].features.dtype == torch.float32
    assert torch.equal(half["out"].indices, full["out"].indices) and half["out"].features.shape == full["out"].features.shape
    scale_out = float(full["out"].features.abs().max())
    dev_out = float((half["out"].features - full["out"].features).abs().max()) / scale_out
    print(f"{name}: fp16 list vs fp32 list on the last tap, max |diff| / max |out| = {dev_out:.2e} (reported, not asserted)")

    # every entry, teacher-forced
    entries = m._chain_blocks()
    assert len(entries) == n_convs
    x = spconv.SparseConvTensor(bd["voxel_features"], bd["voxel_coords"].int(), m.sparse_shape, 2)
    spconv.prebuild_rulebooks(m, x, with_backward=False)
    with torch.no_grad():
        assert chain.eval_half_applicable(entries, x)
        outs = chain._run_eval_chain_half(entries, x, keep_all=True)
        first32 = m.conv_input(x).features                                           # the fp32 input layer (the module tree gives the fp32 list's bits)
    assert len(outs) == n_convs and all(o.dtype == torch.float16 for o in outs[:-1]) and outs[-1].dtype == torch.float32
    assert torch.equal(_bits16(outs[0]), _bits16(first32.half()))
    for tap, k in zip(TAPS + ("out",), [k for k, e in enumerate(entries) if e.tap]):
        assert torch.equal(outs[k].view(torch.uint8), (half[tap].features_half if tap != "out" else half[tap].features).view(torch.uint8)), tap
    # the GPU's own coefficients (the kernel the list runs)
    coefs = [torch.empty(2 * e.cout, dtype=torch.float32, device=cuda) for e in entries]
    jobs = np.zeros((n_convs, 8), dtype=np.int64)
    for k, e in enumerate(entries):
        jobs[k, :7] = (e.bn.weight.data_ptr(), e.bn.bias.data_ptr(), e.bn.running_mean.data_ptr(), e.bn.running_var.data_ptr(), coefs[k].data_ptr(), e.cout,
                       chain._bits(e.bn.eps))
    _lib.check(hip_lib.sv_batchnorm_eval_coef_batch(jobs.ctypes.data, n_convs, _lib.stream()), "sv_batchnorm_eval_coef_batch")
    worst, n_res = 0.0, 0
    for k in range(1, n_convs):
        e = entries[k]
        rb = x.indice_dict[e.conv.indice_key]
        nbr = rb.nbr_out.cpu().numpy()
        w = e.conv.weight_kio_nograd().detach().cpu().contiguous()
        z, p = H.products(outs[k - 1].cpu(), nbr, w)
        c = coefs[k].cpu()
        terms = {"scale": c[:e.cout], "shift": c[e.cout:]}
        names = ["scale", "relu"]
        if e.conv.bias is not None:
            terms["bias"], names = e.conv.bias.detach().cpu(), names + ["bias"]
        if e.residual_from is not None:
            terms["residual"], names, n_res = outs[e.residual_from].cpu(), names + ["residual"], n_res + 1
        store = "float32" if k == n_convs - 1 else "float16"
        y64, tol = H.expected(z, p, e.cin, terms, names, store)
        err = H.excess(outs[k].cpu(), y64, tol)
        worst = max(worst, err)
        assert err <= 1.0, (name, "entry", k, f"{e.cin}->{e.cout}", "largest error / bound", err)
        assert (y64 > 0).mean() > 0.02, (k, "the ReLU must not hide the layer")
    assert n_res == (8 if name == "VoxelResBackBone8x" else 0)
    print(f"{name}: largest error / bound over entries 1..{n_convs - 1}: {worst:.3f}")


@pytest.mark.gpu
def test_hip_half_route_stands_down(cuda, hip_lib):
    """EVAL_DTYPE left at its default, gradients enabled, a norm in train(), a conv with C_out = 48: none takes the half route (last_eval_route says which
    one ran) and each gives the bits of the same model asked for float32."""
    import seevcn_amd.spconv as spconv
    bd = _kitti_batch(cuda, n_az=90)
    name = "VoxelResBackBone8x"
    # default dtype
    m, ref = _built(name, cuda), _built(name, cuda, {"EVAL_DTYPE": "float32"})
    got, want = _forward(m, bd), _forward(ref, bd)
    assert m.last_eval_route == "chain" and ref.last_eval_route == "chain"
    _same_bits(got, want, "default dtype")
    # the half route itself is taken by this model when asked, and differs
    h = _built(name, cuda, {"EVAL_DTYPE": "float16"})
    half = _forward(h, bd)
    assert h.last_eval_route == "half" and not torch.equal(half["out"].features, want["out"].features)
    # gradients enabled
    got, want_g = _forward(h, bd, grad=True), _forward(ref, bd, grad=True)
    assert h.last_eval_route == "modules" and ref.last_eval_route == "modules"
    _same_bits(got, want_g, "gradients enabled")
    # a norm in train()
    h2, r2 = _built(name, cuda, {"EVAL_DTYPE": "float16"}), _built(name, cuda)
    for mm in (h2, r2):
        mm.conv2[1].bn1.train()
    got, want_t = _forward(h2, bd), _forward(r2, bd)
    assert h2.last_eval_route == "modules" and r2.last_eval_route == "modules"
    _same_bits(got, want_t, "a norm in train mode")
    # a conv with C_out = 48 (no fp16 kernel, and no fused BatchNorm either: the module tree)
    def with_48(cfg):
        mm = _backbone("VoxelBackBone8x", cfg)
        mm.conv_out = spconv.SparseSequential(spconv.SparseConv3d(64, 48, (3, 1, 1), stride=(2, 1, 1), padding=0, bias=False, indice_key="spconv_down2"),
                                              torch.nn.BatchNorm1d(48, eps=1e-3, momentum=0.01), torch.nn.ReLU())
        mm.load_state_dict(seeded_state_dict(mm, seed=3))
        return mm.to(cuda).eval()
    h3, r3 = with_48({"EVAL_DTYPE": "float16"}), with_48(None)
    got, want_48 = _forward(h3, bd), _forward(r3, bd)
    assert h3.last_eval_route == r3.last_eval_route and h3.last_eval_route in ("chain", "modules")
    assert got["out"].features.shape[1] == 48
    _same_bits(got, want_48, "C_out = 48")


@pytest.mark.gpu
def test_hip_half_route_follows_the_live_buffers(cuda, hip_lib):
    """running_var and a conv weight changed in place between two forwards: each changes the output (the coefficients and the fp16 fragments are made from
    the live tensors on every forward), and the result equals a fresh model's with the same state."""
    bd = _kitti_batch(cuda, n_az=90)
    m = _built("VoxelBackBone8x", cuda, {"EVAL_DTYPE": "float16"})
    first = _forward(m, bd)["out"].features.clone()
    with torch.no_grad():
        m.conv3[1][1].running_var.mul_(1.7)
    second = _forward(m, bd)["out"].features.clone()
    with torch.no_grad():
        m.conv4[2][0].weight.mul_(-0.5)
    third = _forward(m, bd)["out"].features.clone()
    assert m.last_eval_route == "half"
    assert not torch.equal(first, second) and not torch.equal(second, third)
    fresh = _backbone("VoxelBackBone8x", {"EVAL_DTYPE": "float16"})
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(cuda).eval()
    assert torch.equal(_forward(fresh, bd)["out"].features, third) and fresh.last_eval_route == "half"


@pytest.mark.gpu
def test_hip_second_detector_predicts_in_half_precision(cuda, hip_lib):
    """SECONDNet on 2 scenes with EVAL_DTYPE: float16 predicts without error through the half route; against the fp32 run of the same weights at most 2 % of
    the box count may differ."""
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import detectors
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=100)
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda)}
    counts = {}
    for dtype in ("float32", "float16"):
        cfg = C.second_model_cfg()
        cfg["BACKBONE_3D"] = dict(cfg["BACKBONE_3D"], EVAL_DTYPE=dtype)
        net = detectors.build_detector(cfg, num_class=3, dataset=C.SyntheticDatasetInfo())
        net.load_state_dict(seeded_state_dict(net, seed=4))
        net = net.to(cuda).eval()
        np.random.seed(0)
        torch.manual_seed(0)
        with torch.no_grad():
            preds, _ = net(dict(batch))
        assert net.backbone_3d.last_eval_route == ("half" if dtype == "float16" else "chain")
        assert len(preds) == 2 and all(bool(torch.isfinite(p["pred_boxes"]).all()) and bool(torch.isfinite(p["pred_scores"]).all()) for p in preds)
        counts[dtype] = sum(len(p["pred_scores"]) for p in preds)
        del net
    print(f"SECONDNet boxes: fp32 {counts['float32']}, fp16 {counts['float16']}")
    assert counts["float32"] > 0
    assert abs(counts["float16"] - counts["float32"]) <= 0.02 * counts["float32"], counts
