"""PointRCNN's RoI point pooling: sv_roipoint_pool3d through roipoint_pool3d_cuda.forward, and the RoIPointPool3d module, against the numpy
restatement in tests/roipoint_pool_reference.py.

Inputs leave nothing to rounding: a point is drawn in a box's frame, rotated to the LiDAR frame in float64 and cast to fp32; a float64 check of
the fp32 INPUTS (`_state`) then keeps it only if it is at least 1e-3 m clear of the surface of EVERY box of the case, otherwise it is redrawn.
An fp32 evaluation of the in-box test and a float64 one disagree only below 1e-5 m of clearance (boxes 0.3 - 10 m in the KITTI range, headings in
+-3.2), so no (box, point) pair is excluded from any comparison; test_input_recipe_classifies_alike guards that on the CPU for every case."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import roipoint_pool_reference as R

CLEAR = 1e-3
# box centres far enough apart that boxes of up to 10 m a side never touch, inside the KITTI range
GRID = [(x, y) for y in (-24.0, 0.0, 24.0) for x in (12.0, 34.0, 56.0)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _state(boxes, pts):
    """(safe (M, N), inside (M, N)) in float64: safe = at least CLEAR outside on some axis, or at least CLEAR inside on all three."""
    b = np.asarray(boxes, np.float64).reshape(-1, 7)
    d = np.abs(R.local64(boxes, pts)) - b[:, None, 3:6] / 2
    inside = (d < -CLEAR).all(-1)
    return inside | (d > CLEAR).any(-1), inside


def _boxes(rng, n, headings=None):
    centre = np.concatenate([np.asarray(GRID[:n]), rng.uniform(-1.5, 0.0, (n, 1))], 1)
    rz = rng.uniform(-3.2, 3.2, (n, 1)) if headings is None else np.asarray(headings, np.float64).reshape(n, 1)
    return np.concatenate([centre, rng.uniform(0.3, 10.0, (n, 3)), rz], 1).astype(np.float32)


def _draw(rng, boxes, owner):
    """One point per entry of owner: inside box owner[i] (and wherever else that puts it), or with owner[i] < 0 inside no box; every point is
    CLEAR away from every box's surface.  boxes: the fp32 values the kernel will see."""
    owner = np.asarray(owner, np.int64)
    b64 = boxes.astype(np.float64)
    pts = np.zeros((len(owner), 3), np.float32)
    todo = np.arange(len(owner))
    for _ in range(400):
        if len(todo) == 0:
            return pts
        o = owner[todo]
        src = np.where(o >= 0, o, rng.integers(0, len(boxes), len(todo)))
        bx = b64[src]
        loc = rng.uniform(-1, 1, (len(todo), 3)) * bx[:, 3:6] * np.where(o >= 0, 0.495, 1.5)[:, None]
        c, s = np.cos(bx[:, 6]), np.sin(bx[:, 6])
        p = np.stack([bx[:, 0] + loc[:, 0] * c - loc[:, 1] * s, bx[:, 1] + loc[:, 0] * s + loc[:, 1] * c, bx[:, 2] + loc[:, 2]], 1).astype(np.float32)
        safe, inside = _state(boxes, p)
        ok = safe.all(0) & np.where(o >= 0, inside[np.maximum(o, 0), np.arange(len(todo))], ~inside.any(0))
        pts[todo[ok]] = p[ok]
        todo = todo[~ok]
    raise AssertionError("no safe point found")


def _owners(rng, n, counts):
    """n owners: counts[m] rows for box m at random positions, -1 elsewhere."""
    owner = np.full(n, -1, np.int64)
    rows = rng.permutation(n)[:sum(counts)]
    owner[rows] = np.repeat(np.arange(len(counts)), counts)
    return owner


def _make(seed, boxes, owners, C, extra_width=0.0):
    """boxes (M, 7) shared by len(owners) scenes; the points are drawn against the boxes enlarged by extra_width (fp32 sum)."""
    rng = np.random.default_rng(seed + 977)
    test_boxes = boxes.copy()
    test_boxes[:, 3:6] = test_boxes[:, 3:6] + np.float32(extra_width)
    xyz = np.stack([_draw(rng, test_boxes, o) for o in owners]) if len(owners[0]) else np.zeros((len(owners), 0, 3), np.float32)
    feat = rng.standard_normal((len(owners), xyz.shape[1], C)).astype(np.float32)
    return SimpleNamespace(xyz=xyz, feat=feat, boxes=np.repeat(boxes[None], len(owners), 0), test_boxes=test_boxes)


def _forced(n, rows):
    owner = np.full(n, -1, np.int64)
    owner[list(rows)] = 0
    return owner


@functools.lru_cache(maxsize=None)
def _case(name, n=None):
    rng = np.random.default_rng(sum(map(ord, name)) + (n or 0))
    if name == "order":                     # insiders straddle the wave (64), workgroup (256) and trip boundaries; cnt 7 < S = 16
        return _make(1, _boxes(rng, 1), [_forced(1000, (0, 63, 64, 255, 256, 257, 999))], 4)
    if name == "early_stop":                # S = 3: row 600 must not appear
        return _make(2, _boxes(rng, 1), [_forced(1000, (254, 255, 256, 600))], 4)
    if name == "counts":                    # S = 64
        return _make(3, _boxes(rng, 6), [_owners(rng, 777, (0, 1, 63, 64, 65, 300))], 5)
    if name == "s_edge":                    # S in {1, 100, 512}; box 2 holds 700
        return _make(4, _boxes(rng, 5), [_owners(rng, 2000, (0, 5, 700, 100, 513))], 130)
    if name == "all_inside":
        return _make(5, _boxes(rng, 1), [np.zeros(1024, np.int64)], 2)
    if name == "n_edge":
        return _make(6, _boxes(rng, 3), [rng.integers(-1, 3, n)], 3)
    if name == "scenes":
        return _make(7, _boxes(rng, 4), [rng.integers(-1, 4, 300) for _ in range(3)], 6)
    if name == "nested":                    # the same centre and heading, sides x1, x1.7, x2.3: shared points
        b = np.repeat(_boxes(rng, 1), 3, 0)
        b[:, 3:6] *= np.array([1.0, 1.7, 2.3], np.float32)[:, None]
        return _make(8, b, [rng.integers(-1, 3, 400)], 4)
    if name == "headings":
        h = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 3.2, -3.2])
        return _make(9, _boxes(rng, 7, h), [rng.integers(-1, 7, 500)], 4)
    if name == "module":                    # drawn against the boxes enlarged by 0.2
        return _make(10, _boxes(rng, 4), [rng.integers(-1, 4, 300) for _ in range(2)], 7, extra_width=0.2)
    raise KeyError(name)


N_EDGE = (1, 63, 64, 65, 255, 256, 257)
# (case key, S values)
RUNS = [(("order",), (16,)), (("early_stop",), (3,)), (("counts",), (64,)), (("s_edge",), (1, 100, 512)), (("all_inside",), (512,)),
        (("scenes",), (32,)), (("nested",), (64,)), (("headings",), (32,))] + [(("n_edge", n), (16,)) for n in N_EDGE]
PARAMS = [pytest.param(key, s, id="-".join(map(str, key)) + f"-S{s}") for key, ss in RUNS for s in ss]


@functools.lru_cache(maxsize=None)
def _want(key, S, canonical):
    c = _case(*key)
    return R.pool(c.xyz, c.feat, c.test_boxes[None].repeat(len(c.xyz), 0), S, canonical)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_input_recipe_classifies_alike():
    """The restatement's fp32 classification equals the float64 one for every (box, point) pair of every case, and the forced rows are what the
    cases say they are."""
    keys = [k for k, _ in RUNS] + [("module",)]
    pairs = 0
    for key in keys:
        c = _case(*key)
        for xyz in c.xyz:
            if len(xyz) == 0:
                continue
            safe, inside = _state(c.test_boxes, xyz)
            assert safe.all(), key
            assert np.array_equal(R.inside_fp32(c.test_boxes, xyz), inside), key
            assert np.array_equal(R.inside_f64(c.test_boxes, xyz), inside), key
            pairs += inside.size
    assert pairs > 30000
    assert np.flatnonzero(R.inside_fp32(_case("order").test_boxes, _case("order").xyz[0])[0]).tolist() == [0, 63, 64, 255, 256, 257, 999]
    idx, cnt = R.lists(_case("early_stop").xyz, _case("early_stop").boxes, 3)
    assert idx[0, 0].tolist() == [254, 255, 256]
    assert R.inside_fp32(_case("counts").test_boxes, _case("counts").xyz[0]).sum(1).tolist() == [0, 1, 63, 64, 65, 300]
    assert R.inside_fp32(_case("s_edge").test_boxes, _case("s_edge").xyz[0]).sum(1).tolist() == [0, 5, 700, 100, 513]
    assert R.lists(_case("all_inside").xyz, _case("all_inside").boxes, 512)[0][0, 0].tolist() == list(range(512))
    idx, cnt = R.lists(_case("order").xyz, _case("order").boxes, 16)
    assert idx[0, 0].tolist() == [[0, 63, 64, 255, 256, 257, 999][k % 7] for k in range(16)]


def test_registered_in_the_bindings():
    import seevcn_amd._lib as L
    assert "sv_roipoint_pool3d" in L.SIGNATURES
    from seevcn_amd.pcdet.ops.roipoint_pool3d import roipoint_pool3d_cuda, roipoint_pool3d_utils
    assert callable(roipoint_pool3d_cuda.forward)
    m = roipoint_pool3d_utils.RoIPointPool3d()
    assert (m.num_sampled_points, m.pool_extra_width) == (512, 1.0)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _run(cuda, xyz, feat, boxes, S, canonical):
    """The kernel on outputs pre-filled with NaN and 7: every element must be written."""
    from seevcn_amd.pcdet.ops.roipoint_pool3d import roipoint_pool3d_cuda
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    pooled = torch.full((boxes.shape[0], boxes.shape[1], S, 3 + feat.shape[2]), float("nan"), dtype=torch.float32, device=cuda)
    flag = torch.full((boxes.shape[0], boxes.shape[1]), 7, dtype=torch.int32, device=cuda)
    if canonical is None:
        assert roipoint_pool3d_cuda.forward(t(xyz), t(boxes), t(feat), pooled, flag) == 1          # the reference-shaped call
    else:
        assert roipoint_pool3d_cuda.forward(t(xyz), t(boxes), t(feat), pooled, flag, canonical=canonical) == 1
    return pooled.cpu().numpy(), flag.cpu().numpy()


def _check_plain(got, flag, want, want_flag):
    assert np.array_equal(flag, want_flag)
    assert np.array_equal(_bits(got), _bits(want))


def _check_canonical(got, flag, plain, want64, want_flag, bound):
    """Features and flags bit-identical to canonical = 0, z bit-exact, x / y within the bound of float64."""
    assert np.array_equal(flag, want_flag)
    assert np.array_equal(_bits(got[..., 3:]), _bits(plain[..., 3:]))
    assert np.array_equal(_bits(got[..., 2]), _bits(want64[..., 2].astype(np.float32)))
    err = np.abs(got[..., 0:2].astype(np.float64) - want64[..., 0:2])
    assert np.isfinite(got).all()
    worst = (err - bound[..., None]).max() if err.size else 0.0
    print("canonical x/y: largest error %.3e, largest error / bound %.3f" % (err.max() if err.size else 0.0,
                                                                              (err / np.maximum(bound[..., None], 1e-30)).max() if err.size else 0.0))
    assert worst <= 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("key,S", PARAMS)
def test_pool_matches_restatement(cuda, key, S):
    c = _case(*key)
    want, want_flag = _want(key, S, False)
    got, flag = _run(cuda, c.xyz, c.feat, c.boxes, S, None)
    _check_plain(got, flag, want, want_flag)
    want64, want_flag64, bound = _want(key, S, True)
    got_c, flag_c = _run(cuda, c.xyz, c.feat, c.boxes, S, True)
    _check_canonical(got_c, flag_c, got, want64, want_flag64, bound)


@pytest.mark.gpu
def test_empty_sizes(cuda):
    c = _case("scenes")
    B, N, C = c.feat.shape
    for canonical in (False, True):
        got, flag = _run(cuda, c.xyz, c.feat, c.boxes[:, :0], 8, canonical)                         # n_boxes = 0
        assert got.shape == (B, 0, 8, 3 + C) and flag.shape == (B, 0)
        got, flag = _run(cuda, c.xyz[:, :0], c.feat[:, :0], c.boxes, 8, canonical)                  # n_pts = 0: every box empty
        assert (flag == 1).all() and np.array_equal(_bits(got), np.zeros(got.shape, np.uint32))
    want, want_flag = R.pool(c.xyz, c.feat[:, :, :0], c.boxes, 8)                                   # C = 0: rows of xyz only
    got, flag = _run(cuda, c.xyz, c.feat[:, :, :0], c.boxes, 8, False)
    _check_plain(got, flag, want, want_flag)
    want64, _, bound = R.pool(c.xyz, c.feat[:, :, :0], c.boxes, 8, True)
    got_c, flag_c = _run(cuda, c.xyz, c.feat[:, :, :0], c.boxes, 8, True)
    _check_canonical(got_c, flag_c, got, want64, want_flag, bound)


@pytest.mark.gpu
def test_bad_arguments(cuda):
    import seevcn_amd._lib as L
    from seevcn_amd.pcdet.ops.roipoint_pool3d import roipoint_pool3d_cuda
    c = _case("scenes")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    B, M, C = c.boxes.shape[0], c.boxes.shape[1], c.feat.shape[2]
    pooled = torch.empty((B, M, 8, 3 + C), dtype=torch.float32, device=cuda)
    flag = torch.empty((B, M), dtype=torch.int32, device=cuda)
    with pytest.raises(L.SeevcnHipError):                                                           # a CPU tensor
        roipoint_pool3d_cuda.forward(torch.from_numpy(c.xyz), t(c.boxes), t(c.feat), pooled, flag)
    with pytest.raises(L.SeevcnHipError):                                                           # n_sampled = 0
        roipoint_pool3d_cuda.forward(t(c.xyz), t(c.boxes), t(c.feat), torch.empty((B, M, 0, 3 + C), dtype=torch.float32, device=cuda), flag)
    lib = L.load()
    xyz_d, boxes_d, feat_d = t(c.xyz), t(c.boxes), t(c.feat)
    host = np.ascontiguousarray(c.xyz)                                                              # a host pointer at the C entry itself
    rc = lib.sv_roipoint_pool3d(host.ctypes.data_as(ctypes.c_void_p), feat_d.data_ptr(), boxes_d.data_ptr(), B, c.xyz.shape[1], M, C, 8, 0,
                                pooled.data_ptr(), flag.data_ptr(), L.stream())
    assert rc != 0
    for bad in (dict(n_pts=-1), dict(n_sampled=0), dict(n_sampled=1 << 20), dict(C=-1), dict(canonical=2)):
        a = dict(batch=B, n_pts=c.xyz.shape[1], n_boxes=M, C=C, n_sampled=8, canonical=0)
        a.update(bad)
        rc = lib.sv_roipoint_pool3d(xyz_d.data_ptr(), feat_d.data_ptr(), boxes_d.data_ptr(), a["batch"], a["n_pts"], a["n_boxes"], a["C"],
                                    a["n_sampled"], a["canonical"], pooled.data_ptr(), flag.data_ptr(), L.stream())
        assert rc != 0, bad
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_module_matches_restatement_on_enlarged_boxes(cuda):
    from seevcn_amd.pcdet.ops.roipoint_pool3d.roipoint_pool3d_utils import RoIPointPool3d
    c = _case("module")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    layer = RoIPointPool3d(num_sampled_points=24, pool_extra_width=(0.2, 0.2, 0.2))
    enlarged = np.repeat(c.test_boxes[None], len(c.xyz), 0)
    want, want_flag = R.pool(c.xyz, c.feat, enlarged, 24)
    pooled, flag = layer(t(c.xyz), t(c.feat), t(c.boxes))
    assert flag.dtype == torch.int32
    _check_plain(pooled.cpu().numpy(), flag.cpu().numpy(), want, want_flag)
    want64, _, bound = R.pool(c.xyz, c.feat, enlarged, 24, True)
    pooled_c, flag_c = layer(t(c.xyz), t(c.feat), t(c.boxes), canonical=True)
    _check_canonical(pooled_c.cpu().numpy(), flag_c.cpu().numpy(), pooled.cpu().numpy(), want64, want_flag, bound)
    feat = t(c.feat).requires_grad_(True)
    out, _ = layer(t(c.xyz), feat, t(c.boxes))
    with pytest.raises(NotImplementedError):
        out.sum().backward()
