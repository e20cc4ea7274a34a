"""RoI-aware point feature pooling (Part-A2): sv_roiaware_assign / sv_roiaware_pool / the two backwards and the RoIAwarePool3d module against the
numpy restatement in tests/roiaware_pool_reference.py.

Inputs leave nothing to rounding: an inside point is drawn in its box's frame at a cell centre +- at most 0.3 of the cell per axis, an outside
point at least 0.2 of a cell beyond the surface on one axis, both rotated to the LiDAR frame in float64 and then cast to fp32; a float64 check of
the INPUTS (`_clearance`) then keeps only points that are, for EVERY box of the case, either 0.1 of a cell outside on some axis or 0.1 of a cell
away from every cell wall and the surface -- three orders of magnitude more than fp32 moves them.  So every point is compared, none excluded."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import roiaware_pool_reference as R
from oracle.tolerances import assert_close_per_channel


# ---------------------------------------------------------------------------------------------------------------- inputs
def _local(boxes, pts):
    """float64 box-frame coordinates (N, M, 3) of pts (M, 3) for boxes (N, 7)."""
    b, p = np.asarray(boxes, np.float64), np.asarray(pts, np.float64)
    s = p[None, :, :] - b[:, None, :3]
    c, sn = np.cos(-b[:, 6])[:, None], np.sin(-b[:, 6])[:, None]
    return np.stack([s[..., 0] * c - s[..., 1] * sn, s[..., 0] * sn + s[..., 1] * c, s[..., 2]], -1)


def _clearance(boxes, pts, out):
    """(safe (N, M) bool, inside (N, M) bool) in float64: safe = clearly outside on some axis, or clearly inside a cell on all three."""
    b = np.asarray(boxes, np.float64)
    loc = _local(boxes, pts)
    cell = b[:, None, 3:6] / np.asarray(out, np.float64)
    beyond = (np.abs(loc) - b[:, None, 3:6] / 2) / cell                # > 0: outside on that axis, in cells
    outside = (beyond > 0.1).any(-1)
    frac = (loc + b[:, None, 3:6] / 2) / cell
    wall = np.abs(frac - np.round(frac))                                # distance to the nearest cell wall (the surface is one), in cells
    inside = (beyond < -0.1).all(-1) & (wall > 0.1).all(-1)
    return outside | inside, inside


def _to_lidar(box, loc):
    c, s = np.cos(box[6]), np.sin(box[6])
    return np.stack([box[0] + loc[:, 0] * c - loc[:, 1] * s, box[1] + loc[:, 0] * s + loc[:, 1] * c, box[2] + loc[:, 2]], 1)


def _boxes(rng, n, spacing=40.0):
    """Boxes 0.5 .. 10 m a side, headings in +-3.2, far enough apart that no point of one reaches another."""
    k = np.arange(n)
    centre = np.stack([spacing * (k % 9), spacing * (k // 9), rng.uniform(-1, 1, n)], 1)
    return np.concatenate([centre, rng.uniform(0.5, 10.0, (n, 3)), rng.uniform(-3.2, 3.2, (n, 1))], 1)


def _draw(rng, boxes, out, n_pts, inside_frac, hot=None, hot_frac=0.3, hot_at=(), avoid_hot=False):
    """n_pts points for `boxes` (float64 (N, 7)), each drawn for a random owner box and kept only if _clearance calls it safe for every box.
    hot: one cell index (3,) per box that takes hot_frac of the box's inside points; hot_at: point rows forced into box 0's hot cell;
    avoid_hot: no other point may fall into it."""
    out_a = np.asarray(out)
    pts = np.zeros((n_pts, 3), np.float32)
    for i in range(n_pts):
        for _ in range(1000):
            o = rng.integers(len(boxes))
            d = boxes[o, 3:6]
            if i in hot_at or rng.uniform() < inside_frac:
                cell = rng.integers(0, out_a)
                if i in hot_at:
                    o, d, cell = 0, boxes[0, 3:6], hot[0]
                elif hot is not None and not avoid_hot and rng.uniform() < hot_frac:
                    cell = hot[o]
                elif avoid_hot and hot is not None and o == 0 and (cell == hot[0]).all():
                    continue
                loc = -d / 2 + (cell + 0.5 + rng.uniform(-0.3, 0.3, 3)) * d / out_a
            else:
                loc = rng.uniform(-0.5, 0.5, 3) * d
                ax = rng.integers(3)
                loc[ax] = rng.choice([-1.0, 1.0]) * (d[ax] / 2 + (0.2 + rng.uniform(0, 1)) * d[ax] / out_a[ax])
            p = _to_lidar(boxes[o], loc[None]).astype(np.float32)
            if _clearance(boxes, p, out)[0].all():
                pts[i] = p[0]
                break
        else:
            raise AssertionError("no safe point found")
    return pts


@functools.lru_cache(maxsize=None)
def _case(seed, n_boxes, n_pts, out, inside_frac=0.7, kind="spread"):
    rng = np.random.default_rng(seed)
    out = tuple(out)
    hot_at, avoid = (), False
    if kind == "spread":
        boxes = _boxes(rng, n_boxes)
    elif kind == "nested":                                              # the same centre and heading, sides x1, x1.7, x2.3: shared points
        boxes = np.repeat(_boxes(rng, 1), n_boxes, 0)
        boxes[:, 3:6] *= np.array([1.0, 1.7, 2.3])[:n_boxes, None]
    elif kind == "order":                                               # one cell's points at chosen rows, nobody else in that cell
        boxes = _boxes(rng, 1)
        hot_at, avoid = (0, 63, 64, 255, 256, 999), True
    elif kind == "all_and_none":                                        # box 0 holds every point, box 1 none
        boxes = _boxes(rng, 2)
    hot = rng.integers(0, np.asarray(out), (max(len(boxes), 1), 3)) if len(boxes) else None
    if len(boxes) == 0:
        pts = rng.uniform(-5, 5, (n_pts, 3)).astype(np.float32)
    elif kind == "all_and_none":
        pts = _draw(rng, boxes[:1], out, n_pts, 1.0, hot[:1])
        assert _clearance(boxes, pts, out)[0].all()
    else:
        pts = _draw(rng, boxes, out, n_pts, inside_frac, hot, hot_at=hot_at, avoid_hot=avoid)
    rois = boxes.astype(np.float32).reshape(-1, 7)
    safe, inside = _clearance(rois, pts, out)                           # the fp32 inputs themselves, for every (box, point) pair
    assert safe.all()
    return SimpleNamespace(rois=rois, pts=pts, out=out, inside=inside, hot=hot)


@functools.lru_cache(maxsize=None)
def _want_lists(key, cap):
    c = _case(*key)
    return R.assign(c.rois, c.pts, c.out, cap)


def _dev_assign(cuda, rois, pts, out, cap, rng_=None):
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as U
    r = None if rng_ is None else torch.from_numpy(np.asarray(rng_, np.int32)).to(cuda)
    return U.assign_points_to_cells(torch.from_numpy(rois).to(cuda), torch.from_numpy(pts).to(cuda), out, cap, r)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_restatement_hand_case():
    """One axis-aligned 4 x 2 x 2 box at the origin on a (2, 1, 2) grid and one turned by pi / 2; cap 3 keeps the two earliest rows of a cell."""
    rois = np.array([[0, 0, 0, 4, 2, 2, 0], [10, 0, 0, 4, 2, 2, np.pi / 2]], np.float32)
    pts = np.array([[-1, 0, -0.5],        # box 0 cell (0, 0, 0)
                    [1, 0.5, 0.5],        # box 0 cell (1, 0, 1)
                    [-1.5, -0.5, -0.2],   # box 0 cell (0, 0, 0)
                    [-0.5, 0.2, -0.9],    # box 0 cell (0, 0, 0): the third of a cap-3 cell, dropped
                    [0, 0, 1.5],          # above
                    [2.5, 0, 0],          # beyond +x
                    [10, 1, 0.5],         # box 1: local x = +1 -> cell (1, 0, 1)
                    [10.5, -1.5, -0.5]],  # box 1: local x = -1.5 -> cell (0, 0, 0)
                   np.float32)
    lists = R.assign(rois, pts, (2, 1, 2), 3)
    assert lists.shape == (2, 2, 1, 2, 3)
    assert lists[0, 0, 0, 0].tolist() == [2, 0, 2] and lists[0, 1, 0, 1, :2].tolist() == [1, 1]
    assert lists[0, 0, 0, 1, 0] == 0 and lists[0, 1, 0, 0, 0] == 0
    assert lists[1, 1, 0, 1, :2].tolist() == [1, 6] and lists[1, 0, 0, 0, :2].tolist() == [1, 7]
    assert lists[..., 0].sum() == 5
    feat = np.array([[1, -1], [2, -2], [1, -3], [9, 9], [9, 9], [9, 9], [-4, -4], [0.5, 0.25]], np.float32)
    mx, arg = R.pool(lists, feat, "max")
    assert mx[0, 0, 0, 0].tolist() == [1, -1] and arg[0, 0, 0, 0].tolist() == [0, 0]          # tie on channel 0: the first row wins
    assert mx[1, 1, 0, 1].tolist() == [-4, -4] and arg[1, 1, 0, 1].tolist() == [6, 6]          # an all-negative cell keeps its maximum
    assert mx[0, 0, 0, 1].tolist() == [0, 0] and arg[0, 0, 0, 1].tolist() == [-1, -1]          # an empty cell
    av, none = R.pool(lists, feat, "avg")
    assert none is None and av[0, 0, 0, 0].tolist() == [1, -2] and av[0, 1, 0, 0].tolist() == [0, 0]
    g = np.ones((2, 2, 1, 2, 2))
    gm = R.pool_backward(lists, arg, g, 8, "max")
    assert gm[:, 0].tolist() == [1, 1, 0, 0, 0, 0, 1, 1] and gm[:, 1].tolist() == [1, 1, 0, 0, 0, 0, 1, 1]
    ga = R.pool_backward(lists, None, g, 8, "avg")
    assert ga[:, 0].tolist() == [0.5, 1, 0.5, 0, 0, 0, 1, 1]
    other = lists.copy()
    other[0, 0, 0, 0, 2] = 3
    assert R.lists_equal(lists, lists) and not R.lists_equal(other, lists)
    other = lists.copy()
    other[0, 0, 0, 1, 1] = 99                                                                   # behind the count: not compared
    assert R.lists_equal(other, lists)


def test_inputs_leave_nothing_to_rounding():
    """The construction's claim, on the CPU: the fp32 restatement puts every point of a case where the float64 construction put it."""
    for key in [(3, 3, 257, (3, 5, 2)), (4, 3, 257, (12, 12, 12)), (5, 3, 300, (12, 12, 12), 0.7, "nested")]:
        c = _case(*key)
        for b, box in enumerate(c.rois):
            inside, cell = R.cells_of_points(box, c.pts, c.out)
            assert np.array_equal(inside, c.inside[b])
            loc = _local(c.rois[b:b + 1], c.pts)[0]
            want = np.floor((loc + c.rois[b, 3:6].astype(np.float64) / 2) / (c.rois[b, 3:6].astype(np.float64) / np.asarray(c.out))).astype(np.int64)
            assert np.array_equal(cell[inside], want[inside])


def test_cpu_tensors_are_refused(hip_lib):
    import seevcn_amd._lib as L
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as U
    with pytest.raises(L.SeevcnHipError):
        U.assign_points_to_cells(torch.zeros(1, 7), torch.zeros(4, 3), 2, 4)
    with pytest.raises(L.SeevcnHipError):
        U.RoIAwarePool3d(2, 4)(torch.zeros(1, 7), torch.zeros(4, 3), torch.zeros(4, 2))


def test_entries_refuse_bad_arguments(hip_lib):
    """The C entries themselves, without a GPU: every refusal comes before the first device call that needs one."""
    import ctypes
    buf = (ctypes.c_float * 64)()
    host = ctypes.cast(buf, ctypes.c_void_p)
    for out, cap in [((256, 1, 1), 4), ((1, 256, 1), 4), ((1, 1, 256), 4), ((17, 17, 17), 4), ((0, 1, 1), 4), ((2, 2, 2), 1)]:
        assert hip_lib.sv_roiaware_assign(host, 1, host, 1, None, *out, cap, host, None) != 0
        assert b"roiaware_assign" in hip_lib.sv_last_error()
    assert hip_lib.sv_roiaware_assign(None, 1, None, 0, None, 2, 2, 2, 4, None, None) != 0          # null pointers
    assert b"null" in hip_lib.sv_last_error()
    assert hip_lib.sv_roiaware_assign(None, 0, None, 5, None, 2, 2, 2, 4, None, None) == 0          # no boxes: nothing to do
    assert hip_lib.sv_roiaware_pool(None, 4, None, 1, 4097, 4, 0, None, None, None) != 0
    assert hip_lib.sv_roiaware_pool(None, 4, None, 1, 8, 1, 0, None, None, None) != 0
    assert hip_lib.sv_roiaware_pool(None, 4, None, 1, 8, 4, 2, None, None, None) != 0               # pool_method
    assert hip_lib.sv_roiaware_pool(None, 4, None, 0, 8, 4, 0, None, None, None) == 0
    assert hip_lib.sv_roiaware_pool_backward(None, None, None, 1, 8, 4, 4, 0, 0, None, None) == 0   # no points: nothing to do
    assert hip_lib.sv_roiaware_pool_backward(None, None, None, 1, 8, 4, 4, 0, 3, None, None) != 0
    assert hip_lib.sv_roiaware_pool_backward_ordered(None, None, None, 1, 8, 4, 4, 0, 3, None, None, None) != 0
    assert hip_lib.sv_roiaware_pool_backward_ordered_scratch_bytes(1 << 20, 4096, 128, 128, 0, 10) == 0   # 2^39 keys


def test_module_surface():
    import seevcn_amd
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as U
    m = U.RoIAwarePool3d(12, 128)
    assert m.out_size == 12 and m.max_pts_each_voxel == 128 and not list(m.parameters())
    assert U.RoIAwarePool3d((3, 5, 2)).max_pts_each_voxel == 128
    assert "roiaware_pool" in seevcn_amd.ordered_gradient_calls()


# ---------------------------------------------------------------------------------------------------------------- GPU: lists
LIST_CASES = {
    # name: ((seed, n_boxes, n_pts, out[, inside_frac, kind]), caps)
    "one_cell": ((11, 1, 65, (1, 1, 1)), (2, 5, 128)),
    "anisotropic": ((12, 3, 257, (3, 5, 2)), (2, 5, 128)),
    "twelve": ((13, 3, 1000, (12, 12, 12)), (5, 128)),
    "fourteen": ((14, 3, 257, (14, 14, 14)), (128,)),
    "seventy_boxes": ((15, 70, 1000, (3, 5, 2)), (5,)),
    "no_points": ((16, 3, 0, (3, 5, 2)), (5,)),
    "one_point": ((17, 1, 1, (3, 5, 2), 1.0), (5,)),
    "sixty_three": ((18, 3, 63, (3, 5, 2)), (5,)),
    "sixty_five": ((19, 3, 65, (3, 5, 2)), (5,)),
    "order_across_chunks": ((20, 1, 1000, (3, 5, 2), 0.7, "order"), (128,)),
    "nested_boxes": ((21, 2, 300, (12, 12, 12), 0.7, "nested"), (5, 128)),
    "all_and_none": ((22, 2, 257, (3, 5, 2), 1.0, "all_and_none"), (5, 128)),
    "hot_cell_over_cap_128": ((23, 1, 1000, (1, 1, 1), 0.9), (128,)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LIST_CASES))
def test_lists_bit_exact(cuda, name):
    key, caps = LIST_CASES[name]
    c = _case(*key)
    full = {}
    for cap in caps:
        want = _want_lists(key, cap)
        got = _dev_assign(cuda, c.rois, c.pts, c.out, cap).cpu().numpy()
        assert R.lists_equal(got, want), (name, cap)
        full[cap] = bool((want[..., 0] == cap - 1).any() and (c.inside.sum() > want[..., 0].sum()))
    if name == "order_across_chunks":
        h = c.hot[0]
        assert want[0, h[0], h[1], h[2], :7].tolist() == [6, 0, 63, 64, 255, 256, 999]
    if name == "all_and_none":
        assert c.inside[0].all() and want[0, ..., 0].sum() == len(c.pts) and want[1, ..., 0].sum() == 0
    for cap in {"hot_cell_over_cap_128": (128,), "anisotropic": (2, 5), "one_cell": (2, 5)}.get(name, ()):
        assert full[cap]                                                          # cells with more points than the cap: the earliest survive
    if name == "nested_boxes":
        assert (c.inside.sum(0) == 2).any()                                       # points that two boxes list


@pytest.mark.gpu
def test_lists_no_boxes(cuda):
    c = _case(16, 3, 0, (3, 5, 2))
    pts = _case(12, 3, 257, (3, 5, 2)).pts
    got = _dev_assign(cuda, np.zeros((0, 7), np.float32), pts, (3, 5, 2), 5)
    assert tuple(got.shape) == (0, 3, 5, 2, 5)
    assert c.pts.shape == (0, 3)


@pytest.mark.gpu
def test_lists_batched_equal_single_scene_calls(cuda):
    """Two scenes stacked, ranges that start and end off any multiple of 64: one launch with box_pt_range = two single-scene calls with each
    scene's start added back."""
    a, b = _case(31, 3, 257, (3, 5, 2)), _case(32, 2, 300, (3, 5, 2))
    pad = np.full((37, 3), 500.0, np.float32)                                     # rows no box looks at; scene a starts at 37, b at 294
    pts = np.concatenate([pad, a.pts, b.pts, pad])
    rois = np.concatenate([a.rois, b.rois])
    rng_ = np.array([[37, 294]] * 3 + [[294, 594]] * 2, np.int32)
    cap = 5
    got = _dev_assign(cuda, rois, pts, (3, 5, 2), cap, rng_).cpu().numpy()
    assert R.lists_equal(got, R.assign(rois, pts, (3, 5, 2), cap, rng_))
    for part, c, start in ((got[:3], a, 37), (got[3:], b, 294)):
        single = _dev_assign(cuda, c.rois, c.pts, (3, 5, 2), cap).cpu().numpy()
        shifted = single.copy()
        shifted[..., 1:] += start
        assert R.lists_equal(part, shifted)
        assert R.lists_equal(single, _want_lists((31, 3, 257, (3, 5, 2)) if c is a else (32, 2, 300, (3, 5, 2)), cap))
    # box a[0] pointed at scene b's rows finds nothing of its own there
    alone = _dev_assign(cuda, a.rois[:1], pts, (3, 5, 2), cap, np.array([[294, 594]], np.int32)).cpu().numpy()
    assert R.lists_equal(alone, R.assign(a.rois[:1], pts, (3, 5, 2), cap, np.array([[294, 594]], np.int32)))


# ---------------------------------------------------------------------------------------------------------------- GPU: pooling
POOL_KEYS = {"small": ((41, 3, 257, (3, 5, 2)), 5), "sparse": ((42, 3, 300, (12, 12, 12), 0.7, "nested"), 128)}


def _features(n, C, seed, negative=False):
    """Rows drawn from 6 distinct ones, so that most cells hold ties; negative: every value below zero."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((6, C)).astype(np.float32)
    if negative:
        base = -np.abs(base) - np.float32(0.5)
    return base[rng.integers(0, 6, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 4, 16, 17, 128])
@pytest.mark.parametrize("which", sorted(POOL_KEYS))
def test_pool_forward(cuda, which, C):
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as U
    key, cap = POOL_KEYS[which]
    c = _case(*key)
    lists = _want_lists(key, cap)
    dev_lists = _dev_assign(cuda, c.rois, c.pts, c.out, cap)
    assert R.lists_equal(dev_lists.cpu().numpy(), lists)
    assert (lists[..., 0] == 0).any() and (lists[..., 0] > 1).any()
    for negative in (False, True):
        feat = _features(len(c.pts), C, 7 + C, negative)
        f = torch.from_numpy(feat).to(cuda)
        want, arg = R.pool(lists, feat, "max")
        ctx = SimpleNamespace()
        got = U.RoIAwarePoolFromListsFunction.forward(ctx, f, dev_lists, "max")
        got_arg = ctx.roiaware_pool3d_for_backward[1]
        assert np.array_equal(got.cpu().numpy().astype(np.float64), want)                  # the winning value itself
        assert np.array_equal(got_arg.cpu().numpy(), arg)                                  # ties: the first listed row
        empty = lists[..., 0] == 0
        assert (got.cpu().numpy()[empty] == 0).all() and (got_arg.cpu().numpy()[empty] == -1).all()
        if negative:
            assert (got.cpu().numpy()[~empty] < 0).all()                                   # an all-negative cell keeps its maximum
        want_avg, _ = R.pool(lists, feat, "avg")
        got_avg = U.RoIAwarePoolFromListsFunction.forward(SimpleNamespace(), f, dev_lists, "avg")
        assert_close_per_channel(got_avg.cpu().numpy(), want_avg, name=f"avg pool C={C}")
        assert (got_avg.cpu().numpy()[empty] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["max", "avg"])
@pytest.mark.parametrize("C", [4, 17])
def test_pool_backward(cuda, method, C):
    """Both routes against float64; three nested boxes list the same points.  With the switch on two backwards are bit-identical and the counter
    advances; with it off it does not."""
    import seevcn_amd
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as U
    key, cap = (43, 3, 300, (3, 5, 2), 0.8, "nested"), 128
    c = _case(*key)
    assert (c.inside.sum(0) == 3).any()                                                    # a point listed by three boxes
    lists = _want_lists(key, cap)
    feat = _features(len(c.pts), C, 3)
    _, arg = R.pool(lists, feat, method)
    rng = np.random.default_rng(5)
    g = rng.standard_normal(lists.shape[:-1] + (C,)).astype(np.float32)
    want = R.pool_backward(lists, arg, g, len(c.pts), method)
    pool = U.RoIAwarePool3d(c.out, cap)
    rois, pts, gd = torch.from_numpy(c.rois).to(cuda), torch.from_numpy(c.pts).to(cuda), torch.from_numpy(g).to(cuda)

    def run():
        f = torch.from_numpy(feat).to(cuda).requires_grad_(True)
        pool(rois, pts, f, method).backward(gd)
        return f.grad.cpu().numpy()

    calls = seevcn_amd.ordered_gradient_calls()["roiaware_pool"]
    assert_close_per_channel(run(), want, name=f"{method} backward, atomics")
    assert seevcn_amd.ordered_gradient_calls()["roiaware_pool"] == calls
    with seevcn_amd.set_ordered_gradients(True):
        first, second = run(), run()
    assert seevcn_amd.ordered_gradient_calls()["roiaware_pool"] == calls + 2
    assert_close_per_channel(first, want, name=f"{method} backward, ordered")
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- GPU: module
@pytest.mark.gpu
def test_module(cuda):
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as U
    key = (42, 3, 300, (12, 12, 12), 0.7, "nested")
    c = _case(*key)
    rois, pts = torch.from_numpy(c.rois).to(cuda), torch.from_numpy(c.pts).to(cuda)
    f4, f16 = torch.from_numpy(_features(len(c.pts), 4, 1)).to(cuda), torch.from_numpy(_features(len(c.pts), 16, 2)).to(cuda)
    pool = U.RoIAwarePool3d(12, 128)
    out = pool(rois, pts, f16, pool_method="max")
    assert tuple(out.shape) == (3, 12, 12, 12, 16) and out.dtype == torch.float32
    want, _ = R.pool(_want_lists(key, 128), f16.cpu().numpy(), "max")
    assert np.array_equal(out.cpu().numpy().astype(np.float64), want)
    triple = U.RoIAwarePool3d((3, 5, 2), 5)(rois, pts, f4, "avg")
    assert tuple(triple.shape) == (3, 3, 5, 2, 4)
    with pytest.raises(AssertionError):
        pool(rois, pts, f4, pool_method="sum")
    avg, mx = pool.forward_multi(rois, pts, [f4, f16], ["avg", "max"])
    assert torch.equal(avg, pool(rois, pts, f4, "avg")) and torch.equal(mx, out)
    empty = pool(rois[:0], pts, f4, "max")
    assert tuple(empty.shape) == (0, 12, 12, 12, 4)
