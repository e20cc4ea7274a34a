"""Numpy restatement of the reference's local and frustum augmentors, the yardstick of tests/test_local_augment.py (test infrastructure only).

Restated, statement by statement (line numbers in detector3d/pcdet/datasets/augmentor/augmentor_utils.py):
  random_local_translation_along_x / _y / _z   :257-320        global_frustum_dropout_top / _bottom / _left / _right   :323-388
  local_scaling                                :391-422        local_rotation                                          :425-470
  local_frustum_dropout_*                      :473-550        get_points_in_box                                       :553-570
and the wrappers of datasets/augmentor/data_augmentor.py:134-219 inside prepare_scene (the scene-level function, extended from
augment_reference.prepare_scene, which stays as it is).  tests/golden/local_augment.npz holds what the reference's own functions gave on the
cases below; tests/test_local_augment_reference.py holds this file to it.

Dtypes.  Points and boxes are float32, the draws Python floats.  Every statement's arithmetic type is written out, under the value-based
casting the reference was written for, so that nothing here depends on the installed NumPy:
  float32 array  (op) Python float  -> float32, the scalar rounded first     points[mask, 0] += offset, points[mask, :3] *= noise_scale,
                                                                             gt_boxes[idx, 3:6] *= noise_scale, shift_x * cosa
  float32 scalar (op) Python float  -> float64                               gt_boxes[idx, 0] += offset and gt_boxes[idx, 6] += noise_rotation
                                                                             (rounded on assignment), dz / 2.0, dx / 2.0 + MARGIN, the thresholds
  float32 array (cmp) float64 scalar -> float32, the scalar rounded first    abs(local_x) <= dx / 2.0 + MARGIN, points[:, 2] >= threshold
  math.cos(-rz)                      -> float64 cosine, rounded where it meets shift_x
Under NumPy 2 the second kind stays float32: a threshold or an offset then differs by at most one rounding (2**-24 relative), far below the
ROBUST margin every decision of a case keeps, and within the value bound below.

Bound.  augment_reference's rule: an implementation that evaluates a chain with r roundings and t trigonometric factors is off by at most
(r + 2t) u S, S the sum of the magnitudes of the chain's terms, u = 2**-24; two implementations differ by twice that.
  local translation   x + off: r = 2 (the offset's own rounding to float32, the sum), t = 0 -> 4 u S with S = |x| + |off| + |x'|; an incoming
                      err passes unchanged
  local scaling       (x - c) f + c: r = 3, t = 0 -> 6 u S, taken as 8 u S with S = f |x - c| + |c| + |x'|; incoming err times f
  local rotation  x:  ((x - cx) cos - (y - cy) sin) + cx: r = 6 (two subtractions, two products, two sums), t = 2 -> 2 (6 + 4) u S = 20 u S,
                      taken as 24 u S with S = |x - cx| + |y - cy| + |cx| + |x'| (y alike); incoming err_x + err_y (the reference's matmul may
                      fuse a product into the sum: fewer roundings, inside the same bound)
                  z:  (z - cz) + cz: r = 2 -> 4 u S, taken as 8 u S with S = |z - cz| + |cz| + |z'|
  boxes               centre + offset and heading + angle: a float64 sum rounded once under value-based casting, the float32 sum of the
                      rounded draw under NumPy 2: r = 2 -> 4 u S with S = |value| + |draw| + |value'|; sizes * scale: the scale's rounding
                      and the product, r = 2 -> 4 u |value'|
Dropouts move nothing.  Per tested point the functions carry the smallest float64 gap of any comparison it met: the in-box test (with its
0.1 margin), the local thresholds (for the points inside the box) and the world threshold; the world dropout also returns the gap of every box
centre.  The in-box test is the conjunction of three comparisons, so its gap is the distance of the decision from flipping: for a point inside,
the smallest of the three slacks; for a point outside, the largest violation (all violated comparisons would have to flip, and one that holds
can only join them).  With intensity exactly 0, or one live coordinate value, the world threshold is the extreme itself on
every arithmetic path, so that comparison carries no gap.
"""
import math

import numpy as np

import augment_reference as R

f32, U, ROBUST = R.f32, R.U, R.ROBUST
LOCAL_MARGIN = 1e-1
AXES = {"x": 0, "y": 1, "z": 2}
LOCAL_NAMES = ("local_translation_x", "local_translation_y", "local_translation_z", "local_rotation", "local_scaling", "local_dropout_top",
               "local_dropout_bottom", "local_dropout_left", "local_dropout_right")
WORLD_NAMES = ("world_dropout_top", "world_dropout_bottom", "world_dropout_left", "world_dropout_right")
TRACK_MOVED = True                                               # count moved_decisions (a second in-box pass per box; tools/local_augment_micro.py turns it off)
a64 = lambda v: np.abs(np.asarray(v, np.float64))


def get_points_in_box(xyz, box):
    """:553-570.  xyz (M, 3) fp32, box (7+) fp32 -> (mask (M,) bool, gap (M,) float64, (shift_x, shift_y, shift_z))."""
    xyz = np.asarray(xyz, f32)
    cx, cy, cz, dx, dy, dz, rz = [f32(v) for v in box[:7]]
    sx, sy, sz = (xyz[:, 0] - cx).astype(f32), (xyz[:, 1] - cy).astype(f32), (xyz[:, 2] - cz).astype(f32)
    cosa, sina = f32(math.cos(-float(rz))), f32(math.sin(-float(rz)))
    lx = ((sx * cosa).astype(f32) + (sy * f32(-sina)).astype(f32)).astype(f32)
    ly = ((sx * sina).astype(f32) + (sy * cosa).astype(f32)).astype(f32)
    hz, hx, hy = f32(float(dz) / 2.0), f32(float(dx) / 2.0 + LOCAL_MARGIN), f32(float(dy) / 2.0 + LOCAL_MARGIN)
    mask = (np.abs(sz) <= hz) & (np.abs(lx) <= hx) & (np.abs(ly) <= hy)
    slack = np.stack([float(hz) - a64(sz), float(hx) - a64(lx), float(hy) - a64(ly)])           # >= 0: the comparison holds
    gap = np.where(mask, slack.min(axis=0), np.where(slack < 0, -slack, 0.0).max(axis=0))
    return mask, gap, (sx, sy, sz)


class Scene:
    """One sample's state while the restated functions run: dropped points stay in place with alive = False."""

    def __init__(self, gt_boxes, points, alive=None, err=None):
        self.boxes, self.pts = np.array(gt_boxes, f32), np.array(points, f32)
        M = len(self.pts)
        self.alive = np.ones(M, bool) if alive is None else np.array(alive, bool)
        self.err = np.zeros((M, 3)) if err is None else np.array(err, np.float64)
        self.berr = np.zeros(self.boxes.shape)
        self.gap = np.full(M, np.inf)
        self.box_gap = np.inf                                    # the world dropout's box-centre comparisons
        self.exists = np.ones(len(self.boxes), bool)
        self.moved_decisions = 0                                 # tests whose outcome differs between the point's current and original position
        self.orig = self.pts.copy()


def local_step(s, name, values):
    """One local function over all boxes in order; values: one draw per existing box, in box order."""
    assert name in LOCAL_NAMES
    if name == "local_rotation" and s.boxes.shape[1] > 8:
        raise ValueError("np.hstack of a (2,) with an (N, 1) (:465-468)")
    values = [float(v) for v in np.asarray(values, np.float64).reshape(-1)]
    assert len(values) == int(s.exists.sum())
    it = iter(values)
    for k in range(len(s.boxes)):
        if not s.exists[k]:
            continue
        v = next(it)
        box = s.boxes[k]
        idx = np.nonzero(s.alive)[0]
        mask, gap, (sx, sy, sz) = get_points_in_box(s.pts[idx, :3], box)
        s.gap[idx] = np.minimum(s.gap[idx], gap)
        if TRACK_MOVED:
            s.moved_decisions += int((mask != get_points_in_box(s.orig[idx, :3], box)[0]).sum())
        mv = idx[mask]
        cx, cy, cz, dx, dy, dz = [f32(t) for t in box[:6]]
        if name.startswith("local_translation_"):
            c = AXES[name[-1]]
            before = a64(s.pts[mv, c])
            s.pts[mv, c] = (s.pts[mv, c] + f32(v)).astype(f32)
            s.err[mv, c] += 4 * U * (before + abs(v) + a64(s.pts[mv, c]))
            new = f32(float(box[c]) + v)
            s.berr[k, c] += 4 * U * (abs(float(box[c])) + abs(v) + abs(float(new)))
            s.boxes[k, c] = new
        elif name == "local_scaling":
            sf = f32(v)
            for c, (p, ctr) in enumerate(zip((sx, sy, sz), (cx, cy, cz))):
                p = p[mask]
                new = ((p * sf).astype(f32) + ctr).astype(f32)
                s.err[mv, c] = float(sf) * s.err[mv, c] + 8 * U * (float(sf) * a64(p) + abs(float(ctr)) + a64(new))
                s.pts[mv, c] = new
            s.boxes[k, 3:6] = (s.boxes[k, 3:6] * sf).astype(f32)
            s.berr[k, 3:6] = float(sf) * s.berr[k, 3:6] + 4 * U * a64(s.boxes[k, 3:6])
        elif name == "local_rotation":
            ang = f32(v)                                         # check_numpy_to_torch(...).float()
            c_, s_ = f32(np.cos(ang)), f32(np.sin(ang))
            px, py, pz = sx[mask], sy[mask], sz[mask]
            rx, ry = R._rotate(px, py, c_, s_)
            nx, ny, nz = (rx + cx).astype(f32), (ry + cy).astype(f32), (pz + cz).astype(f32)
            carried = s.err[mv, 0] + s.err[mv, 1]
            spread = a64(px) + a64(py)
            s.err[mv, 0] = carried + 24 * U * (spread + abs(float(cx)) + a64(nx))
            s.err[mv, 1] = carried + 24 * U * (spread + abs(float(cy)) + a64(ny))
            s.err[mv, 2] += 8 * U * (a64(pz) + abs(float(cz)) + a64(nz))
            s.pts[mv, 0], s.pts[mv, 1], s.pts[mv, 2] = nx, ny, nz
            # box[0:3]: minus the centroid, rotated (zeros), plus the centroid (:447-461)
            zero = np.array([f32(cx - cx)]), np.array([f32(cy - cy)])
            bx, by = R._rotate(zero[0], zero[1], c_, s_)
            s.boxes[k, 0], s.boxes[k, 1], s.boxes[k, 2] = f32(bx[0] + cx), f32(by[0] + cy), f32(f32(cz - cz) + cz)
            new = f32(float(box[6]) + v)
            s.berr[k, 6] += 4 * U * (abs(float(box[6])) + abs(v) + abs(float(new)))
            s.boxes[k, 6] = new
        else:
            z, y = float(cz), float(cy)
            hz, hy = float(dz) / 2.0, float(dy) / 2.0
            if name == "local_dropout_top":
                thr, col, upper = f32((z + hz) - v * float(dz)), 2, True
            elif name == "local_dropout_bottom":
                thr, col, upper = f32((z - hz) + v * float(dz)), 2, False
            elif name == "local_dropout_left":
                thr, col, upper = f32((y + hy) - v * float(dy)), 1, True
            else:
                thr, col, upper = f32((y - hy) + v * float(dy)), 1, False
            coord = s.pts[mv, col]
            s.gap[mv] = np.minimum(s.gap[mv], np.abs(a64(coord) - float(thr)))
            s.alive[mv[coord >= thr if upper else coord <= thr]] = False
    return s


def world_dropout(s, name, v):
    """:323-388 on the points alive and the boxes that exist; a dropped box stops existing (here with its class)."""
    assert name in WORLD_NAMES
    v = float(v)
    idx = np.nonzero(s.alive)[0]
    if len(idx) == 0:
        return s                                                 # np.max of an empty array raises in the reference
    col = 2 if name in ("world_dropout_top", "world_dropout_bottom") else 1
    upper = name in ("world_dropout_top", "world_dropout_left")
    coord = s.pts[idx, col]
    mx, mn = f32(coord.max()), f32(coord.min())
    span = f32(mx - mn)
    thr = f32(float(mx) - v * float(span)) if upper else f32(float(mn) + v * float(span))
    keep = coord < thr if upper else coord > thr
    exact = v == 0.0 or span == 0                                # the threshold is the extreme itself on every arithmetic path
    if not exact:
        s.gap[idx] = np.minimum(s.gap[idx], np.abs(a64(coord) - float(thr)))
    s.alive[idx[~keep]] = False
    ex = np.nonzero(s.exists)[0]
    bc = s.boxes[ex, col]
    if len(ex) and not exact:
        s.box_gap = min(s.box_gap, float(np.abs(a64(bc) - float(thr)).min()))
    s.exists[ex[~(bc < thr if upper else bc > thr)]] = False
    return s


def run_ops(gt_boxes, points, ops, alive=None, exists=None):
    """ops: [(name, value)] with the names above, per-box values as arrays.  Returns the Scene."""
    s = Scene(gt_boxes, points, alive)
    if exists is not None:
        s.exists = np.array(exists, bool)
    for name, value in ops:
        if name in LOCAL_NAMES:
            local_step(s, name, value)
        else:
            world_dropout(s, name, value)
    return s


def robust_points(gt_boxes, points, ops, protect=0, **kw):
    """The points without those that come within ROBUST of a comparison they meet; at most 2 % may go, and none of the first `protect`."""
    def run(p):
        return run_ops(gt_boxes, p, ops, **kw).gap
    pts = np.array(points, f32)
    first = run(pts) < ROBUST
    assert not first[:protect].any(), "a protected point is not robust"
    out = R.robust_scene(pts, run)
    assert len(pts) - len(out) <= 0.02 * len(pts), f"robustness removed {len(pts) - len(out)} of {len(pts)} points"
    assert np.array_equal(out[:protect], pts[:protect])
    return out


# ------------------------------------------------------------------ the scene-level function
def prepare_scene(points, gt_boxes, gt_cls, draws, min_points=1, point_range=None, min_num_corners=0, num_points_in_gt=None, check=True,
                  extra_width=(0.0, 0.0, 0.0), count_boxes=False):
    """augment_reference.prepare_scene with the local / frustum names.  The local functions move every box there is, those with gt_cls == -1
    too; behind a gt_sampling that accepted something those are gone (gt_boxes[gt_boxes_mask]).  Returns what that function returns; the robust
    flag also says whether every pasted point kept ROBUST from the comparisons it met.  count_boxes: only the number of boxes the scene holds
    after `draws` (what the next per-box draw is sized by)."""
    pts, boxes, cls = np.array(points, f32), np.array(gt_boxes, f32), np.asarray(gt_cls)
    counts, gap = R.points_in_boxes_count(pts, boxes) if num_points_in_gt is None else (np.asarray(num_points_in_gt), np.full(len(pts), np.inf))
    boxes, cls = boxes[counts >= min_points], cls[counts >= min_points]
    mask = cls >= 0
    origin, err, pairs_ok = np.arange(len(pts)), np.zeros((len(pts), 3)), True
    world, berr = [], np.zeros(boxes.shape)
    cgap = np.full(len(pts), np.inf)                             # per current point, pasted ones included

    def flush():
        nonlocal boxes, pts, err, berr, world
        if world:
            boxes, pts, err, be = R.world_transform(boxes, pts, world, err)
            berr = berr + be
            world = []

    def note(g):
        gap[origin[origin >= 0]] = np.minimum(gap[origin[origin >= 0]], g[origin >= 0])

    for name, value in draws:
        if name in LOCAL_NAMES or name in WORLD_NAMES:
            flush()
            s = Scene(boxes, pts, err=err)
            s.berr = berr.copy()
            local_step(s, name, value) if name in LOCAL_NAMES else world_dropout(s, name, value)
            note(s.gap)
            pairs_ok = pairs_ok and s.box_gap >= ROBUST
            cgap = np.minimum(cgap, s.gap)[s.alive]
            pts, err, origin = s.pts[s.alive], s.err[s.alive], origin[s.alive]
            boxes, berr, cls, mask = s.boxes[s.exists], s.berr[s.exists], cls[s.exists], mask[s.exists]
        elif name == "object_scaling":
            flush()
            pts, boxes, alive, _, e2, (g, ok) = R.scale_pre_object(boxes, pts, mask, value, check=check)
            err = np.maximum(err, e2)
            note(g)
            cgap = np.minimum(cgap, g)[alive]
            pts, err, origin = pts[alive], err[alive], origin[alive]
            pairs_ok = pairs_ok and ok
        elif name == "gt_sampling":
            flush()
            groups = []
            for gid in sorted({g for g, _ in value}):
                infos = [i for g, i in value if g == gid]
                groups.append((np.stack([np.asarray(i["box3d_lidar"], f32) for i in infos]), [i["points"] for i in infos]))
            new_pts, new_boxes, accept, removed, (g, ok) = R.gt_sampling(pts, boxes, mask, groups, extra_width, check=check)
            note(g)
            cgap = np.minimum(cgap, g)
            pairs_ok = pairs_ok and ok
            if accept.any():
                n_new = len(new_pts) - int((~removed).sum())
                err = np.concatenate([np.zeros((n_new, 3)), err[~removed]])
                origin = np.concatenate([np.full(n_new, -1), origin[~removed]])
                cgap = np.concatenate([np.full(n_new, np.inf), cgap[~removed]])
                cls = np.concatenate([cls[mask], [i["class_index"] for (_, i), a in zip(value, accept) if a]])
                berr = np.concatenate([berr[mask], np.zeros((int(accept.sum()), berr.shape[1]))])
                pts, boxes, mask = new_pts, new_boxes, np.ones(len(new_boxes), bool)
        else:
            world.append((name, value))
    flush()
    if count_boxes:
        return len(boxes)
    pairs_ok = pairs_ok and bool((cgap[origin < 0] >= ROBUST).all())
    if len(boxes):
        boxes[:, 6], e = R.limit_period(boxes[:, 6])
        berr[:, 6] += e
    boxes, berr, cls = boxes[mask], berr[mask], cls[mask]
    boxes = np.concatenate([boxes, (cls + 1).astype(f32)[:, None]], axis=1)
    berr = np.concatenate([berr, np.zeros((len(berr), 1))], axis=1)
    if point_range is not None:
        m = R.mask_points_by_range(pts, point_range)
        pts, err, origin = pts[m], err[m], origin[m]
        if min_num_corners:
            m = R.mask_boxes_outside_range(boxes, point_range, min_num_corners)
            boxes, berr = boxes[m], berr[m]
    return pts, boxes, err, berr, (gap, pairs_ok), origin


# ------------------------------------------------------------------ seeded case generators
OPS_ALONE = {"local_translation_x": (-0.5, 0.5), "local_translation_y": (-0.5, 0.5), "local_translation_z": (-0.3, 0.3),
             "local_rotation": (-0.4, 0.4), "local_scaling": (0.8, 1.25), "local_dropout_top": (0.0, 0.5), "local_dropout_bottom": (0.0, 0.5),
             "local_dropout_left": (0.0, 0.5), "local_dropout_right": (0.0, 0.5), "world_dropout_top": (0.0, 0.3), "world_dropout_bottom": (0.0, 0.3),
             "world_dropout_left": (0.0, 0.3), "world_dropout_right": (0.0, 0.3)}


def replay(draw_seed, specs, n):
    """The draws the reference's functions make under np.random.seed(draw_seed) when called in the order of specs [(name, lo, hi)] on n boxes:
    one uniform(lo, hi) per box for a local function, one for a world dropout."""
    rs = np.random.RandomState(draw_seed)
    return [(name, np.array([rs.uniform(lo, hi) for _ in range(n)]) if name in LOCAL_NAMES else float(rs.uniform(lo, hi))) for name, lo, hi in specs]


def _case(boxes, pts, specs, draw_seed, **extra):
    ops = replay(draw_seed, specs, len(boxes))
    pts = robust_points(boxes, pts, ops)
    s = run_ops(boxes, pts, ops)
    assert s.box_gap >= ROBUST
    return dict(boxes=boxes, points=pts, ops=ops, specs=specs, draw_seed=draw_seed, final=s, **extra)


def case_alone(name, num_boxes, seed):
    """One op on num_boxes boxes (|heading| up to pi) with 40 points around each and 500 background points."""
    rng = np.random.RandomState(seed)
    boxes = R.make_boxes(rng, num_boxes)
    pts = R.make_points(rng, boxes, 500, 40, C=4)
    return _case(boxes, pts, [(name,) + OPS_ALONE[name]], seed + 1000)


def _pair_boxes(rng, pairs, extent=30.0):
    """`pairs` pairs of parallel boxes, the second 0.12 .. 0.18 m off the first's long side, and 80 points per pair around the gap."""
    first = R.make_boxes(rng, pairs, extent=extent, min_gap=6.0)
    boxes, strip = [], []
    for a in first:
        a = a.copy()
        a[3:6] = [4.0, 2.0, 1.6]
        gap = rng.uniform(0.12, 0.18)
        c, s = np.cos(float(a[6])), np.sin(float(a[6]))
        b = a.copy()
        b[0], b[1] = a[0] - s * (2.0 + gap), a[1] + c * (2.0 + gap)
        boxes += [a, b]
        n = 80
        lx, ly, lz = rng.uniform(-1.6, 1.6, n), rng.uniform(0.85, 1.15 + gap, n), rng.uniform(-0.5, 0.5, n)
        strip.append(np.stack([a[0] + lx * c - ly * s, a[1] + lx * s + ly * c, a[2] + lz, rng.uniform(0, 1, n)], axis=1))
    return np.array(boxes, f32), np.concatenate(strip).astype(f32)


SEQUENTIAL = {"local_translation_x": (0.25, 0.35), "local_translation_y": (0.25, 0.35), "local_translation_z": (0.85, 0.95),
              "local_rotation": (0.12, 0.18), "local_scaling": (1.15, 1.25)}


def case_sequential(name, seed):
    """Three pairs of parallel boxes 0.12 .. 0.18 m apart: with the 0.1 m margin on both sides they share a strip of points.  For at least 8
    points the later box's decision differs between the moved and the unmoved position: a kernel that tests every box against the original
    points fails here."""
    rng = np.random.RandomState(seed)
    boxes, strip = _pair_boxes(rng, 3)
    pts = np.concatenate([strip, R.make_points(rng, boxes, 200, 20, C=4)])
    case = _case(boxes, pts, [(name,) + SEQUENTIAL[name]], seed + 1000)
    assert case["final"].moved_decisions >= 8, f"{name}: only {case['final'].moved_decisions} decisions depend on the move"
    return case


def case_translation_xyz(seed):
    """random_local_translation over [x, y, z] (pointpillar_newaugs.yaml's range): three whole passes; the y pass tests against the centres the x
    pass moved, and with the original centres at least 8 points would end elsewhere."""
    rng = np.random.RandomState(seed)
    boxes = R.make_boxes(rng, 6)
    pts = R.make_points(rng, boxes, 300, 60, C=4, spread=0.9)
    case = _case(boxes, pts, [("local_translation_" + a, 0.95, 1.05) for a in "xyz"], seed + 1000)
    ops, pts = case["ops"], case["points"]
    stale = Scene(boxes, pts)
    local_step(stale, *ops[0])
    assert not np.array_equal(stale.boxes, boxes)
    stale.boxes = np.array(boxes, f32)
    local_step(stale, *ops[1])
    fresh = Scene(boxes, pts)
    local_step(fresh, *ops[0])
    local_step(fresh, *ops[1])
    case["differ"] = int((np.abs(stale.pts[:, 1] - fresh.pts[:, 1]) > 0.5).sum())
    assert case["differ"] >= 8
    return case


def case_world_all(seed):
    """All four directions in one op, each over the survivors of the last."""
    rng = np.random.RandomState(seed)
    boxes = R.make_boxes(rng, 12)
    pts = R.make_points(rng, boxes, 500, 20, C=4)
    case = _case(boxes, pts, [(n, 0.0, 0.3) for n in WORLD_NAMES], seed + 1000)
    assert 0 < case["final"].exists.sum() < 12                   # some box centres are on the dropped side
    return case


_CASES = {}


def golden_cases():
    """name -> case: what tests/golden/make_local_augment_golden.py runs the reference's own functions on (and the GPU tests reuse)."""
    if not _CASES:
        for i, name in enumerate(LOCAL_NAMES + WORLD_NAMES):
            _CASES[name] = case_alone(name, 6, 100 + i)
            _CASES[name + "_one_box"] = case_alone(name, 1, 150 + i)
        for i, name in enumerate(SEQUENTIAL):
            _CASES["seq_" + name] = case_sequential(name, 200 + i)
        _CASES["translation_xyz"] = case_translation_xyz(300)
        _CASES["world_all"] = case_world_all(310)
    return _CASES
