"""Float64 references for the rotated-box kernels (BEV overlap / IoU, 3-D IoU, NMS, points in boxes), independent of the kernels' method, and the
edge-case inputs the tests in test_boxes.py run them on.  Imports nothing from seevcn_amd; the C oracle (oracle/geometry.c) is used only to
decide, before any GPU result is looked at, where the reference algorithm itself is ill-conditioned."""
import functools

import numpy as np

from oracle import boxes as ob

EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 1e-2                 # the reference's in_box2d margin: corners this close to the other box count as inside
BAND_DELTA = 1e-4             # slack around the margin band (corner_band, and the grown side of the sandwich)

# Tolerances of test_hip_overlap_iou_iou3d, as functions of the reference value.
OVERLAP_TOL = lambda v: 2e-4 + 1e-3 * np.abs(v)
IOU_TOL = lambda v: 1e-4 + 1e-3 * np.abs(v)

# |oracle - clip_area| / (eps32 * (1 + max|centre coordinate|) * (dx_a + dy_a + dx_b + dy_b)) over every pair of family_cases() and
# shape_cases() off the corner band, the oracle built with glibc's sinf/cosf/atan2f and -ffp-contract=off: worst value measured 2.448 (family
# 'huge', whose products of 40 m extents round coarser than the sum of extents says; 0.04 ... 0.70 elsewhere).  The kernel does the same fp32
# arithmetic with the device's sinf/cosf/atan2f, which round differently, and nothing else differs: it gets 8x.
# (Measured on an MI355X: 2.03 in 'huge', 0.04 ... 0.98 elsewhere; |IoU(box, copy) - 1| <= 5.96e-7 against the oracle's 5.36e-7.)
K_ORACLE_MEASURED = 2.45
K_KERNEL = 8 * K_ORACLE_MEASURED

# Pairs that oracle_unstable flags, or that the oracle itself leaves outside the float64 sandwich, are excluded from the comparison concerned and
# count towards these caps.  Measured on family_cases() (130 pairs on each diagonal, the same for the overlap and the IoU tolerance):
#   off_tie_gaps 3 (2.3 %), identical 1, swapped_half_pi 1 (flagged, and outside the sandwich), nested_shared_corner 1 (0.8 % each), the other
#   thirteen 0; margin_tie (118 of 130 flagged, held to the sandwich only) 0 outside the sandwich.
# Over all 338 381 pairs of family_cases() and shape_cases(), off-diagonal ones included: 25 excluded (0.007 %).
CAP_FAMILY_DIAGONAL = 0.05
CAP_ALL_PAIRS = 0.02


def rand_boxes(rng, n, spread=20.0):
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-spread, spread, (n, 2))
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3] = rng.uniform(1.5, 5.0, n)
    b[:, 4] = rng.uniform(0.6, 2.5, n)
    b[:, 5] = rng.uniform(1.2, 2.0, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


# ------------------------------------------------------------------------------------------ exact intersection area
def _corners(b):
    c = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) * b[3:5]
    ca, sa = np.cos(b[6]), np.sin(b[6])
    return c @ np.array([[ca, sa], [-sa, ca]]) + b[0:2]


def _clip_area(pa, pb):
    """Sutherland-Hodgman intersection area of two convex polygons (float64) — independent of the reference's method."""
    out = [tuple(p) for p in pa]
    for i in range(len(pb)):
        a, b = pb[i], pb[(i + 1) % len(pb)]
        inp, out = out, []
        if not inp:
            break
        def side(p):
            return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        for j in range(len(inp)):
            p, q = inp[j], inp[(j + 1) % len(inp)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if sp * sq < 0:
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    if len(out) < 3:
        return 0.0
    x, y = np.array([p[0] for p in out]), np.array([p[1] for p in out])
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def _as64(boxes):
    return np.asarray(boxes, np.float32).astype(np.float64)          # the kernel's inputs are float32: that value, then float64


def _corners_batch(b, grow):
    """(P,7) float64 -> (P,4,2) counter-clockwise corners, every half-extent grown by `grow`."""
    unit = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])
    c = unit[None] * (b[:, None, 3:5] + 2.0 * grow)
    ca, sa = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    return np.stack([c[..., 0] * ca - c[..., 1] * sa + b[:, None, 0], c[..., 0] * sa + c[..., 1] * ca + b[:, None, 1]], -1)


def _clip_area_batch(pa, pb, cap=16):
    """_clip_area for P polygon pairs at once: pa, pb (P,4,2) float64."""
    n = pa.shape[0]
    rows, slots = np.arange(n)[:, None], np.arange(cap)[None, :]
    v = np.zeros((n, cap, 2))
    v[:, :4] = pa
    cnt = np.full(n, 4)
    for i in range(4):
        a, e = pb[:, i], pb[:, (i + 1) % 4] - pb[:, i]
        side = e[:, None, 0] * (v[..., 1] - a[:, None, 1]) - e[:, None, 1] * (v[..., 0] - a[:, None, 0])
        nxt = np.where(slots + 1 < cnt[:, None], slots + 1, 0)
        sq, q = side[rows, nxt], v[rows, nxt]
        live = slots < cnt[:, None]
        keep, cross = live & (side >= 0), live & (side * sq < 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(cross, side / (side - sq), 0.0)
        cand = np.empty((n, 2 * cap, 2))
        cand[:, 0::2], cand[:, 1::2] = v, v + t[..., None] * (q - v)
        flag = np.empty((n, 2 * cap), bool)
        flag[:, 0::2], flag[:, 1::2] = keep, cross
        cnt = flag.sum(1)
        assert cnt.max() <= cap
        pos = np.cumsum(flag, 1) - 1
        v = np.zeros((n, cap, 2))
        r = np.broadcast_to(rows, flag.shape)
        v[r[flag], pos[flag]] = cand[flag]
    live = slots < cnt[:, None]
    nxt = np.where(slots + 1 < cnt[:, None], slots + 1, 0)
    w = v[rows, nxt]
    area = 0.5 * np.abs(np.where(live, v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0], 0.0).sum(1))
    return np.where(cnt >= 3, area, 0.0)


def clip_area(box_a, box_b, grow=0.0):
    """Exact (float64) BEV intersection area of the float32 boxes, every half-extent grown by `grow`.  (7,) and (7,) -> float; (P,7) and (P,7) ->
    (P,) for the P pairs."""
    a, b = _as64(box_a), _as64(box_b)
    if a.ndim == 1:
        return float(clip_area(a[None], b[None], grow)[0])
    if len(a) == 0:
        return np.zeros(0)
    area = _clip_area_batch(_corners_batch(a, grow), _corners_batch(b, grow))
    flat = ((a[:, 3:5] + 2.0 * grow) <= 0).any(1) | ((b[:, 3:5] + 2.0 * grow) <= 0).any(1)     # a box without area (a clip polygon without edges cuts nothing away)
    return np.where(flat, 0.0, area)


def _all_pairs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.repeat(a, len(b), 0), np.tile(b, (len(a), 1))


def clip_area_pairs(boxes_a, boxes_b, grow=0.0):
    """clip_area of every (a, b): (na,7), (nb,7) -> (na,nb)."""
    out = np.zeros((len(boxes_a), len(boxes_b)))
    i, j = np.nonzero(~circles_apart(boxes_a, boxes_b, 0.05 + 3.0 * grow))          # the others cannot meet, grown or not
    out[i, j] = clip_area(np.asarray(boxes_a)[i], np.asarray(boxes_b)[j], grow)
    return out


# ------------------------------------------------------------------------------------------ where the reference algorithm is ill-conditioned
def _band_one_way(box, other, margin, delta):
    """any corner of `other` inside `box` grown by margin + delta but not inside `box` shrunk by delta (in box's frame, float64): (P,)"""
    c = _corners_batch(other, 0.0) - box[:, None, 0:2]
    ca, sa = np.cos(box[:, 6])[:, None], np.sin(box[:, 6])[:, None]
    lx, ly = np.abs(c[..., 0] * ca + c[..., 1] * sa), np.abs(-c[..., 0] * sa + c[..., 1] * ca)
    hx, hy = box[:, None, 3] / 2, box[:, None, 4] / 2
    grown = (lx < hx + margin + delta) & (ly < hy + margin + delta)
    shrunk = (lx < hx - delta) & (ly < hy - delta)
    return (grown & ~shrunk).any(1)


def corner_band(box_a, box_b, margin=MARGIN, delta=BAND_DELTA):
    """True when a corner of one box lies in the other's margin band, where the reference's count of inside corners (and with it the polygon it
    builds) is decided by rounding.  (7,),(7,) -> bool; (P,7),(P,7) -> (P,) bool."""
    a, b = _as64(box_a), _as64(box_b)
    if a.ndim == 1:
        return bool(corner_band(a[None], b[None], margin, delta)[0])
    return _band_one_way(a, b, margin, delta) | _band_one_way(b, a, margin, delta)


def corner_band_pairs(boxes_a, boxes_b, margin=MARGIN, delta=BAND_DELTA):
    pa, pb = _all_pairs(boxes_a, boxes_b)
    return corner_band(pa, pb, margin, delta).reshape(len(boxes_a), len(boxes_b))


def _iou_from_overlap(a, b, overlap):
    """orc_iou_bev's last line in the same float32 operations (numpy does not contract them)"""
    sa, sb = (a[:, 3] * a[:, 4])[:, None], (b[:, 3] * b[:, 4])[None]
    return overlap / np.maximum(sa + sb - overlap, np.float32(1e-8))


def oracle_nudged(boxes_a, boxes_b, iou=False):
    """The oracle's all-pairs answer and its thirteen re-evaluations (swapped; x, y, heading of either box one float32 step up and down):
    (na,nb) float32 and a list of thirteen such."""
    a, b = np.ascontiguousarray(boxes_a, np.float32), np.ascontiguousarray(boxes_b, np.float32)
    fn = ob.boxes_iou_bev if iou else ob.boxes_overlap_bev
    moved = [fn(b, a).T]
    for k in (0, 1, 6):
        for towards in (np.float32(np.inf), np.float32(-np.inf)):
            a2, b2 = a.copy(), b.copy()
            a2[:, k], b2[:, k] = np.nextafter(a[:, k], towards), np.nextafter(b[:, k], towards)
            moved += [fn(a2, b), fn(a, b2)]
    return fn(a, b), moved


def _moved_beyond(base, moved, tol):
    base = base.astype(np.float64)
    limit = tol(base)
    bad = np.zeros(base.shape, bool)
    for m in moved:
        bad |= ~(np.abs(m.astype(np.float64) - base) <= limit)
    return bad


def oracle_unstable_pairs(boxes_a, boxes_b, tol, iou=False):
    """oracle_unstable for every (a, b): (na,nb) bool, on the oracle's overlap (iou False) or IoU (iou True)."""
    return _moved_beyond(*oracle_nudged(boxes_a, boxes_b, iou), tol)


def oracle_unstable(box_a, box_b, tol, iou=False):
    """The oracle's own answer moves by more than tol(answer) under a 1-ulp change of x, y or heading of either box (np.nextafter up and down on
    elements 0, 1, 6: twelve nudges) or under swapping the boxes: the reference algorithm is ill-conditioned at this pair, and a comparison with
    another fp32 evaluation of it (other sinf/cosf/atan2f roundings) says nothing there.  Decided by the oracle alone."""
    return bool(oracle_unstable_pairs(np.asarray(box_a)[None], np.asarray(box_b)[None], tol, iou)[0, 0])


def area_unit(boxes_a, boxes_b):
    """eps32 * (1 + max|centre coordinate|) * (sum of the four BEV extents) of every pair: (na,nb).  Times K: the fp32 rounding bound."""
    a, b = _as64(boxes_a), _as64(boxes_b)
    cmax = np.maximum(np.abs(a[:, 0:2]).max(1)[:, None], np.abs(b[:, 0:2]).max(1)[None])
    return EPS32 * (1.0 + cmax) * (a[:, 3:5].sum(1)[:, None] + b[:, 3:5].sum(1)[None])


def circles_apart(boxes_a, boxes_b, gap=0.05):
    """bounding circles more than `gap` apart (float64): (na,nb) bool"""
    a, b = _as64(boxes_a), _as64(boxes_b)
    ra, rb = 0.5 * np.hypot(a[:, 3], a[:, 4]), 0.5 * np.hypot(b[:, 3], b[:, 4])
    d = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
    return d - ra[:, None] - rb[None] > gap


def iou3d_reference(boxes_a, boxes_b, overlap_bev):
    """3-D IoU from a given BEV overlap: height overlap and volumes in float64 (boxes_iou3d_gpu's arithmetic)."""
    a, b = _as64(boxes_a), _as64(boxes_b)
    ov = np.asarray(overlap_bev, np.float64)
    h = np.clip(np.minimum((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None]) -
                np.maximum((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None]), 0, None)
    o3 = ov * h
    return o3 / np.clip((a[:, 3] * a[:, 4] * a[:, 5])[:, None] + (b[:, 3] * b[:, 4] * b[:, 5])[None] - o3, 1e-6, None)


# ------------------------------------------------------------------------------------------ points in boxes
def in_box_truth(points, boxes, margin):
    """The in-box test in float64 on the float32 inputs: points (M,3), boxes (T,7) -> (first containing box or -1 (M,) int32, smallest distance
    (M,) of the point to the decision surface of any box up to and including the first containing one -- the surface of the set |z - cz| <= dz/2,
    local |x| < dx/2 + margin, local |y| < dy/2 + margin, measured per axis: how far the point would have to move along one axis for that box's
    answer to change; inf without boxes).  z: |z - cz| <= dz/2; x/y: local |x|, |y| < d/2 + margin.  `margin` is taken at
    float32, as the constant the reference adds."""
    p, b = _as64(points), _as64(boxes)
    m = float(np.float32(margin))
    idx = np.full(len(p), -1, np.int32)
    dist = np.full(len(p), np.inf)
    for k in range(len(b)):
        todo = idx < 0
        if not todo.any():
            break
        q = p[todo]
        sx, sy, sz = q[:, 0] - b[k, 0], q[:, 1] - b[k, 1], q[:, 2] - b[k, 2]
        ca, sa = np.cos(-b[k, 6]), np.sin(-b[k, 6])
        lx, ly = sx * ca - sy * sa, sx * sa + sy * ca
        gz, gx, gy = np.abs(sz) - b[k, 5] / 2, np.abs(lx) - (b[k, 3] / 2 + m), np.abs(ly) - (b[k, 4] / 2 + m)
        dist[todo] = np.minimum(dist[todo], np.abs(np.maximum(gz, np.maximum(gx, gy))))        # inside: the nearest face; outside: the test that fails by most
        inside = (gz <= 0) & (gx < 0) & (gy < 0)
        where = np.flatnonzero(todo)[inside]
        idx[where] = k
    return idx, dist


# ------------------------------------------------------------------------------------------ inputs: the families of paired boxes
GAPS_OFF_TIE = (-3e-2, -1.5e-2, -5e-3, 5e-3, 8e-3, 1.2e-2, 1.5e-2)


def _sized(rng, n, spread, lo, hi, off=0.0):
    b = rand_boxes(rng, n, spread)
    b[:, 0:2] += np.float32(off)
    b[:, 3] = rng.uniform(lo, hi, n)
    b[:, 4] = rng.uniform(lo, hi, n)
    return b


def _along_local_x(a, b_dx, gap):
    """copy of a with dx = b_dx, moved along a's local x axis so that the facing sides are `gap` apart (negative: overlapping by that much)"""
    b = a.copy()
    b[:, 3] = b_dx
    d = (a[:, 3].astype(np.float64) + b[:, 3]) / 2 + gap
    b[:, 0] = a[:, 0] + d * np.cos(a[:, 6].astype(np.float64))
    b[:, 1] = a[:, 1] + d * np.sin(a[:, 6].astype(np.float64))
    return b


def box_families(rng, n):
    """name -> (A, B): n paired float32 boxes (n,7) per family; pair i is (A[i], B[i]).  Extents are rand_boxes' unless the family says otherwise;
    centres are spread over a few metres so that the off-diagonal pairs of an all-pairs call meet as well."""
    pi = np.float32(np.pi)
    fam = {}
    seeds = iter(rng.integers(0, 2 ** 32, 32))
    fresh = lambda: np.random.default_rng(next(seeds))           # one generator per family: changing one family leaves the others' boxes alone
    rng = fresh()
    fam["random"] = (rand_boxes(rng, n, 4.0), rand_boxes(rng, n, 4.0))
    rng = fresh()
    a = rand_boxes(rng, n, 4.0)
    a[:, 0:2] += np.float32(70.0)
    b = rand_boxes(rng, n, 4.0)
    b[:, 0:2] = a[:, 0:2] + rng.uniform(-2, 2, (n, 2)).astype(np.float32)
    fam["far"] = (a, b)
    rng = fresh()
    a = rand_boxes(rng, n, 1.0)          # centres within 1 m: the reference's own IoU of a box with its copy leaves 1 by more than 1e-6 further out
    fam["identical"] = (a, a.copy())
    rng = fresh()
    a = rand_boxes(rng, n, 4.0)
    b = a.copy()
    b[:, 6] += pi * rng.integers(-3, 4, n).astype(np.float32)
    fam["identical_kpi"] = (a, b)
    b = a.copy()
    b[:, [3, 4]] = a[:, [4, 3]]
    b[:, 6] += pi / 2
    fam["swapped_half_pi"] = (a, b)
    b = a.copy()
    b[:, 6] += (10.0 ** rng.uniform(-7, np.log10(3e-2), n) * rng.choice([-1, 1], n)).astype(np.float32)
    fam["tiny_rotation"] = (a, b)
    b = a.copy()
    b[:, 0:2] += (10.0 ** rng.uniform(-6, -1, (n, 2)) * rng.choice([-1, 1], (n, 2))).astype(np.float32)
    fam["tiny_shift"] = (a, b)
    rng = fresh()
    a = rand_boxes(rng, n, 4.0)
    fam["touching"] = (a, _along_local_x(a, rng.uniform(1.5, 5.0, n).astype(np.float32), 0.0))
    fam["off_tie_gaps"] = (a, _along_local_x(a, a[:, 3], rng.choice(GAPS_OFF_TIE, n)))
    fam["margin_tie"] = (a, _along_local_x(a, a[:, 3], MARGIN))
    b = a.copy()                                                     # nested, concentric: B's bounding circle inside A, any heading
    scale = rng.uniform(0.2, 0.9, n) * np.minimum(a[:, 3], a[:, 4]) / np.hypot(a[:, 3], a[:, 4])
    b[:, 3:5] = a[:, 3:5] * scale[:, None].astype(np.float32)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    fam["nested_concentric"] = (a, b)
    b = a.copy()                                                     # nested, same heading, one corner shared
    s = rng.uniform(0.2, 0.8, n).astype(np.float32)
    b[:, 3], b[:, 4] = a[:, 3] * s, a[:, 4] * s
    lx = (a[:, 3].astype(np.float64) - b[:, 3]) / 2 * rng.choice([-1, 1], n)
    ly = (a[:, 4].astype(np.float64) - b[:, 4]) / 2 * rng.choice([-1, 1], n)
    ca, sa = np.cos(a[:, 6].astype(np.float64)), np.sin(a[:, 6].astype(np.float64))
    b[:, 0], b[:, 1] = a[:, 0] + lx * ca - ly * sa, a[:, 1] + lx * sa + ly * ca
    fam["nested_shared_corner"] = (a, b)
    rng = fresh()
    a, b = rand_boxes(rng, n, 4.0), rand_boxes(rng, n, 4.0)
    quarter = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi], np.float32)
    a[:, 6], b[:, 6] = rng.choice(quarter, n), rng.choice(quarter, n)
    fam["axis_aligned"] = (a, b)
    rng = fresh()
    fam["tiny"] = (_sized(rng, n, 0.3, 0.03, 0.3), _sized(rng, n, 0.3, 0.03, 0.3))
    rng = fresh()
    fam["huge"] = (_sized(rng, n, 20.0, 10.0, 40.0), _sized(rng, n, 20.0, 10.0, 40.0))
    rng = fresh()
    b = rand_boxes(rng, n, 4.0)
    a = _sized(rng, n, 4.0, 0.05, 0.2)
    a[:, 0:2] = b[:, 0:2] + rng.uniform(-2.5, 2.5, (n, 2)).astype(np.float32)
    fam["mixed"] = (a, b)
    rng = fresh()
    a = rand_boxes(rng, n, 3.0)                                      # slivers: against slivers crossing at the centre, and against car-sized boxes nearby
    a[:, 4] = 0.02
    b = a.copy()
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    b[n // 2:] = rand_boxes(rng, n - n // 2, 3.0)
    b[n // 2:, 0:2] = a[n // 2:, 0:2] + rng.uniform(-2, 2, (n - n // 2, 2)).astype(np.float32)
    fam["sliver"] = (a, b)
    rng = fresh()
    a, b = rand_boxes(rng, n, 4.0), rand_boxes(rng, n, 4.0)          # zero padding rows against real boxes and against each other
    a[::2] = 0
    b[::3] = 0
    fam["zero_padding"] = (a, b)
    return fam


def set_heights(a, b):
    """z and dz of box i of either set by i % 4, so that pair (i, i) has: equal heights; touching in z (height overlap exactly 0: every sum is
    exact in float32); B inside A in z; dz = 0 for B, and for both every other time.  Returns copies."""
    a, b = a.copy(), b.copy()
    for boxes, z, dz in ((a, (0.25, -0.5, 0.25, 0.25), (1.5, 1.5, 3.0, 1.5)), (b, (0.25, 1.0, 0.0, 0.25), (1.5, 1.5, 1.0, 0.0))):
        m = np.arange(len(boxes)) % 4
        boxes[:, 2], boxes[:, 5] = np.array(z, np.float32)[m], np.array(dz, np.float32)[m]
    a[7::8, 5] = 0.0
    return a, b


FAMILY_N = 130
SHAPES = ((1, 1), (3, 63), (4, 64), (5, 65), (257, 130))       # the edges of the kernels' 4 x 64 tile


class Case:
    """One all-pairs call and everything the tests hold its result to (computed once, on the CPU, without looking at any GPU result)."""

    def __init__(self, name, a, b, paired):
        self.name, self.a, self.b, self.paired = name, a, b, paired
        self.overlap, moved = oracle_nudged(a, b)
        self.iou = ob.boxes_iou_bev(a, b)
        self.unstable_overlap = _moved_beyond(self.overlap, moved, OVERLAP_TOL)
        self.unstable_iou = _moved_beyond(self.iou, [_iou_from_overlap(a, b, m) for m in moved], IOU_TOL)     # same bits as orc_iou_bev of the nudged pair
        self.exact = clip_area_pairs(a, b)
        self.grown = clip_area_pairs(a, b, MARGIN + BAND_DELTA)
        self.band = corner_band_pairs(a, b)
        self.unit = area_unit(a, b)
        self.apart = circles_apart(a, b)
        zero_a, zero_b = ~a.any(1), ~b.any(1)
        self.padding = zero_a[:, None] | zero_b[None]
        self.area_a, self.area_b = (a[:, 3] * a[:, 4]).astype(np.float64)[:, None], (b[:, 3] * b[:, 4]).astype(np.float64)[None]

    def worst_ratio(self, overlap):
        """largest |overlap - exact| / unit off the corner band (0 without such pairs)"""
        sel = ~self.band & (self.unit > 0)
        return float((np.abs(np.asarray(overlap, np.float64) - self.exact)[sel] / self.unit[sel]).max()) if sel.any() else 0.0

    def sandwich_misses(self, overlap, k):
        """pairs whose overlap lies outside [exact - s, grown + s] (inside the band) or further than s from exact (off it), s = k * unit"""
        s = k * self.unit
        got = np.asarray(overlap, np.float64)
        return np.where(self.band, (got < self.exact - s) | (got > self.grown + s), np.abs(got - self.exact) > s)


@functools.lru_cache(maxsize=None)
def family_cases(n=FAMILY_N, seed=20):
    return tuple(Case(name, a, b, True) for name, (a, b) in box_families(np.random.default_rng(seed), n).items())


@functools.lru_cache(maxsize=None)
def shape_cases(seed=21):
    """(na, nb) calls at the tile edges, rows drawn from every family."""
    rng = np.random.default_rng(seed)
    fam = box_families(rng, 24)
    pool_a = np.concatenate([a for a, _ in fam.values()])
    pool_b = np.concatenate([b for _, b in fam.values()])
    pool_a, pool_b = pool_a[rng.permutation(len(pool_a))], pool_b[rng.permutation(len(pool_b))]
    pool_a[0] = rand_boxes(rng, 1, 4.0)[0]                           # the 1 x 1 call is a pair that meets
    pool_b[0] = pool_a[0] + np.array([0.5, -0.25, 0, 0.5, 0.25, 0, 0.3], np.float32)
    return tuple(Case("shape_%dx%d" % (na, nb), pool_a[:na].copy(), pool_b[:nb].copy(), False) for na, nb in SHAPES)


# ------------------------------------------------------------------------------------------ inputs: NMS with closed-form answers
FIRST_MEMBERS = (0, 63, 64, 65, 1023, 1024, 1025, 3071, 3072)


def nms_clusters(n, seed=0):
    """n boxes in score order: position p in FIRST_MEMBERS (and n - 1) opens a cluster 100 m from every other, any other position is an exact
    copy of an earlier first member (IoU 1 inside a cluster, 0 across by the circle test) -- the last 64 positions copy cluster 0, so a
    keeper of block 0 suppresses in the last block.  Returns (boxes (n,7) in score order, keepers: sorted positions of the first members)."""
    rng = np.random.default_rng(1000 + n + seed)
    first = sorted({p for p in FIRST_MEMBERS + (n - 1,) if 0 <= p < n})
    boxes = np.zeros((n, 7), np.float32)
    opened = []
    for p in range(n):
        if p in first:
            boxes[p] = rand_boxes(rng, 1, 0.0)[0]
            boxes[p, 0], boxes[p, 1] = 100.0 * (len(opened) % 4), 100.0 * (len(opened) // 4)
            opened.append(p)
        else:
            boxes[p] = boxes[opened[0] if p >= n - 64 else opened[p % len(opened)]]
    return boxes, np.array(first, np.int64)


def nms_chain(n):
    """Axis-aligned unit squares at x = 0.5 i in score order: neighbours have IoU 1/3, next-but-one only touch (overlap exactly 0: every
    coordinate is exact in float32).  With threshold 0.2 the keepers are the even positions."""
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, 0] = 0.5 * np.arange(n)
    boxes[:, 3:6] = 1.0
    return boxes, np.arange(0, n, 2, dtype=np.int64)


def nms_max_keeps(keepers, n):
    """None, 1, the keepers in the first chunk of a chunked sweep (sorted positions below 1024) and one more, those through the second chunk
    (below 3072) and one more, all, all + 10"""
    c1, c2, k = int((keepers < 1024).sum()), int((keepers < 3072).sum()), len(keepers)
    out = [None]
    for v in (1, c1, c1 + 1, c2, c2 + 1, k, k + 10):
        if v not in out:
            out.append(v)
    return out


# ------------------------------------------------------------------------------------------ inputs: points in boxes
# Heading-0 boxes whose numbers are short binary fractions and whose centres are far larger than their extents: for every point placed below, the
# float32 differences x - cx, y - cy, z - cz to the box it is placed at are exact (checked by exact_or_far), the rotation by cos = 1, sin = 0 is exact, so the kernel's
# float32 arithmetic and in_box_truth decide the same real numbers and must agree bit for bit.
EXACT_BOXES = np.array([[8.0, -16.0, 4.0, 3.0, 1.5, 2.0, 0.0],
                        [-32.0, 8.0, -8.0, 5.0, 2.5, 1.5, 0.0],
                        [16.0, 16.0, 4.0, 1.5, 0.75, 1.25, 0.0],
                        [-8.0, -32.0, 8.0, 4.0, 2.0, 3.0, 0.0]], np.float32)


def _around(t):
    """the float32 numbers next to the real threshold t: one step below, nearest, one step above"""
    f = np.float32(t)
    return [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]


def exact_face_points(margin, boxes=EXACT_BOXES):
    """Points on and next to every decision surface of heading-0 boxes: x (then y) at c +- d/2 and one float32 step either side of
    c +- (d/2 + margin), each with z at cz, at cz +- dz/2 (inside) and one step beyond (outside)."""
    m = float(np.float32(margin))
    pts = []
    for b in boxes.astype(np.float64):
        zs = [b[2]]
        for sgn in (-1.0, 1.0):
            z = np.float32(b[2] + sgn * b[5] / 2)
            zs += [z, np.nextafter(z, np.float32(sgn * np.inf))]
        for axis in (0, 1):
            us = []
            for sgn in (-1.0, 1.0):
                us += [np.float32(b[axis] + sgn * b[3 + axis] / 2)] + _around(b[axis] + sgn * (b[3 + axis] / 2 + m))
            for u in us:
                for z in zs:
                    p = [b[0], b[1], z]
                    p[axis] = u
                    pts.append(p)
    return np.array(pts, np.float32)


def exact_or_far(points, boxes, margin):
    """(M,) bool: for every box, either the box has heading 0 and the float32 differences point - centre equal the real differences (float32 and
    float64 then test the same numbers), or the point is further than decision_delta from each of that box's decision surfaces."""
    p32, b32 = np.asarray(points, np.float32), np.asarray(boxes, np.float32)
    delta = decision_delta(p32, b32)
    ok = np.ones(len(p32), bool)
    for k in range(len(b32)):
        exact = ((p32 - b32[k, 0:3]).astype(np.float64) == p32.astype(np.float64) - b32[k, 0:3].astype(np.float64)).all(1) & (b32[k, 6] == 0)
        ok &= exact | (in_box_truth(p32, b32[k:k + 1], margin)[1] > delta)
    return ok


FIRST_BOX_SCENES = {
    # nested boxes, both index orders; duplicates; zero padding rows in front of real boxes.  Heading 0 and short binary fractions throughout.
    "outer_first": np.array([[8, 8, 0, 4, 4, 2, 0], [8, 8, 0, 2, 2, 1, 0], [8, 8, 0, 1, 1, 0.5, 0]], np.float32),
    "inner_first": np.array([[8, 8, 0, 1, 1, 0.5, 0], [8, 8, 0, 2, 2, 1, 0], [8, 8, 0, 4, 4, 2, 0]], np.float32),
    "duplicates": np.array([[8, 8, 0, 2, 2, 1, 0]] * 4 + [[0, 0, 0, 4, 4, 2, 0]] * 3, np.float32),
    "padding_first": np.array([[0, 0, 0, 0, 0, 0, 0]] * 3 + [[0, 0, 0, 4, 4, 2, 0], [8, 8, 0, 2, 2, 1, 0]], np.float32),
}


def first_box_points(margin):
    """Points for FIRST_BOX_SCENES: the origin exactly (inside an all-zero row: 0 <= 0 in z, 0 < margin in x and y), points exactly `margin`
    from it (outside: the test is strict), points inside one, two and three of the nested boxes."""
    m = np.float32(margin)
    return np.array([[0, 0, 0], [m, 0, 0], [0, m, 0], [-m, 0, 0], [np.nextafter(m, np.float32(0)), 0, 0], [0, 0, np.float32(1e-30)],
                     [8, 8, 0], [8.25, 7.75, 0.25], [8.75, 8, 0], [8, 8, 0.5], [9.5, 9.5, 0.75], [9.5, 8, -1], [8, 8, 1.25], [1, 1, 0.5], [12, 12, 0]],
                    np.float32)


SPECIAL_HEADINGS = (np.pi / 2, -np.pi / 2, np.pi, -np.pi, 7.5 * np.pi)


def decision_delta(points, boxes):
    """64 * eps32 * (1 + max|coordinate|): float32 evaluations of the in-box test may disagree with float64 only this close to a decision surface"""
    return 64.0 * EPS32 * (1.0 + max(np.abs(np.asarray(points)).max(initial=0.0), np.abs(np.asarray(boxes)[..., 0:6]).max(initial=0.0)))


def general_scene(rng, num_boxes, num_points, margin, spread=10.0):
    """One scene of boxes with any heading (the first ones SPECIAL_HEADINGS) and points: half uniform over the scene, half next to a face of a
    random box -- at a distance from it drawn uniformly from 2 * decision_delta ... 1e-3, either side: closer, float32 cannot decide, and the
    point would only count against the 1 % cap."""
    boxes = rand_boxes(rng, num_boxes, spread)
    boxes[:len(SPECIAL_HEADINGS), 6] = SPECIAL_HEADINGS[:num_boxes]
    pts = rng.uniform(-spread - 2, spread + 2, (num_points, 3))
    pts[:, 2] *= 0.15
    delta = 64.0 * EPS32 * (1.0 + spread + 6.0)
    for i in range(num_points // 2):
        b = boxes[rng.integers(num_boxes)].astype(np.float64)
        half = np.array([b[3] / 2 + float(np.float32(margin)), b[4] / 2 + float(np.float32(margin)), b[5] / 2])
        local = rng.uniform(-0.95, 0.95, 3) * half
        axis = rng.integers(3)
        local[axis] = rng.choice([-1, 1]) * (half[axis] + rng.choice([-1, 1]) * rng.uniform(2 * delta, 1e-3))
        ca, sa = np.cos(b[6]), np.sin(b[6])
        pts[i] = [b[0] + local[0] * ca - local[1] * sa, b[1] + local[0] * sa + local[1] * ca, b[2] + local[2]]
    return pts.astype(np.float32), boxes


def grid_scene(rng, num_boxes, num_points, pitch=8.0):
    """num_boxes boxes on a square grid `pitch` apart (none touches another) and points well inside randomly chosen ones -- the last box always
    among them -- or between the boxes."""
    side = int(np.ceil(np.sqrt(max(num_boxes, 1))))
    boxes = rand_boxes(rng, num_boxes, 0.0)
    k = rng.permutation(num_boxes)
    boxes[:, 0], boxes[:, 1] = pitch * (k % side), pitch * (k // side)
    pts = np.zeros((num_points, 3))
    for i in range(num_points):
        if num_boxes == 0 or i % 4 == 3:
            pts[i] = [rng.uniform(0, pitch * side), rng.uniform(0, pitch * side), rng.uniform(-3, 3)]
            continue
        b = boxes[num_boxes - 1 if i % 4 == 0 else rng.integers(num_boxes)].astype(np.float64)
        local = rng.uniform(-0.8, 0.8, 3) * b[3:6] / 2
        ca, sa = np.cos(b[6]), np.sin(b[6])
        pts[i] = [b[0] + local[0] * ca - local[1] * sa, b[1] + local[0] * sa + local[1] * ca, b[2] + local[2]]
    return pts.astype(np.float32), boxes
