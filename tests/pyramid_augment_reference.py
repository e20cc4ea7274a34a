"""numpy restatement of the reference's pyramid augmentor, random_local_pyramid_aug (data_augmentor.py:221-242; augmentor_utils.py:573-762:
get_pyramids, points_in_pyramids_mask, local_pyramid_dropout, local_pyramid_sparsify, local_pyramid_swap), with an explicit RandomState in place
of np.random, and the seeded cases both test files use.  tests/test_pyramid_augment_reference.py holds it to the reference's own functions
(tests/golden/pyramid_augment.npz); tests/test_pyramid_augment.py holds the device to it.

Pyramids.  boxes_to_corners_3d in float32, one rounding per operation: template * size, the matmul row x c + y (-s), + centre.  The reference
takes cos / sin from torch's float32 kernels, which are faithful, not correctly rounded (of 20 000 headings drawn uniformly, 963 cosines differ
from the correctly rounded value on the machine the golden was made on, and the corners then differ by an ulp); the restatement and the device
take the float64 function rounded once, which is the same number everywhere.  Parity with the reference's bits is therefore stated for headings
whose cosine and sine both lie within HEADING_ULP of a float32 value, where every faithful implementation returns that value: the generator
draws such headings (robust_heading), in the ranges a case asks for.

Membership.  in_hull(p, 5 vertices) = Delaunay.find_simplex(p) >= 0: the closed convex hull.  Here: the float32 point and vertices widened to
float64, n = (p1 - p0) x (p2 - p0) per face plane, the sign of n . (p - p0) against that of the opposite vertex, closed (member()).  The base
is planar in float32 too (a face's corners share two x, y pairs or one z).  The float64 products round at 2^-53 relative: at 70 m and 5 m boxes
|n . (p - p0)| carries an error below 1e-12 m times |n|, so a point whose distance from every face plane is at least BAND = 1e-6 m is decided the
same way by any evaluation order and by qhull; the generator rejects the others and asserts that they are at most MAX_DISCARD of its draws (for
points uniform in a 1.5 m box the band's share is about 1e-5).

Swap arithmetic.  get_points_ratio / recover_points_by_ratio and the rescaling of the last column are float32 array operations in the reference:
one rounding per operation, sums of three left to right (numpy's add.reduce over three elements), np.clip(max - min, 1e-6, 1) in float32.  The
device is built with contraction off and IEEE division, so swapped rows are expected bit-equal and the tests ask for that.

Streams.  Legacy np.random order per scene: randint(0, 6, n), uniform(0, 1, n); if m > 0 boxes are left randint(0, 6, m), uniform(0, 1, m), then
per valid selected pyramid in box order choice(count, size=MAX, replace=False); uniform(0, 1, k) over the k boxes left; per selected box with a
valid face choice(its valid faces); per chosen pair choice(boxes whose face is still valid) where there is one.  Every call with size 0 draws
nothing, so the restatement (and the device's host side) makes them unconditionally.
"""
import numpy as np

f32 = np.float32
BAND = 1e-6
MAX_DISCARD = 1e-3
HEADING_ULP = 0.05
ORDERS = np.array([[0, 1, 5, 4], [4, 5, 6, 7], [7, 6, 2, 3], [3, 2, 1, 0], [1, 2, 6, 5], [0, 4, 7, 3]])
DRAW_NAMES = ("pyramid_drop_face", "pyramid_drop_u", "pyramid_sparsify_face", "pyramid_sparsify_u", "pyramid_sparsify_choice", "pyramid_swap_u",
              "pyramid_swap_face", "pyramid_swap_partner")


# ------------------------------------------------------------------ pyramids (box_utils.py:28-53, augmentor_utils.py:573-595)
def boxes_to_corners_3d(boxes):
    b = np.asarray(boxes, f32)
    t = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]], f32) / f32(2)
    loc = b[:, None, 3:6] * t[None]
    c, s = np.cos(b[:, 6].astype(np.float64)).astype(f32)[:, None], np.sin(b[:, 6].astype(np.float64)).astype(f32)[:, None]
    x = loc[:, :, 0] * c + loc[:, :, 1] * (-s)
    y = loc[:, :, 0] * s + loc[:, :, 1] * c
    return np.stack([x, y, loc[:, :, 2]], axis=2) + b[:, None, 0:3]


def get_pyramids(boxes):
    """(N, 6, 15) float32: apex (the centre), then the face's four corners."""
    b = np.asarray(boxes, f32).reshape(-1, 7)
    corners = boxes_to_corners_3d(b)
    out = np.zeros((len(b), 6, 15), f32)
    for f, order in enumerate(ORDERS):
        out[:, f, 0:3] = b[:, 0:3]
        for i, m in enumerate(order):
            out[:, f, 3 + 3 * i:6 + 3 * i] = corners[:, m]
    return out


# ------------------------------------------------------------------ membership (box_utils.py:12-25, augmentor_utils.py:606-611)
def _planes(pyramid):
    """The five face planes of one pyramid (5, 3) as (p0, p1, p2, opposite vertex), float64: the base, then the four sides."""
    v = np.asarray(pyramid, np.float64).reshape(5, 3)
    a, q = v[0], v[1:]
    return [(q[0], q[1], q[2], a)] + [(a, q[i], q[(i + 1) & 3], q[(i + 2) & 3]) for i in range(4)]


def _side(points, plane):
    p0, p1, p2, opp = plane
    a, b = p1 - p0, p2 - p0
    n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    d = points - p0
    so = (n[0] * (opp[0] - p0[0]) + n[1] * (opp[1] - p0[1])) + n[2] * (opp[2] - p0[2])
    sp = (n[0] * d[:, 0] + n[1] * d[:, 1]) + n[2] * d[:, 2]
    return so, sp, n


def member(points, pyramid):
    """(n,) bool: the float32 points inside the closed pyramid, by the signs of the five float64 plane sides."""
    p = np.asarray(points, f32)[:, 0:3].astype(np.float64)
    inside = np.ones(len(p), bool)
    for plane in _planes(pyramid):
        so, sp, _ = _side(p, plane)
        inside &= (sp >= 0.0) if so >= 0.0 else (sp <= 0.0)
    return inside


def plane_distances(points, pyramid):
    """(n, 5) float64: the signed distance in metres from each face plane, positive inside; what BAND is measured in."""
    p = np.asarray(points, f32)[:, 0:3].astype(np.float64)
    out = np.zeros((len(p), 5))
    for i, plane in enumerate(_planes(pyramid)):
        so, sp, n = _side(p, plane)
        out[:, i] = sp / np.linalg.norm(n) * (1.0 if so >= 0.0 else -1.0)
    return out


def points_in_pyramids_mask(points, pyramids):
    pyramids = np.asarray(pyramids, f32).reshape(-1, 5, 3)
    flags = np.zeros((len(points), len(pyramids)), bool)
    for i, pyramid in enumerate(pyramids):
        flags[:, i] = member(points, pyramid)
    return flags


# ------------------------------------------------------------------ the three functions (augmentor_utils.py:614-762)
def _log(log, name, value):
    if log is not None:
        log.append((name, value))


def local_pyramid_dropout(gt_boxes, points, dropout_prob, rng, pyramids=None, log=None):
    if pyramids is None:
        pyramids = get_pyramids(gt_boxes).reshape([-1, 6, 5, 3])
    n = pyramids.shape[0]
    face = rng.randint(0, 6, n)
    u = rng.uniform(0, 1, n)
    drop = u <= dropout_prob
    if drop.sum() != 0:
        masks = points_in_pyramids_mask(points, pyramids[drop, face[drop]])
        points = points[~masks.any(-1)]
    _log(log, "pyramid_drop_face", face)
    _log(log, "pyramid_drop_u", u)
    return gt_boxes, points, pyramids[~drop]


def local_pyramid_sparsify(gt_boxes, points, prob, max_num_pts, rng, pyramids=None, log=None):
    if pyramids is None:
        pyramids = get_pyramids(gt_boxes).reshape([-1, 6, 5, 3])
    m = pyramids.shape[0]
    face = rng.randint(0, 6, m)                                  # (size 0 draws nothing: the reference's `if pyramids.shape[0] > 0`)
    u = rng.uniform(0, 1, m)
    sel = u <= prob
    choices = []
    if m > 0:
        sampled = pyramids[sel, face[sel]]
        masks = points_in_pyramids_mask(points, sampled)
        valid = masks.sum(0) > max_num_pts
        if valid.sum() > 0:
            pm = masks[:, valid]
            parts = [points[~pm.any(-1)]]
            for i in range(pm.shape[1]):
                sample = points[pm[:, i]]
                idx = rng.choice(sample.shape[0], size=max_num_pts, replace=False)
                choices.append(np.asarray(idx, np.int64))
                parts.append(sample[idx])
            points = np.concatenate(parts, axis=0)
        pyramids = pyramids[~sel]
    _log(log, "pyramid_sparsify_face", face)
    _log(log, "pyramid_sparsify_u", u)
    _log(log, "pyramid_sparsify_choice", choices)
    return gt_boxes, points, pyramids


def get_points_ratio(points, pyramid):
    """float32, one rounding per operation (augmentor_utils.py:665-671); pyramid (15,)."""
    points, pyramid = np.asarray(points, f32), np.asarray(pyramid, f32)
    centre = (pyramid[3:6] + pyramid[6:9] + pyramid[9:12] + pyramid[12:]) / f32(4.0)
    v0, v1, v2 = pyramid[6:9] - pyramid[3:6], pyramid[12:] - pyramid[3:6], pyramid[0:3] - centre
    alphas = ((points[:, 0:3] - pyramid[3:6]) * v0).sum(-1) / (v0 * v0).sum()
    betas = ((points[:, 0:3] - pyramid[3:6]) * v1).sum(-1) / (v1 * v1).sum()
    gammas = ((points[:, 0:3] - centre) * v2).sum(-1) / (v2 * v2).sum()
    assert alphas.dtype == betas.dtype == gammas.dtype == f32
    return [alphas, betas, gammas]


def recover_points_by_ratio(ratio, pyramid):
    alphas, betas, gammas = ratio
    pyramid = np.asarray(pyramid, f32)
    centre = (pyramid[3:6] + pyramid[6:9] + pyramid[9:12] + pyramid[12:]) / f32(4.0)
    v0, v1, v2 = pyramid[6:9] - pyramid[3:6], pyramid[12:] - pyramid[3:6], pyramid[0:3] - centre
    out = (alphas[:, None] * v0 + betas[:, None] * v1) + pyramid[3:6] + gammas[:, None] * v2
    assert out.dtype == f32
    return out


def _intensity_ratio(col):
    lo, hi = col.min(), col.max()
    span = np.minimum(np.maximum(hi - lo, f32(1e-6)), f32(1))    # np.clip(max - min, 1e-6, 1), float32
    return (col - lo) / span


def local_pyramid_swap(gt_boxes, points, prob, max_num_pts, rng, pyramids=None, log=None):
    if pyramids is None:
        pyramids = get_pyramids(gt_boxes).reshape([-1, 6, 5, 3])
    k = pyramids.shape[0]
    u = rng.uniform(0, 1, k)
    sel = u <= prob
    faces, partners = np.zeros(0, np.int64), np.zeros(0, np.int64)
    boxes_chosen = np.zeros(0, np.int64)
    if sel.sum() > 0:
        masks = points_in_pyramids_mask(points, pyramids)
        valid = masks.sum(0).reshape(k, 6) > max_num_pts
        selected = valid & sel[:, None]
        if selected.sum() > 0:
            ii, jj = np.nonzero(selected)
            pick = [rng.choice(jj[ii == i]) if e and (ii == i).any() else 0 for i, e in enumerate(sel)]
            chosen = selected & (np.arange(6)[None, :] == np.asarray(pick)[:, None])
            ci, cj = np.nonzero(chosen)
            valid[chosen] = False
            part = np.array([rng.choice(np.where(valid[:, j])[0]) if valid[:, j].any() else ci[t] for t, j in enumerate(cj.tolist())])
            boxes_chosen, faces, partners = ci, cj, part
            if points.shape[1] != 4:
                raise ValueError(f"local_pyramid_swap re-assembles x y z and the last column: {points.shape[1]} columns cannot be concatenated "
                                 "(np.concatenate raises in the reference)")
            involved = np.zeros(len(points), bool)
            res = []
            for t in range(len(ci)):
                ma, mb = masks[:, ci[t] * 6 + cj[t]], masks[:, part[t] * 6 + cj[t]]
                involved |= ma | mb
                pa, pb = pyramids[ci[t], cj[t]].reshape(15), pyramids[part[t], cj[t]].reshape(15)
                a, b = points[ma], points[mb]
                ia, ib = _intensity_ratio(a[:, -1:]), _intensity_ratio(b[:, -1:])
                ra, rb = get_points_ratio(a, pa), get_points_ratio(b, pb)
                new_a = recover_points_by_ratio(rb, pa)
                new_b = recover_points_by_ratio(ra, pb)
                new_ai = ib * (a[:, -1:].max() - a[:, -1:].min()) + a[:, -1:].min()
                new_bi = ia * (b[:, -1:].max() - b[:, -1:].min()) + b[:, -1:].min()
                res.append(np.concatenate([new_a, new_ai], axis=1))
                res.append(np.concatenate([new_b, new_bi], axis=1))
            points = np.concatenate([points[~involved]] + res, axis=0)
            assert points.dtype == f32
    _log(log, "pyramid_swap_u", u)
    _log(log, "pyramid_swap_face", np.asarray(faces, np.int64))
    _log(log, "pyramid_swap_partner", np.asarray(partners, np.int64))
    return gt_boxes, points


def random_local_pyramid_aug(gt_boxes, points, cfg, rng):
    """data_augmentor.py:221-242 on one scene.  Returns (points, draws): draws as the device's out["draws"] lists them."""
    log = []
    gt_boxes = np.asarray(gt_boxes, f32).reshape(-1, 7)
    _, points, pyr = local_pyramid_dropout(gt_boxes, points, cfg["DROP_PROB"], rng, log=log)
    _, points, pyr = local_pyramid_sparsify(gt_boxes, points, cfg["SPARSIFY_PROB"], cfg["SPARSIFY_MAX_NUM"], rng, pyr, log=log)
    _, points = local_pyramid_swap(gt_boxes, points, cfg["SWAP_PROB"], cfg["SWAP_MAX_NUM"], rng, pyr, log=log)
    assert tuple(n for n, _ in log) == DRAW_NAMES
    return points, log


def run_case(case):
    """A case as the entry sees it: the box rows that exist (cls != -2) and the points that are alive.  Returns (points, draws, rng)."""
    rng = np.random.RandomState(case["seed"])
    boxes = case["boxes"][case["cls"] != -2][:, :7]
    points, draws = random_local_pyramid_aug(boxes, case["points"][~case["dead"]], case["cfg"], rng)
    return points, draws, rng


# ------------------------------------------------------------------ the cases
def _near_f32(v):
    r = np.float64(f32(v))
    return abs(v - r) <= HEADING_ULP * float(np.spacing(f32(abs(r))))


def robust_heading(rs, lo, hi):
    """A float32 heading in [lo, hi] whose float64 cos and sin both lie within HEADING_ULP ulps of a float32 value (module docstring)."""
    while True:
        h = f32(rs.uniform(lo, hi))
        if _near_f32(np.cos(np.float64(h))) and _near_f32(np.sin(np.float64(h))):
            return h


def make_box(rs, centre, size, heading):
    return np.array([centre[0], centre[1], centre[2], size[0], size[1], size[2], robust_heading(rs, heading[0], heading[1])], f32)


class _Tally:
    drawn = 0
    discarded = 0


TALLY = _Tally()


def _in_band(points, pyramids):
    """(n,) bool: closer than BAND to a face plane of any pyramid."""
    bad = np.zeros(len(points), bool)
    for pyramid in np.asarray(pyramids, f32).reshape(-1, 5, 3):
        bad |= (np.abs(plane_distances(points, pyramid)) < BAND).any(axis=1)
    return bad


def _accept(rs, draw, n, pyramids):
    """n float32 points from draw(count) with those inside the band of any pyramid drawn again; every draw and discard is tallied."""
    out = np.zeros((0, 3), f32)
    while len(out) < n:
        cand = draw(n - len(out)).astype(f32)
        bad = _in_band(cand, pyramids) if len(pyramids) else np.zeros(len(cand), bool)
        TALLY.drawn += len(cand)
        TALLY.discarded += int(bad.sum())
        out = np.concatenate([out, cand[~bad]])
    return out


def _inside_pyramid(rs, pyramid, n):
    """Points well inside one pyramid: apex + t (base point - apex)."""
    v = np.asarray(pyramid, np.float64).reshape(5, 3)
    a, b, t = rs.uniform(0.03, 0.97, (n, 1)), rs.uniform(0.03, 0.97, (n, 1)), rs.uniform(0.1, 0.97, (n, 1))
    base = v[1] + a * (v[2] - v[1]) + b * (v[4] - v[1])
    return v[0] + t * (base - v[0])


def _inside_box(rs, box, n):
    """Points uniform in a box (float64 arithmetic; which pyramid holds them is the membership test's business)."""
    b = np.asarray(box, np.float64)
    loc = rs.uniform(-0.5, 0.5, (n, 3)) * b[3:6]
    c, s = np.cos(b[6]), np.sin(b[6])
    return np.stack([loc[:, 0] * c - loc[:, 1] * s + b[0], loc[:, 0] * s + loc[:, 1] * c + b[1], loc[:, 2] + b[2]], axis=1)


def _background(rs, boxes, n, lo, hi):
    """Points of the scene outside every box's circumsphere."""
    out = np.zeros((0, 3))
    while len(out) < n:
        cand = rs.uniform(lo, hi, (n, 3))
        far = np.ones(len(cand), bool)
        for b in np.asarray(boxes, np.float64).reshape(-1, 7):
            far &= np.linalg.norm(cand - b[0:3], axis=1) > 0.5 * np.linalg.norm(b[3:6]) + 0.05
        out = np.concatenate([out, cand[far]])[:n]
    return out


def make_case(seed, boxes, fill, background, cfg, C=4, region=((0, -40, -3), (70, 40, 1)), cls=None, dead_share=0.0):
    """fill: per box either an int (points uniform in the box) or six ints (points well inside each face's pyramid).  The rows are shuffled, so a
    pyramid's members are spread over the whole scene; dead_share of them are dead on entry (keep = 0), and they are members as often as the
    others.  cls: the class code per box row (default 0); rows with -2 do not exist and get no points of their own."""
    rs = np.random.RandomState(seed)
    boxes = np.asarray(boxes, f32).reshape(-1, 7)
    cls = np.zeros(len(boxes), np.int32) if cls is None else np.asarray(cls, np.int32)
    pyramids = get_pyramids(boxes)                               # the band is kept from every row's pyramids, existing or not
    parts = []
    for i, want in enumerate(fill):
        if np.ndim(want) == 0:
            parts.append(_accept(rs, lambda m, i=i: _inside_box(rs, boxes[i], m), int(want), pyramids))
        else:
            for f, m in enumerate(want):
                parts.append(_accept(rs, lambda m_, i=i, f=f: _inside_pyramid(rs, pyramids[i, f], m_), int(m), pyramids))
    parts.append(_accept(rs, lambda m: _background(rs, boxes, m, region[0], region[1]), int(background), pyramids))
    xyz = np.concatenate(parts)
    xyz = xyz[rs.permutation(len(xyz))]
    extra = rs.uniform(0, 1, (len(xyz), C - 3)).astype(f32)
    points = np.concatenate([xyz, extra], axis=1).astype(f32)
    dead = rs.uniform(0, 1, len(points)) < dead_share
    return {"seed": int(seed), "boxes": boxes, "cls": cls, "points": points, "dead": dead, "cfg": dict(cfg)}


def _cfg(drop, sparsify, sparsify_max, swap, swap_max):
    return {"DROP_PROB": drop, "SPARSIFY_PROB": sparsify, "SPARSIFY_MAX_NUM": sparsify_max, "SWAP_PROB": swap, "SWAP_MAX_NUM": swap_max}


def _face_counts(case):
    """(boxes that exist, 6): the live points per pyramid on entry."""
    boxes = case["boxes"][case["cls"] != -2]
    return points_in_pyramids_mask(case["points"][~case["dead"]], get_pyramids(boxes)).sum(0).reshape(-1, 6)


def _all_stages(seed, build):
    """The first seed from `seed` on at which every stage the case enables (probability > 0) does something."""
    for seed in range(seed, seed + 50):
        c = build(seed)
        d = dict(run_case(c)[1])
        drop = (d["pyramid_drop_u"] <= c["cfg"]["DROP_PROB"]).any()
        if ((drop or not c["cfg"]["DROP_PROB"]) and (len(d["pyramid_sparsify_choice"]) or not c["cfg"]["SPARSIFY_PROB"])
                and (len(d["pyramid_swap_face"]) or not c["cfg"]["SWAP_PROB"])):
            return c
    raise AssertionError("no seed at which every stage acts")


_CASES = {}


def cases():
    """name -> case, built once.  Each states what it is for; the properties are asserted here, so a generator that stops producing them fails."""
    if _CASES:
        return _CASES
    rs = np.random.RandomState(20240)
    out = {}
    near, far_pi = (-3.0, 3.0), (3.10, 3.1415)

    # a scene of about 3 000 rows with dead points: ordered ranks cross a dozen chunks of a workgroup's sweep; boxes at 60-70 m, headings near +-pi
    boxes = [make_box(rs, (62.0, -12.0, -0.8), (4.1, 1.7, 1.5), far_pi), make_box(rs, (66.5, 9.0, -0.6), (3.8, 1.6, 1.6), (-3.1415, -3.10)),
             make_box(rs, (69.0, -1.0, -0.7), (1.5, 1.5, 1.5), near), make_box(rs, (30.0, 4.0, -0.9), (4.4, 1.8, 1.4), near),
             make_box(rs, (18.0, -20.0, -1.0), (0.8, 0.6, 1.7), near), make_box(rs, (45.0, 25.0, -0.5), (10.0, 2.6, 3.2), near)]
    out["large"] = _all_stages(1, lambda seed: make_case(seed, boxes, [420, 380, 300, 350, 120, 500], 930, _cfg(0.3, 0.5, 50, 0.6, 50), dead_share=0.1))
    # 70 rows, the thresholds at 5
    boxes = [make_box(rs, (12.0, 3.0, -1.0), (3.9, 1.6, 1.5), near), make_box(rs, (20.0, -6.0, -1.0), (4.2, 1.7, 1.6), near)]
    out["small"] = make_case(2, boxes, [(5, 6, 5, 6, 5, 6), (6, 5, 6, 5, 6, 5)], 4, _cfg(0.0, 1.0, 5, 1.0, 5))
    assert len(out["small"]["points"]) == 70 and (_face_counts(out["small"]) == [[5, 6, 5, 6, 5, 6], [6, 5, 6, 5, 6, 5]]).all()
    # exactly MAX_NUM points (left alone) against MAX_NUM + 1 (sparsified / valid), for 0, 5 and 50; every face of three boxes
    for mx in (0, 5, 50):
        boxes = [make_box(rs, (10.0 + 8 * i, -5.0 + 4 * i, -1.0), (3.6 + 0.3 * i, 1.6, 1.5), near) for i in range(3)]
        fill = [(mx, mx + 1, mx, mx + 1, mx, mx + 1), (mx + 1, mx, mx + 1, mx, mx + 1, mx), (mx + 1, mx + 1, mx, mx, mx + 1, mx + 1)]
        c = make_case(10 + mx, boxes, fill, 40, _cfg(0.0, 1.0, mx, 0.0, mx))
        assert (_face_counts(c) == np.array(fill)).all()
        out[f"sparsify_max{mx}"] = c
        c = make_case(20 + mx, boxes, fill, 40, _cfg(0.0, 0.0, mx, 1.0, mx))
        assert (_face_counts(c) == np.array(fill)).all()
        out[f"swap_max{mx}"] = c
    # no boxes; every box dropped (sparsify draws nothing); sparsify takes every box (the swap's uniform draws nothing)
    out["no_boxes"] = make_case(30, np.zeros((0, 7), f32), [], 50, _cfg(0.5, 0.5, 5, 0.5, 5))
    boxes = [make_box(rs, (15.0 + 7 * i, 2.0 * i, -1.0), (3.9, 1.6, 1.5), near) for i in range(3)]
    out["all_dropped"] = make_case(31, boxes, [90, 80, 70], 60, _cfg(1.0, 1.0, 5, 1.0, 5))
    out["all_sparsified"] = make_case(32, boxes, [90, 80, 70], 60, _cfg(0.0, 1.0, 5, 1.0, 5))
    # rows of another class take part (-1), rows that do not exist (-2) do not, though points lie inside them
    boxes = [make_box(rs, (14.0 + 6 * i, -8.0 + 5 * i, -1.0), (3.9, 1.6, 1.5), near) for i in range(5)]
    out["classes"] = _all_stages(33, lambda seed: make_case(seed, boxes, [120, 110, 100, 90, 80], 80, _cfg(0.3, 0.5, 5, 0.8, 5),
                                                            cls=[0, -2, -1, 1, -2], dead_share=0.15))
    # a single box: the swap's partner is the box itself and its points come out twice
    out["self_swap"] = make_case(34, [make_box(rs, (22.0, 1.0, -1.0), (4.0, 1.7, 1.5), near)], [600], 20, _cfg(0.0, 0.0, 5, 1.0, 5))
    # three boxes, two of which draw the same partner: the scene grows
    boxes = [make_box(rs, (15.0 + 7 * i, 3.0 * i, -1.0), (3.9, 1.6, 1.5), near) for i in range(3)]
    seed = 100
    while True:
        c = make_case(seed, boxes, [150, 150, 150], 30, _cfg(0.0, 0.0, 5, 1.0, 5))
        pts, draws, _ = run_case(c)
        d = dict(draws)
        pairs = list(zip(d["pyramid_swap_partner"].tolist(), d["pyramid_swap_face"].tolist()))
        if len(pairs) == 3 and len(set(pairs)) < 3 and len(pts) > len(c["points"]):
            break
        seed += 1
    assert seed < 200
    out["shared_partner"] = c
    # two overlapping boxes: points inside an involved pyramid of each
    boxes = [make_box(rs, (25.0, 0.0, -1.0), (4.0, 1.8, 1.5), (0.0, 0.1)), make_box(rs, (26.2, 0.3, -1.0), (4.0, 1.8, 1.5), (0.3, 0.5))]
    seed = 200
    while True:
        c = make_case(seed, boxes, [400, 400], 30, _cfg(0.0, 0.0, 5, 1.0, 5))
        m = points_in_pyramids_mask(c["points"], get_pyramids(c["boxes"]))
        d = dict(run_case(c)[1])
        cols = [int(i) * 6 + int(j) for i, j in zip(range(2), d["pyramid_swap_face"])] if len(d["pyramid_swap_face"]) == 2 else []
        cols += [int(p) * 6 + int(j) for p, j in zip(d["pyramid_swap_partner"], d["pyramid_swap_face"])]
        if cols and (m[:, sorted(set(cols))].sum(1) >= 2).sum() >= 3:
            break
        seed += 1
    assert seed < 300
    out["overlap"] = c
    # dropout and sparsify alone work for any C >= 3
    boxes = [make_box(rs, (12.0 + 9 * i, -3.0 * i, -1.0), (3.9, 1.6, 1.5), near) for i in range(3)]
    for C in (3, 5):
        out[f"columns{C}"] = _all_stages(40 + C, lambda seed: make_case(seed, boxes, [100, 90, 80], 50, _cfg(0.4, 0.7, 5, 0.0, 5), C=C, dead_share=0.1))
    out["columns3_swap"] = make_case(50, boxes, [100, 90, 80], 50, _cfg(0.0, 0.0, 5, 1.0, 5), C=3)
    assert TALLY.discarded <= MAX_DISCARD * TALLY.drawn, (TALLY.discarded, TALLY.drawn)
    _CASES.update(out)
    return _CASES


GOLDEN_CASES = ("large", "small", "sparsify_max0", "sparsify_max5", "sparsify_max50", "swap_max0", "swap_max5", "swap_max50", "no_boxes",
                "all_dropped", "all_sparsified", "classes", "self_swap", "shared_partner", "overlap", "columns3", "columns5")
