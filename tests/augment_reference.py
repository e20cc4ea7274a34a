"""Numpy restatement of the reference's training augmentation, the yardstick of tests/test_augment.py (test infrastructure only).

Restated, statement by statement and in fp32 where the reference computes in fp32:
  scale_pre_object                          detector3d/pcdet/datasets/augmentor/augmentor_utils.py:10-80
  random_flip_along_x / _y, global_rotation, global_scaling, random_translation_along_x / _y / _z      :82-160, :203-254
  limit_period + the gt_boxes_mask filter    datasets/augmentor/data_augmentor.py:258-272
  MIN_POINTS_OF_GT, class filter / column    datasets/dataset.py:126-157
  DataBaseSampler.__call__, add_sampled_boxes_to_scene      datasets/augmentor/database_sampler.py:358-479 (no road planes, no image paste)
  mask_points_by_range, mask_boxes_outside_range_numpy, shuffle_points     utils/common_utils.py:60-63, utils/box_utils.py:28-53, 93-109,
                                                                           datasets/processor/data_processor.py:78-103
PARITY UNPINNED: the reference's extensions (points_in_boxes_cpu, boxes_bev_iou_cpu) do not import here; the in-box test is the vectorised form of
oracle.pool_ops.points_in_boxes_cpu (held to it in tests/test_augment_reference.py) and the BEV IoU is oracle.boxes.boxes_iou_bev.

Dtypes.  Points and boxes are float32, the draws float64.  The reference ran under NumPy's value-based casting, which this file states explicitly
so that it does not depend on the installed NumPy: `float32 array * float64 array` is a float64 product rounded on assignment (the try boxes),
`float32 array * float64 scalar` is a float32 product with the scalar rounded first (new_lwh, the points, global_scaling, the rotation angle),
`float32 array += float64 array` is a float64 sum rounded on assignment (the translations, whose offset is normal(0, std, 1)).

Next to every moved coordinate the functions carry `err`, a bound on |device - this file| per element.  With u = 2**-24 (fp32 unit roundoff) an
implementation that evaluates a chain with r roundings and t trigonometric factors (cos / sin of an fp32 angle, at most 1 ulp = 2u off, |.| <= 1)
is off its exact value by at most (r + 2t) u S to first order, S the sum of the magnitudes of the chain's terms; two implementations differ by
at most twice that.
  object scaling, x:  ((px c - py s) f c' - (px s + py c) f s') + cx with px = x - cx:  r = 7 (sub, mul, add, mul f, mul, add, add), t = 2
                      -> 2 (7 + 4) u S = 22 u S, taken as 24 u S with S = 2 f (|px| + |py|) + |cx| + |x'|      (y alike)
                  z:  (z - cz) f + cz': r = 3, t = 0 -> 6 u S, taken as 8 u S with S = f |pz| + |cz'| + |z'|
  rotation:           x c - y s: r = 3, t = 2 (the angle itself is the same fp32 number on both sides) -> 14 u (|x| + |y|), taken as 16 u
  scaling, translation: one rounding each -> 2 u |x'|, taken as 4 u |x'|; flips are exact
and an incoming err passes through a rotation as err_x + err_y, through a scaling as f err, through the others unchanged.
"""
import numpy as np

f32 = np.float32
U = 2.0 ** -24
MARGIN = 1e-2
ROBUST = 1e-3                                                    # metres: every decision of a generated case is at least this far from flipping
APART = MARGIN + ROBUST                                          # boxes count as apart only beyond the IoU's own 1e-2 corner margin


# ------------------------------------------------------------------ the in-box test (roiaware_pool3d.cpp:121-165), vectorised
def in_box(xyz, box, margin=MARGIN):
    """xyz (M, 3) fp32, box (7+) fp32 -> (inside (M,) bool, gap (M,) float64: the distance of the nearest of the three comparisons from flipping)."""
    xyz = np.asarray(xyz, f32)
    cx, cy, cz, dx, dy, dz, rz = [f32(v) for v in box[:7]]
    zd = np.abs((xyz[:, 2] - cz).astype(f32)).astype(np.float64)
    z_in = ~(zd > float(dz) / 2.0)
    cosa, sina = f32(np.cos(f32(-rz))), f32(np.sin(f32(-rz)))
    sx, sy = (xyz[:, 0] - cx).astype(f32), (xyz[:, 1] - cy).astype(f32)
    lx = ((sx * cosa).astype(f32) + (sy * f32(-sina)).astype(f32)).astype(f32)
    ly = ((sx * sina).astype(f32) + (sy * cosa).astype(f32)).astype(f32)
    ax, ay = np.abs(lx.astype(np.float64)), np.abs(ly.astype(np.float64))
    hx, hy = float(dx) / 2.0 + float(f32(margin)), float(dy) / 2.0 + float(f32(margin))
    inside = z_in & (ax < hx) & (ay < hy)
    gap = np.minimum(np.abs(zd - float(dz) / 2.0), np.minimum(np.abs(ax - hx), np.abs(ay - hy)))
    return inside, gap


def points_in_boxes_count(points, boxes):
    """points_in_boxes_cpu(points, boxes).sum(axis=1) (dataset.py:131-133) and per point the smallest gap it met."""
    counts, gap = np.zeros(len(boxes), np.int64), np.full(len(points), np.inf)
    for i, b in enumerate(boxes):
        m, g = in_box(points[:, :3], b)
        counts[i] = m.sum()
        gap = np.minimum(gap, g)
    return counts, gap


# ------------------------------------------------------------------ float64 rectangle geometry, for the robustness of a case only
def _corners64(b):
    x, y, dx, dy, a = float(b[0]), float(b[1]), float(b[3]), float(b[4]), float(b[6])
    c, s = np.cos(a), np.sin(a)
    loc = np.array([[dx, dy], [-dx, dy], [-dx, -dy], [dx, -dy]]) / 2.0
    return loc @ np.array([[c, s], [-s, c]]) + np.array([x, y])


def separation64(a, b):
    """A lower bound of the distance between two rotated rectangles (separating axes of both), negative when they overlap."""
    A, B = _corners64(a), _corners64(b)
    best = -np.inf
    for poly in (A, B):
        for i in range(4):
            e = poly[(i + 1) % 4] - poly[i]
            n = np.array([e[1], -e[0]]) / np.hypot(*e)
            pa, pb = A @ n, B @ n
            best = max(best, pb.min() - pa.max(), pa.min() - pb.max())
    return best


def overlap64(a, b):
    """Intersection area of two rotated rectangles by clipping (float64)."""
    poly, clip = [tuple(p) for p in _corners64(a)], _corners64(b)
    for i in range(4):
        p0, p1 = clip[i], clip[(i + 1) % 4]
        side = lambda q: (p1[0] - p0[0]) * (q[1] - p0[1]) - (p1[1] - p0[1]) * (q[0] - p0[0])
        out = []
        for j in range(len(poly)):
            q0, q1 = poly[j], poly[(j + 1) % len(poly)]
            s0, s1 = side(q0), side(q1)
            if s0 >= 0:
                out.append(q0)
            if (s0 >= 0) != (s1 >= 0):
                t = s0 / (s0 - s1)
                out.append((q0[0] + t * (q1[0] - q0[0]), q0[1] + t * (q1[1] - q0[1])))
        poly = out
        if not poly:
            return 0.0
    x, y = np.array([p[0] for p in poly]), np.array([p[1] for p in poly])
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def pair_is_robust(a, b):
    """(collides, robust): robust when the pair is at least APART apart or overlaps by at least ROBUST m^2."""
    sep = separation64(a, b)
    if sep >= APART:
        return False, True
    area = overlap64(a, b)
    return True, area >= ROBUST


# ------------------------------------------------------------------ scale_pre_object (augmentor_utils.py:10-80)
def _rotate(x, y, c, s):
    """rotate_points_along_z's matmul row: x c + y (-s), x s + y c in fp32 (common_utils.py:35-57)."""
    nx = ((x * c).astype(f32) + (y * f32(-s)).astype(f32)).astype(f32)
    ny = ((x * s).astype(f32) + (y * c).astype(f32)).astype(f32)
    return nx, ny


def scale_pre_object(gt_boxes, points, gt_boxes_mask, scale_noises, iou_fn=None, check=True):
    """Returns (points with the dropped ones still in place, gt_boxes, alive (M,) bool, plan (N,) float64 with 0 = no free try, err (M, 3),
    robust: per point the smallest in-box gap it met, and whether every compared box pair was robust)."""
    if iou_fn is None:
        from oracle.boxes import boxes_iou_bev as iou_fn
    boxes, pts = np.array(gt_boxes, f32), np.array(points, f32)
    noises = np.asarray(scale_noises, np.float64)
    N, M = len(boxes), len(pts)
    alive, plan, err = np.ones(M, bool), np.zeros(N), np.zeros((M, 3))
    pgap, pairs_ok = np.full(M, np.inf), True
    for k in range(N):
        if gt_boxes_mask[k] == 0:
            continue
        num_try = noises.shape[1]
        scl = np.repeat(boxes[k][None], num_try, axis=0)
        scl[:, 3:6] = (boxes[k, 3:6].astype(np.float64)[None] * noises[k][:, None]).astype(f32)
        if N > 1:
            others = np.ones(N, bool)
            others[k] = False
            iou = iou_fn(scl[:, :7], boxes[others][:, :7])
            free = iou.max(axis=1) == 0
            try_idx = int(np.nonzero(free)[0][0]) if free.any() else -1
            if check:                                           # the tries that decide: those up to the chosen one
                for t in range(num_try if try_idx < 0 else try_idx + 1):
                    res = [pair_is_robust(scl[t], o) for o in boxes[others]]
                    if t == try_idx:
                        pairs_ok &= all(r and not c for c, r in res)
                    else:
                        pairs_ok &= any(c and r for c, r in res)
            if try_idx < 0:
                continue
        else:
            try_idx = 0
        s = noises[k][try_idx]
        sf = f32(s)
        plan[k] = s
        idx = np.nonzero(alive)[0]
        inb, gap = in_box(pts[idx, :3], boxes[k])
        pgap[idx] = np.minimum(pgap[idx], gap)
        cx, cy, cz, dx, dy, dz, ry = [f32(v) for v in boxes[k, :7]]
        ndx, ndy, ndz = f32(dx * sf), f32(dy * sf), f32(dz * sf)
        ncz = f32(cz + f32(f32(ndz - dz) / f32(2)))
        mv = idx[inb]
        px, py, pz = (pts[mv, 0] - cx).astype(f32), (pts[mv, 1] - cy).astype(f32), (pts[mv, 2] - cz).astype(f32)
        x1, y1 = _rotate(px, py, f32(np.cos(f32(-ry))), f32(np.sin(f32(-ry))))
        x2, y2, z2 = (x1 * sf).astype(f32), (y1 * sf).astype(f32), (pz * sf).astype(f32)
        x3, y3 = _rotate(x2, y2, f32(np.cos(ry)), f32(np.sin(ry)))
        nx, ny, nz = (x3 + cx).astype(f32), (y3 + cy).astype(f32), (z2 + ncz).astype(f32)
        spread = 2.0 * float(sf) * (np.abs(px.astype(np.float64)) + np.abs(py.astype(np.float64)))
        carried = 2.0 * float(sf) * (err[mv, 0] + err[mv, 1])     # an incoming error passes through both rotations
        err[mv, 0] = carried + 24 * U * (spread + abs(float(cx)) + np.abs(nx.astype(np.float64)))
        err[mv, 1] = carried + 24 * U * (spread + abs(float(cy)) + np.abs(ny.astype(np.float64)))
        err[mv, 2] = float(sf) * err[mv, 2] + 8 * U * (float(sf) * np.abs(pz.astype(np.float64)) + abs(float(ncz)) + np.abs(nz.astype(np.float64)))
        pts[mv, 0], pts[mv, 1], pts[mv, 2] = nx, ny, nz
        boxes[k, 2], boxes[k, 3], boxes[k, 4], boxes[k, 5] = ncz, ndx, ndy, ndz
        if s > 1:
            ina, gap = in_box(pts[idx, :3], boxes[k])
            pgap[idx] = np.minimum(pgap[idx], gap)
            alive[idx[inb ^ ina]] = False
    return pts, boxes, alive, plan, err, (pgap, pairs_ok)


# ------------------------------------------------------------------ gt_sampling (database_sampler.py:358-479)
def gt_sampling(points, gt_boxes, gt_boxes_mask, groups, extra_width, iou_fn=None, check=True):
    """groups: [(sampled_boxes (G, W), [obj_points (n, C) in the object's own frame, ...]), ...] in SAMPLE_GROUPS order.  Returns (points, gt_boxes,
    accept flags over all candidates in order, removed (M,) bool over the input points, robust = (gap per input point, pairs_ok)); with nothing
    accepted points and boxes are the input's."""
    if iou_fn is None:
        from oracle.boxes import boxes_iou_bev as iou_fn
    pts, boxes = np.array(points, f32), np.array(gt_boxes, f32)
    existed, accept, new_boxes, new_pts, pairs_ok = boxes.copy(), [], [], [], True
    for sampled, objs in groups:
        sampled = np.asarray(sampled, f32)
        iou2 = iou_fn(sampled[:, :7], sampled[:, :7])
        iou2[range(len(sampled)), range(len(sampled))] = 0
        iou1 = iou_fn(sampled[:, :7], existed[:, :7]) if len(existed) else iou2
        valid = (iou1.max(axis=1) + iou2.max(axis=1)) == 0
        if check:
            for i, v in enumerate(valid):
                res = [pair_is_robust(sampled[i], o) for o in existed] + [pair_is_robust(sampled[i], o) for j, o in enumerate(sampled) if j != i]
                pairs_ok &= all(r and not c for c, r in res) if v else any(c and r for c, r in res)
        accept += valid.tolist()
        existed = np.concatenate([existed, sampled[valid]])
        new_boxes += [b for b, v in zip(sampled, valid) if v]
        new_pts += [np.concatenate([(np.asarray(o, f32)[:, :3] + b[:3]).astype(f32), np.asarray(o, f32)[:, 3:]], axis=1) for o, b, v in zip(objs, sampled, valid) if v]
    gap, removed = np.full(len(pts), np.inf), np.zeros(len(pts), bool)
    if not new_boxes:
        return pts, boxes, np.array(accept, bool), removed, (gap, pairs_ok)
    large = np.stack(new_boxes)[:, :7].copy()
    large[:, 3:6] = (large[:, 3:6] + np.asarray(extra_width, f32)).astype(f32)
    for b in large:
        m, g = in_box(pts[:, :3], b)
        removed |= m
        gap = np.minimum(gap, g)
    out_pts = np.concatenate(new_pts + [pts[~removed]])
    out_boxes = np.concatenate([boxes[np.asarray(gt_boxes_mask, bool)], np.stack(new_boxes)])
    return out_pts, out_boxes, np.array(accept, bool), removed, (gap, pairs_ok)


# ------------------------------------------------------------------ world transforms (augmentor_utils.py:82-160, 203-254)
def world_transform(gt_boxes, points, ops, err=None):
    """ops: (name, value) in order with the names of seevcn_amd...augmentor_utils.OPS.  Returns boxes, points, err (M, 3), box_err (N, W)."""
    boxes, pts = np.array(gt_boxes, f32), np.array(points, f32)
    err = np.zeros((len(pts), 3)) if err is None else np.array(err, np.float64)
    berr = np.zeros(boxes.shape)
    a64 = lambda v: np.abs(np.asarray(v, np.float64))
    for name, v in ops:
        if name == "flip_x" and v:
            boxes[:, 1], boxes[:, 6], pts[:, 1] = -boxes[:, 1], -boxes[:, 6], -pts[:, 1]
            if boxes.shape[1] > 7:
                boxes[:, 8] = -boxes[:, 8]
        elif name == "flip_y" and v:
            boxes[:, 0], pts[:, 0] = -boxes[:, 0], -pts[:, 0]
            boxes[:, 6] = -(boxes[:, 6] + f32(np.pi)).astype(f32)
            berr[:, 6] += 4 * U * a64(boxes[:, 6])
            if boxes.shape[1] > 7:
                boxes[:, 7] = -boxes[:, 7]
        elif name == "rotation":
            ang = f32(v)
            c, s = f32(np.cos(ang)), f32(np.sin(ang))
            e = 16 * U * (a64(pts[:, 0]) + a64(pts[:, 1])) + err[:, 0] + err[:, 1]
            pts[:, 0], pts[:, 1] = _rotate(pts[:, 0].copy(), pts[:, 1].copy(), c, s)
            err[:, 0] = err[:, 1] = e
            e = 16 * U * (a64(boxes[:, 0]) + a64(boxes[:, 1])) + berr[:, 0] + berr[:, 1]
            boxes[:, 0], boxes[:, 1] = _rotate(boxes[:, 0].copy(), boxes[:, 1].copy(), c, s)
            berr[:, 0] = berr[:, 1] = e
            boxes[:, 6] = (boxes[:, 6] + ang).astype(f32)
            berr[:, 6] += 4 * U * a64(boxes[:, 6])
            if boxes.shape[1] > 7:
                e = 16 * U * (a64(boxes[:, 7]) + a64(boxes[:, 8])) + berr[:, 7] + berr[:, 8]
                boxes[:, 7], boxes[:, 8] = _rotate(boxes[:, 7].copy(), boxes[:, 8].copy(), c, s)
                berr[:, 7] = berr[:, 8] = e
        elif name == "scaling":
            sf = f32(v)
            pts[:, :3] = (pts[:, :3] * sf).astype(f32)
            err = float(sf) * err + 4 * U * a64(pts[:, :3])
            boxes[:, :6] = (boxes[:, :6] * sf).astype(f32)
            berr[:, :6] = float(sf) * berr[:, :6] + 4 * U * a64(boxes[:, :6])
        elif name.startswith("translation_"):
            c = "xyz".index(name[-1])
            pts[:, c] = (pts[:, c].astype(np.float64) + float(v)).astype(f32)
            err[:, c] += 4 * U * a64(pts[:, c])
            boxes[:, c] = (boxes[:, c].astype(np.float64) + float(v)).astype(f32)
            berr[:, c] += 4 * U * a64(boxes[:, c])
    return boxes, pts, err, berr


def limit_period(val, offset=0.5, period=2 * np.pi):
    """common_utils.py:22-25 as torch evaluates it on float32; the bound: three roundings around values of size |val| + period."""
    val, p = np.asarray(val, f32), f32(period)
    out = (val - (np.floor(((val / p).astype(f32) + f32(offset)).astype(f32)) * p).astype(f32)).astype(f32)
    return out, 8 * U * (np.abs(val.astype(np.float64)) + float(p))


# ------------------------------------------------------------------ the tail (dataset.py:152-157, data_processor.py:78-103)
def mask_points_by_range(points, limit_range):
    r = [float(v) for v in limit_range]
    x, y = points[:, 0].astype(np.float64), points[:, 1].astype(np.float64)
    return (x >= r[0]) & (x <= r[3]) & (y >= r[1]) & (y <= r[4])


def boxes_to_corners_3d(boxes):
    b = np.asarray(boxes, f32)
    t = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]], f32) / f32(2)
    loc = (b[:, None, 3:6] * t[None]).astype(f32)
    c, s = np.cos(b[:, 6]).astype(f32)[:, None], np.sin(b[:, 6]).astype(f32)[:, None]
    x = ((loc[:, :, 0] * c).astype(f32) + (loc[:, :, 1] * (-s)).astype(f32)).astype(f32)
    y = ((loc[:, :, 0] * s).astype(f32) + (loc[:, :, 1] * c).astype(f32)).astype(f32)
    return np.stack([x, y, loc[:, :, 2]], axis=2) + b[:, None, 0:3]


def mask_boxes_outside_range(boxes, limit_range, min_num_corners=1):
    corners = boxes_to_corners_3d(boxes[:, :7]).astype(np.float64)
    r = np.array([float(v) for v in limit_range])
    inside = ((corners >= r[0:3]) & (corners <= r[3:6])).all(axis=2)
    return inside.sum(axis=1) >= min_num_corners


def prepare_scene(points, gt_boxes, gt_cls, draws, min_points=1, point_range=None, min_num_corners=0, shuffle=None, num_points_in_gt=None,
                  check=True, extra_width=(0.0, 0.0, 0.0)):
    """One sample through MIN_POINTS_OF_GT, the augmentor queue (draws: the scene's list from draw_params; a gt_sampling entry holds (group, info)
    pairs whose infos carry box3d_lidar, class_index and points), the mask / class filter and the DataProcessor tail.  gt_cls: index into
    class_names or -1.  Returns points (n, C), gt_boxes (m, W + 1), err (n, 3), box_err (m, W + 1), robust = (per input point the smallest gap it
    met, whether every compared box pair was robust) and origin (n,): the input row of every output point, -1 for a pasted one."""
    pts, boxes, cls = np.array(points, f32), np.array(gt_boxes, f32), np.asarray(gt_cls)
    counts, gap = points_in_boxes_count(pts, boxes) if num_points_in_gt is None else (np.asarray(num_points_in_gt), np.full(len(pts), np.inf))
    boxes, cls = boxes[counts >= min_points], cls[counts >= min_points]
    mask = cls >= 0
    origin, err, pairs_ok = np.arange(len(pts)), np.zeros((len(pts), 3)), True
    world = []
    berr = np.zeros(boxes.shape)

    def flush():
        nonlocal boxes, pts, err, berr, world
        if world:
            boxes, pts, err, be = world_transform(boxes, pts, world, err)
            berr = berr + be                                    # (a bound: earlier box errors are small against it)
            world = []

    def note(g):
        gap[origin[origin >= 0]] = np.minimum(gap[origin[origin >= 0]], g[origin >= 0])

    for name, value in draws:
        if name == "object_scaling":
            flush()
            pts, boxes, alive, _, e2, (g, ok) = scale_pre_object(boxes, pts, mask, value, check=check)
            err = np.maximum(err, e2)
            note(g)
            pts, err, origin = pts[alive], err[alive], origin[alive]
            pairs_ok = pairs_ok and ok
        elif name == "gt_sampling":
            flush()
            groups = []
            for gid in sorted({g for g, _ in value}):
                infos = [i for g, i in value if g == gid]
                groups.append((np.stack([np.asarray(i["box3d_lidar"], f32) for i in infos]), [i["points"] for i in infos]))
            new_pts, new_boxes, accept, removed, (g, ok) = gt_sampling(pts, boxes, mask, groups, extra_width, check=check)
            note(g)
            pairs_ok = pairs_ok and ok
            if accept.any():
                n_new = len(new_pts) - int((~removed).sum())
                err = np.concatenate([np.zeros((n_new, 3)), err[~removed]])
                origin = np.concatenate([np.full(n_new, -1), origin[~removed]])
                cls = np.concatenate([cls[mask], [i["class_index"] for (_, i), a in zip(value, accept) if a]])
                berr = np.concatenate([berr[mask], np.zeros((int(accept.sum()), berr.shape[1]))])
                pts, boxes, mask = new_pts, new_boxes, np.ones(len(new_boxes), bool)
        else:
            world.append((name, value))
    flush()
    if len(boxes):
        boxes[:, 6], e = limit_period(boxes[:, 6])
        berr[:, 6] += e
    boxes, berr, cls = boxes[mask], berr[mask], cls[mask]
    boxes = np.concatenate([boxes, (cls + 1).astype(f32)[:, None]], axis=1)
    berr = np.concatenate([berr, np.zeros((len(berr), 1))], axis=1)
    if point_range is not None:
        m = mask_points_by_range(pts, point_range)
        pts, err, origin = pts[m], err[m], origin[m]
        if min_num_corners:
            m = mask_boxes_outside_range(boxes, point_range, min_num_corners)
            boxes, berr = boxes[m], berr[m]
    if shuffle is not None:
        pts, err, origin = pts[shuffle], err[shuffle], origin[shuffle]
    return pts, boxes, err, berr, (gap, pairs_ok), origin


def collate(samples):
    """collate_batch's points / gt_boxes: [b, x, y, z, ...] rows and (B, max_gt, W + 1) zero padded."""
    pts = np.concatenate([np.concatenate([np.full((len(p), 1), b, f32), p], axis=1) for b, (p, _) in enumerate(samples)])
    max_gt = max(len(g) for _, g in samples)
    width = samples[0][1].shape[1]
    gt = np.zeros((len(samples), max_gt, width), f32)
    for b, (_, g) in enumerate(samples):
        gt[b, :len(g)] = g
    return pts, gt


# ------------------------------------------------------------------ seeded case generators
def make_boxes(rng, n, extent=40.0, min_gap=1.5, width=7):
    """n boxes on a jittered grid, every pair at least min_gap apart at any heading (circumscribed circles)."""
    side = int(np.ceil(np.sqrt(max(n, 1))))
    pitch = 2 * extent / side
    assert pitch > 5.4 + min_gap, "too many boxes for the extent"
    cells = rng.permutation(side * side)[:n]
    out = np.zeros((n, width), f32)
    for i, c in enumerate(cells):
        out[i, 0] = -extent + (c % side + 0.5) * pitch + rng.uniform(-0.2, 0.2)
        out[i, 1] = -extent + (c // side + 0.5) * pitch + rng.uniform(-0.2, 0.2)
        out[i, 2] = rng.uniform(-1.2, -0.6)
        out[i, 3:6] = [rng.uniform(3.2, 4.6), rng.uniform(1.5, 2.0), rng.uniform(1.4, 1.8)]
        out[i, 6] = rng.uniform(-np.pi, np.pi)
        if width > 7:
            out[i, 7:9] = rng.uniform(-5, 5, 2)
    return out


def make_points(rng, boxes, n_bg, per_box, C=5, extent=44.0, spread=0.75):
    """Background points plus per_box points in and closely around every box: uniform over `spread` times the box's size either side of its centre
    (0.75: scaling moves some and an enlarged box swallows others)."""
    parts = [np.concatenate([rng.uniform(-extent, extent, (n_bg, 2)), rng.uniform(-2.5, 1.0, (n_bg, 1))], axis=1)]
    for b in boxes:
        loc = rng.uniform(-spread, spread, (per_box, 3)) * b[3:6].astype(np.float64)
        c, s = np.cos(float(b[6])), np.sin(float(b[6]))
        parts.append(np.stack([loc[:, 0] * c - loc[:, 1] * s + b[0], loc[:, 0] * s + loc[:, 1] * c + b[1], loc[:, 2] + b[2]], axis=1))
    xyz = np.concatenate(parts)
    pts = np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), C - 3))], axis=1).astype(f32)
    return pts[rng.permutation(len(pts))]


def robust_scene(points, run):
    """Drop the input points that sit within ROBUST of a face they are tested against, until `run(points)` -> (gap per input point or a scalar)
    reports none.  run returns an (M,) array of the smallest gap each input point met (inf when never tested)."""
    pts = np.array(points, f32)
    for _ in range(8):
        gaps = run(pts)
        bad = gaps < ROBUST
        if not bad.any():
            return pts
        pts = pts[~bad]
    raise AssertionError("the case does not become robust")
