"""The VCN validation metrics restated in numpy, the reference's way, with the seeded cases and the bounds the GPU tests hold the kernels to.

UNPINNED.  The reference's Metrics.get (see/surface_completion/models/vcn/utils/metrics.py) cannot run here: open3d, its CUDA Chamfer extension
and its iou3d_nms extension do not import.  Like the spconv and shapely restatements, this file states the arithmetic from the reference's source
and is the yardstick of the kernels; nothing pins it against an execution of the reference.

What is restated (values30): for every enabled item and every group (the whole batch, then num_pts levels L1 .. L4) the batch is MASKED and the
metric recomputed on the subset, as Metrics._get_* do: ChamferDistanceL1/L2 with ignore_zeros acting exactly when the subset holds one object
(chamfer_dist/__init__.py:37), the `except` that turns a failed call into -1, get_oob_error through the set difference of row tuples and
torch.unique without dim, the diagonal of the 3-D IoU of get_bbox_from_keypoints' box, the lower median of |rotm_to_heading - heading|, the mean of
|reg_centre - centre|.  The per-point Chamfer distance is the kernels' stated fp32, bit for bit: min over the other cloud of
(dx*dx + dy*dy) + dz*dz, every operation rounded to float32.  Everything else is float64 on the float32 inputs.

Where parity with the reference ends (stated, not measured): its box extents and heading use torch's fp32 cos / sin / bmm / atan2, its IoU the
fp32 polygon construction of iou3d_nms (held to float64 by tests/box_reference.py's allowance), open3d's crop an OrientedBoundingBox fitted to the
eight corners of opd_to_boxpts -- here the cuboid itself, faces inclusive.

BOUNDS.  u = 2^-24.  A sum of k non-negative fp32 terms in any order is within gamma(k - 1) = (k - 1) u / (1 - (k - 1) u) of the real sum, relative
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4); every further correctly rounded sqrt, division, product or int -> float
conversion multiplies by (1 + u).  The kernels' orders (csrc/vc_metrics.hip) are sums of that kind, so each bound below is built from those two facts
and the number of operations the kernel states; no constant is chosen.  The device's trigonometry is given the allowance DESIGN.md already uses for
it, 16 ulp.  The IoU uses tests/box_reference.py's per-pair allowance K_KERNEL * area_unit on the BEV overlap, and its corner-band sandwich.
"""
import functools

import numpy as np

import box_reference as br

U = 2.0 ** -24
EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
TRIG_ULPS = 16                      # DESIGN.md's allowance for the device's atan2 / cos / sin against numpy's
ITEM_NAMES = ("CDL1", "CDL2", "OUT_OF_BOX", "IOU_3D", "Rotation_Error", "Translation_Error")
LEVELS = (("L1", 201, 1000000), ("L2", 81, 200), ("L3", 31, 80), ("L4", 5, 30))
NAMES = [n + s for n in ITEM_NAMES for s in ("",) + tuple("_" + l for l, _, _ in LEVELS)]
TILE = 1024                         # rows of the complete cloud the kernel stages at a time (asserted against the library by the GPU test)
SCALE = 128.0                       # every coordinate and extent of every case is below this

# The float64 membership test computes lx = dx * c + dy * s with |dx|, |dy| < 2 SCALE.  A difference of TRIG_ULPS ulp in c and s (|c|, |s| <= 1)
# moves lx by at most 2 * (2 SCALE) * TRIG_ULPS * EPS64 / 2; the products, the sum and the subtractions p - centre add at most 4 roundings of
# values below 4 SCALE.  A point further than GAP from every face is decided the same way by both evaluations.
GAP = (2 * SCALE * TRIG_ULPS * EPS64) + 4 * (4 * SCALE) * (EPS64 / 2)


def gamma(k):
    k = max(int(k), 0)
    return k * U / (1.0 - k * U)


def group_masks(num_pts):
    num_pts = np.asarray(num_pts)
    return [np.ones(len(num_pts), bool)] + [(num_pts >= lo) & (num_pts <= hi) for _, lo, hi in LEVELS]


# ------------------------------------------------------------------------------------------ the stated arithmetic
def nn_dist32(a, b):
    """(n,3), (m,3) float32 -> (n,) float32: min over b of (dx*dx + dy*dy) + dz*dz, every operation rounded to float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    out = np.empty(len(a), np.float32)
    for i0 in range(0, len(a), 64):
        d = b[None, :, :] - a[i0:i0 + 64, None, :]
        sq = d * d
        out[i0:i0 + 64] = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]).min(1)
    return out


def nonzero_rows(x):
    """torch.sum(xyz, dim=2).ne(0) on float32: (x + y) + z != 0"""
    x = np.asarray(x, np.float32)
    return ((x[:, 0] + x[:, 1]) + x[:, 2]) != 0


def chamfer_module(pred, gt, l1):
    """ChamferDistanceL1 / L2 (ignore_zeros=True).forward on a (possibly masked) batch; raises like the extension on an empty cloud."""
    if len(pred) == 1:
        pred, gt = [pred[0][nonzero_rows(pred[0])]], [gt[0][nonzero_rows(gt[0])]]
        if len(pred[0]) == 0 or len(gt[0]) == 0:
            raise RuntimeError("empty cloud")
    d1 = np.concatenate([nn_dist32(p, g) for p, g in zip(pred, gt)]).astype(np.float64)
    d2 = np.concatenate([nn_dist32(g, p) for p, g in zip(pred, gt)]).astype(np.float64)
    if l1:
        return (np.sqrt(d1).mean() + np.sqrt(d2).mean()) / 2
    return d1.mean() + d2.mean()


def inside_box(pc, box):
    """opd_to_boxpts' cuboid, faces inclusive, float64 on the float32 inputs: (n,) bool and the distance of every point to the nearest face plane"""
    p, b = np.asarray(pc, np.float32).astype(np.float64), np.asarray(box, np.float32).astype(np.float64)
    c, s = np.cos(b[6]), np.sin(b[6])
    dx, dy, dz = p[:, 0] - b[0], p[:, 1] - b[1], p[:, 2] - b[2]
    lx, ly = dx * c + dy * s, -dx * s + dy * c
    g = np.stack([np.abs(lx) - b[3] / 2, np.abs(ly) - b[4] / 2, np.abs(dz) - b[5] / 2], 1)
    return (g <= 0).all(1), np.abs(g).min(1)


def oob_counts(pc, box):
    """get_oob_points + torch.unique: (distinct rows outside, distinct scalars), the reference's way: a set difference of row tuples."""
    pc = np.asarray(pc, np.float32)
    inside, _ = inside_box(pc, box)
    pc_set = set(map(tuple, pc.tolist()))
    crop_set = set(map(tuple, pc[inside].tolist()))
    return len(pc_set - crop_set), len(np.unique(pc))


def oob_ratio32(pc, box):
    """num_oob / num_pc as the float32 the reference keeps (.float() of the float64 quotient; the fp32 quotient of the two integers is the same
    number: both are below 2^24 and 53 >= 2 * 24 + 2 bits make the double rounding innocuous)"""
    a, b = oob_counts(pc, box)
    return np.float32(np.float32(a) / np.float32(b))


def pred_box64(coarse, box):
    """get_bbox_from_keypoints in float64: centre of the bounds, extents of (p - centre) @ rot_from_heading(h).T, heading"""
    p, h = np.asarray(coarse, np.float32).astype(np.float64), float(np.float32(box[6]))
    centre = (p.max(0) + p.min(0)) / 2
    c, s = np.cos(h), np.sin(h)
    d = p - centre
    norm = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1)
    return np.concatenate([centre, norm.max(0) - norm.min(0), [h]])


def _bev_overlap64(a, b, grow=0.0):
    a, b = np.asarray(a, np.float64)[None], np.asarray(b, np.float64)[None]
    if ((a[:, 3:5] + 2 * grow) <= 0).any() or ((b[:, 3:5] + 2 * grow) <= 0).any():
        return 0.0
    return float(br._clip_area_batch(br._corners_batch(a, grow), br._corners_batch(b, grow))[0])


def iou3d_from_overlap(a, b, overlap_bev):
    """boxes_iou3d_gpu's arithmetic in float64 from a given BEV overlap"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    h = max(min(a[2] + a[5] / 2, b[2] + b[5] / 2) - max(a[2] - a[5] / 2, b[2] - b[5] / 2), 0.0)
    o3 = overlap_bev * h
    return o3 / max(a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - o3, 1e-6)


def iou3d64(a, b):
    return iou3d_from_overlap(a, b, _bev_overlap64(a, b))


def heading_error64(rot, heading):
    r = np.asarray(rot, np.float32).astype(np.float64)[0]
    nrm = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    return abs(np.arctan2(r[1] / nrm, r[0] / nrm) - float(np.float32(heading)))


# ------------------------------------------------------------------------------------------ Metrics.get, the reference's way
def values30(case):
    """The 30 values in NAMES order (float64; -1 as the reference returns it): mask, recompute per group."""
    coarse, complete, boxes, num_pts = case["coarse"], case["complete"], case["gt_boxes"], case["num_pts"]
    rot, centre = case["reg_rot"], case["reg_centre"]
    masks = group_masks(num_pts)
    out = []

    def chamfer(mask, l1):
        if complete.shape[1] == 1:
            return -1
        if not mask.any():
            return -1
        try:
            return chamfer_module(list(coarse[mask]), list(complete[mask]), l1) * 1000
        except RuntimeError:
            return -1

    out += [chamfer(m, True) for m in masks]
    out += [chamfer(m, False) for m in masks]
    for m in masks:
        if not m.any():
            out.append(-1)
            continue
        ratios = np.array([oob_ratio32(p, b) for p, b in zip(coarse[m], boxes[m])], np.float32)
        out.append(float(ratios.astype(np.float64).mean()))
    for m in masks:
        out.append(float(np.mean([iou3d64(pred_box64(p, b), b.astype(np.float64)) for p, b in zip(coarse[m], boxes[m])])) if m.any() else -1)
    for m in masks:
        if rot is None or not m.any():
            out.append(-1)
            continue
        errs = np.sort([heading_error64(r, b[6]) for r, b in zip(rot[m], boxes[m])])
        out.append(float(errs[(len(errs) - 1) // 2]))                 # torch.median: the lower of the two middle elements
    for m in masks:
        if centre is None or not m.any():
            out.append(-1)
            continue
        out.append(float(np.abs(centre[m].astype(np.float64) - boxes[m][:, :3].astype(np.float64)).mean()))
    return np.array(out, np.float64)


# ------------------------------------------------------------------------------------------ per object, once (what the kernel's table holds)
def per_object(case):
    """Every per-object quantity of the kernel's table in float64 (sums of the fp32 distances), with the bound of each fp32 column."""
    coarse, complete, boxes = case["coarse"], case["complete"], case["gt_boxes"]
    B, n, m = len(coarse), coarse.shape[1], complete.shape[1]
    t = {k: np.zeros(B) for k in ("d1", "s1", "d2", "s2", "zd1", "zs1", "zd2", "zs2", "iou", "rot", "trans", "tol_rot", "tol_trans")}
    t.update(nz1=np.zeros(B, np.int64), nz2=np.zeros(B, np.int64), num_oob=np.zeros(B, np.int64), num_pc=np.zeros(B, np.int64),
             ratio=np.zeros(B, np.float32), box=np.zeros((B, 7)), tol_box=np.zeros((B, 6)), dist1=[], dist2=[])
    for b in range(B):
        p, g, box = coarse[b], complete[b], boxes[b]
        d1, d2 = nn_dist32(p, g).astype(np.float64), nn_dist32(g, p).astype(np.float64)
        t["dist1"].append(d1), t["dist2"].append(d2)
        t["d1"][b], t["s1"][b], t["d2"][b], t["s2"][b] = d1.sum(), np.sqrt(d1).sum(), d2.sum(), np.sqrt(d2).sum()
        k1, k2 = nonzero_rows(p), nonzero_rows(g)
        t["nz1"][b], t["nz2"][b] = k1.sum(), k2.sum()
        if k1.any() and k2.any():
            z1, z2 = nn_dist32(p[k1], g[k2]).astype(np.float64), nn_dist32(g[k2], p[k1]).astype(np.float64)
            t["zd1"][b], t["zs1"][b], t["zd2"][b], t["zs2"][b] = z1.sum(), np.sqrt(z1).sum(), z2.sum(), np.sqrt(z2).sum()
        t["num_oob"][b], t["num_pc"][b] = oob_counts(p, box)
        t["ratio"][b] = oob_ratio32(p, box)
        pb = pred_box64(p, box)
        t["box"][b] = pb
        t["iou"][b] = iou3d64(pb, box.astype(np.float64))
        # the box's bound.  Centre: one rounding of max + min (the halving is exact).  Extents: the kernel's nx = fl(fl(dx c) + fl(dy s)) with
        # dx = fl(x - cx): against float64 each of c, s is off by at most TRIG_ULPS * EPS32 (|c|, |s| <= 1), each dx by u |dx| and the centre's own
        # rounding, each product and the sum by u: (|dx| + |dy|) (TRIG_ULPS EPS32 + 3 u) + u (|cx| + |cy|) per point, twice for max - min, and one
        # rounding of the difference.  z: the centre's rounding and one subtraction, twice, and the difference.
        p64 = p.astype(np.float64)
        reach = (np.abs(p64[:, 0] - pb[0]) + np.abs(p64[:, 1] - pb[1])).max()
        t["tol_box"][b, :3] = U * np.abs(p64.max(0) + p64.min(0))
        xy = 2 * (reach * (TRIG_ULPS * EPS32 + 3 * U) + U * (abs(pb[0]) + abs(pb[1]))) + U * max(pb[3], pb[4])
        t["tol_box"][b, 3:5] = xy
        t["tol_box"][b, 5] = 2 * (U * abs(pb[2]) + U * np.abs(p64[:, 2] - pb[2]).max()) + U * pb[5]
        if case["reg_rot"] is not None:
            e = heading_error64(case["reg_rot"][b], box[6])
            t["rot"][b] = e
            # sum of three squares gamma(3) (products and two sums), halved by the root, + u for the root, + u for each quotient: the relative error of
            # both arguments; atan2 moves by at most that (|x dy - y dx| / (x^2 + y^2) <= 2 |x y| rel / (x^2 + y^2) <= rel); the device's atan2f gets
            # TRIG_ULPS ulp of a result below pi; the subtraction and the absolute value one rounding of the result.
            theta = abs(e) + abs(float(box[6]))
            t["tol_rot"][b] = (gamma(3) / 2 + 2 * U) + TRIG_ULPS * EPS32 * theta + U * e
        if case["reg_centre"] is not None:
            e = np.abs(case["reg_centre"][b].astype(np.float64) - box[:3].astype(np.float64)).mean()
            t["trans"][b] = e
            t["tol_trans"][b] = ((1 + U) ** 4 - 1) * e                 # three differences, two sums of non-negative terms, one division
    # sums of fp32 terms in the kernel's order: gamma(count - 1); the root sums carry one more rounding a term
    t["tol_d1"], t["tol_s1"] = gamma(n - 1) * t["d1"], gamma(n) * t["s1"]
    t["tol_d2"], t["tol_s2"] = gamma(m - 1) * t["d2"], gamma(m) * t["s2"]
    t["tol_zd1"], t["tol_zs1"] = np.array([gamma(k - 1) for k in t["nz1"]]) * t["zd1"], np.array([gamma(k) for k in t["nz1"]]) * t["zs1"]
    t["tol_zd2"], t["tol_zs2"] = np.array([gamma(k - 1) for k in t["nz2"]]) * t["zd2"], np.array([gamma(k) for k in t["nz2"]]) * t["zs2"]
    return t


def iou_interval(pred_box32, gt_box):
    """The interval the kernel's fp32 IoU of (its own fp32 predicted box, the ground truth) must lie in: box_reference's allowance K_KERNEL *
    area_unit around the exact BEV overlap, the grown overlap on the upper side when a corner lies in the margin band (the sandwich of
    Case.sandwich_misses), through the monotone o / (va + vb - o) in float64, and (1 + u)^8 for the fp32 operations behind the overlap (two
    products for each volume, the height difference, the product, the sum and difference, the division)."""
    a = np.asarray(pred_box32, np.float32)
    b = np.asarray(gt_box, np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    exact = _bev_overlap64(a64, b64)
    band = bool(br.corner_band(a, b))
    upper = _bev_overlap64(a64, b64, br.MARGIN + br.BAND_DELTA) if band else exact
    s = br.K_KERNEL * float(br.area_unit(a[None], b[None])[0, 0])
    lo, hi = iou3d_from_overlap(a64, b64, max(exact - s, 0.0)), iou3d_from_overlap(a64, b64, upper + s)
    r = (1 + U) ** 8 - 1
    return lo * (1 - r) - 1e-6 * r, hi * (1 + r) + 1e-6 * r


def values30_from_objects(case, t=None):
    """The 30 values recomputed from the per-object quantities (the kernels' route, in float64) and the bound of each."""
    t = per_object(case) if t is None else t
    n, m = case["coarse"].shape[1], case["complete"].shape[1]
    vals, tols = np.full(30, -1.0), np.zeros(30)
    for g, mask in enumerate(group_masks(case["num_pts"])):
        cnt = int(mask.sum())
        if cnt == 0:
            continue
        idx = np.flatnonzero(mask)
        add = gamma(cnt - 1)                                           # the sum over the group's objects, ascending index
        if m != 1:
            if cnt == 1:
                b = idx[0]
                if t["nz1"][b] > 0 and t["nz2"][b] > 0:
                    k1, k2 = float(t["nz1"][b]), float(t["nz2"][b])
                    m1, m2, e1, e2 = t["zs1"][b] / k1, t["zs2"][b] / k2, t["tol_zs1"][b] / k1, t["tol_zs2"][b] / k2
                    q1, q2, f1, f2 = t["zd1"][b] / k1, t["zd2"][b] / k2, t["tol_zd1"][b] / k1, t["tol_zd2"][b] / k2
                else:
                    m1 = None
            else:
                k1, k2 = float(cnt * n), float(cnt * m)
                m1, m2 = t["s1"][idx].sum() / k1, t["s2"][idx].sum() / k2
                q1, q2 = t["d1"][idx].sum() / k1, t["d2"][idx].sum() / k2
                e1, e2 = t["tol_s1"][idx].sum() / k1 + add * m1, t["tol_s2"][idx].sum() / k2 + add * m2
                f1, f2 = t["tol_d1"][idx].sum() / k1 + add * q1, t["tol_d2"][idx].sum() / k2 + add * q2
            if m1 is not None:
                # behind the sums: the conversion of each denominator, each division, the sum of the two means, the product with 1000: (1 + u)^4
                r = (1 + U) ** 4 - 1
                vals[g], tols[g] = (m1 + m2) / 2 * 1000, ((e1 + e2) / 2 * (1 + r) + r * (m1 + m2) / 2) * 1000
                vals[5 + g], tols[5 + g] = (q1 + q2) * 1000, ((f1 + f2) * (1 + r) + r * (q1 + q2)) * 1000
        r = (1 + U) ** 2 - 1                                           # count -> float, the division
        oob = t["ratio"][idx].astype(np.float64).mean()
        vals[10 + g], tols[10 + g] = oob, (add + r) * oob
        iou = t["iou"][idx].mean()
        vals[15 + g], tols[15 + g] = iou, t["tol_iou"][idx].mean() * (1 + add + r) + (add + r) * iou if "tol_iou" in t else 0.0
        if case["reg_rot"] is not None:
            errs = np.sort(t["rot"][idx])
            # two sequences that differ by at most e element by element have order statistics that differ by at most e
            vals[20 + g], tols[20 + g] = errs[(cnt - 1) // 2], t["tol_rot"][idx].max()
        if case["reg_centre"] is not None:
            tr = t["trans"][idx].mean()
            vals[25 + g], tols[25 + g] = tr, t["tol_trans"][idx].mean() * (1 + add + r) + (add + r) * tr
    return vals, tols


def iou_tolerance(case, t):
    """|kernel IoU - float64 IoU of the float64 box| per object, bounded WITHOUT the kernel's output: the box's bound moves each side of the
    predicted rectangle by at most tol_centre + tol_extent / 2, which sweeps at most that times the side's length; the overlap's own allowance and
    the band's sandwich as in iou_interval; heights and volume through interval ends."""
    B = len(case["coarse"])
    out = np.zeros(B)
    for b in range(B):
        a64, g32 = t["box"][b], case["gt_boxes"][b]
        g64 = g32.astype(np.float64)
        tb = t["tol_box"][b]
        a32 = a64.astype(np.float32)
        move = (tb[0] + tb[3] / 2) * 2 * a64[4] + (tb[1] + tb[4] / 2) * 2 * a64[3] + 4 * (tb[0] + tb[3] / 2) * (tb[1] + tb[4] / 2)
        exact = _bev_overlap64(a64, g64)
        # the band is decided on boxes whose margin is widened by the box's bound, so that the kernel's own box cannot be in the band unseen
        band = bool(br.corner_band(a32, g32, br.MARGIN, br.BAND_DELTA + float(tb[:5].max()) * 2 + 2 * EPS32 * SCALE))
        grow = br.MARGIN + br.BAND_DELTA + float(tb[:5].max()) * 2 + 2 * EPS32 * SCALE
        upper = _bev_overlap64(a64, g64, grow) if band else exact
        s = br.K_KERNEL * float(br.area_unit(a32[None], g32[None])[0, 0]) * (1 + 4 * EPS32) + move
        lo_box, hi_box = a64.copy(), a64.copy()
        lo_box[5], hi_box[5] = max(a64[5] - tb[5] - 2 * tb[2], 0.0), a64[5] + tb[5] + 2 * tb[2]    # height overlap: shrink / stretch the box in z
        va_lo = max(a64[3] - tb[3], 0) * max(a64[4] - tb[4], 0) * max(a64[5] - tb[5], 0)
        va_hi = (a64[3] + tb[3]) * (a64[4] + tb[4]) * (a64[5] + tb[5])
        vb = g64[3] * g64[4] * g64[5]

        def iou(o, box, va):
            h = max(min(box[2] + box[5] / 2, g64[2] + g64[5] / 2) - max(box[2] - box[5] / 2, g64[2] - g64[5] / 2), 0.0)
            o3 = o * h
            return o3 / max(va + vb - o3, 1e-6)

        lo, hi = iou(max(exact - s, 0.0), lo_box, va_hi), iou(upper + s, hi_box, max(va_lo, 0.0))
        r = (1 + U) ** 8 - 1
        lo, hi = lo * (1 - r) - 1e-6 * r, hi * (1 + r) + 1e-6 * r
        out[b] = max(t["iou"][b] - lo, hi - t["iou"][b], 0.0)
    return out


# ------------------------------------------------------------------------------------------ the seeded cases
HEADINGS = (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 0.3, -2.1, 1.234, 2.9, -0.7, 0.05, -3.0, 1.9, -1.2, 2.2, 0.9, -0.4)


def _rand_box(rng, heading):
    return np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-1, 1), rng.uniform(3.1, 5.3), rng.uniform(1.55, 2.3),
                     rng.uniform(1.35, 1.9), heading], np.float32)


def _cloud_around(rng, box, count, where, quantum=None):
    """count rows placed in the box's frame: 'inside' within 0.8 of the half extents, 'outside' beyond 1.3 of one of them, 'mixed' either"""
    b = box.astype(np.float64)
    half = b[3:6] / 2
    local = rng.uniform(-0.8, 0.8, (count, 3)) * half
    if where != "inside":
        out = np.ones(count, bool) if where == "outside" else rng.random(count) < 0.35
        axis = rng.integers(0, 3, count)
        far = rng.choice([-1.0, 1.0], count) * rng.uniform(1.3, 1.8, count) * half[axis]
        local[out, axis[out]] = far[out]
    c, s = np.cos(b[6]), np.sin(b[6])
    world = np.stack([b[0] + local[:, 0] * c - local[:, 1] * s, b[1] + local[:, 0] * s + local[:, 1] * c, b[2] + local[:, 2]], 1)
    if quantum:
        world = np.round(world / quantum) * quantum                   # duplicate scalars (and, in small clouds, duplicate rows)
    return world.astype(np.float32)


def make_case(name, B, n, m, num_pts, seed, where="mixed", regress=True, zero_rows=(), all_zero=(), quantum=None, tie=()):
    """One batch.  zero_rows: objects that get rows (0, 0, 0) and (a, -a, 0) in both clouds; all_zero: objects whose coarse cloud is nothing but
    such rows; tie: pairs of objects with the same heading and the same reg_rot (equal heading errors, bit for bit)."""
    rng = np.random.default_rng(seed)
    headings = [HEADINGS[b % len(HEADINGS)] for b in range(B)]
    for i, j in tie:
        headings[j] = headings[i]
    boxes = np.stack([_rand_box(rng, headings[b]) for b in range(B)])
    w = where if isinstance(where, (list, tuple)) else [where] * B
    coarse = np.stack([_cloud_around(rng, boxes[b], n, w[b], quantum) for b in range(B)])
    complete = np.stack([_cloud_around(rng, boxes[b], m, "inside") for b in range(B)])
    for b in range(B):
        if n >= 8:                                                    # duplicate rows
            coarse[b, n // 2:n // 2 + 3] = coarse[b, 0:3]
            coarse[b, n - 1] = coarse[b, 1]
    for b in zero_rows:
        for cloud in (coarse[b], complete[b]):
            k = len(cloud)
            a = np.float32(rng.uniform(0.5, 3.0))
            cloud[0] = 0
            if k > 2:
                cloud[k // 3] = (a, -a, 0)
            if k > 5:
                cloud[k - 2] = (0, 0, 0)
                cloud[k // 2 + 1] = (-a, 0, a)
    for b in all_zero:
        a = rng.uniform(0.5, 3.0, n).astype(np.float32)
        coarse[b] = np.stack([a, -a, np.zeros(n, np.float32)], 1)
        coarse[b, ::3] = 0
    reg_rot = reg_centre = None
    if regress:
        ang = boxes[:, 6].astype(np.float64) + rng.uniform(-0.4, 0.4, B)
        reg_rot = np.zeros((B, 3, 3), np.float32)
        for b in range(B):
            c, s = np.cos(ang[b]), np.sin(ang[b])
            reg_rot[b] = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]]) * rng.uniform(0.8, 1.2) + rng.uniform(-0.05, 0.05, (3, 3))
        reg_centre = (boxes[:, :3] + rng.uniform(-0.5, 0.5, (B, 3))).astype(np.float32)
        for i, j in tie:
            reg_rot[j] = reg_rot[i]
    case = dict(name=name, coarse=coarse + np.float32(0), complete=complete + np.float32(0), gt_boxes=boxes, reg_rot=reg_rot, reg_centre=reg_centre,
                num_pts=np.asarray(num_pts, np.int64))
    assert len(case["num_pts"]) == B
    return case


BORDERS17 = (4, 5, 30, 31, 80, 81, 200, 201, 12, 12, 50, 150, 150, 150, 3, 1000000, 1000001)


@functools.lru_cache(maxsize=None)
def cases():
    """The smallest shapes at which the kernels can go wrong: n in {1, 63, 64, 257}, m in {1, TILE - 1, TILE + 1, 2 TILE + 3}, B in {1, 2, 17}; every
    level border; groups of 0, 1 and more objects, even-sized ones; tied heading errors; zero-sum rows in one-object and larger groups; a one-object
    group stripped empty; duplicate rows and scalars; all inside / all outside; headings 0, +-pi/2, +-pi and arbitrary; null regressions."""
    return (
        make_case("b1_n1_m1", 1, 1, 1, (40,), 1),
        make_case("b1_n63_tile-1_zero_rows_null", 1, 63, TILE - 1, (5,), 2, regress=False, zero_rows=(0,)),
        make_case("b2_n64_tile+1_one_object_levels", 2, 64, TILE + 1, (250, 10), 3, zero_rows=(1,), quantum=0.125),
        make_case("b2_n64_tile+1_even_group_tied", 2, 64, TILE + 1, (30, 5), 4, tie=((0, 1),)),
        make_case("b1_n64_stripped_empty", 1, 64, TILE + 1, (81,), 5, all_zero=(0,)),
        make_case("b2_n257_inside_outside", 2, 257, TILE - 1, (201, 200), 6, where=("inside", "outside"), quantum=0.25),
        make_case("b17_n257_2tile+3_borders", 17, 257, 2 * TILE + 3, BORDERS17, 7, zero_rows=(1, 8, 9), tie=((11, 12), (12, 13)), quantum=0.0625),
        make_case("b17_n63_m1", 17, 63, 1, BORDERS17, 8, zero_rows=(0,)),
        make_case("b17_n1_tile+1_null", 17, 1, TILE + 1, BORDERS17[::-1], 9, regress=False),
    )


def face_gap(case):
    """the smallest distance of any coarse row of the case to any face plane of its ground-truth cuboid (float64)"""
    return min(float(inside_box(p, b)[1].min()) for p, b in zip(case["coarse"], case["gt_boxes"]))


def has_negative_zero(case):
    return any(bool((np.signbit(case[k]) & (case[k] == 0)).any()) for k in ("coarse", "complete"))


@functools.lru_cache(maxsize=None)
def expected(index):
    """(per-object quantities with their bounds, the 30 values the reference's way, the bound of each) of cases()[index], computed once"""
    case = cases()[index]
    t = per_object(case)
    t["tol_iou"] = iou_tolerance(case, t)
    _, tols = values30_from_objects(case, t)
    return t, values30(case), tols
