"""Plain numpy / Python restatement, in float64, of the reference's KITTI evaluation (detector3d/pcdet/datasets/kitti/kitti_object_eval_python:
eval.py and rotate_iou.py): the three overlaps, clean_data, the sequential compute_statistics_jit (both modes, kept as the LOOP, not the closed
form the pass-2 kernel uses), get_thresholds, eval_class and the result string.  It needs neither numba nor a GPU.

What is pinned to the reference and what is not
  tests/golden/kitti_eval.npz is produced by the reference's own eval.py (make_kitti_eval_golden.py).  It pins the matching, the thresholds,
  the AP arithmetic and the result string.  The overlap VALUES stay unpinned beyond fp32 rounding: numba would type rotate_iou.py's `area_val`
  as float64 while the fp32 kernel sums in fp32, and a device `cos` / `sin` differs from libm's.  The fixture keeps every compared overlap at
  least 1e-3 away from every min_overlap in use, so these differences never decide a match.

Where this departs from the reference's literal statements
  * quadrilateral_intersection stops adding points at CAP = 8 (the reference writes past its 16-float local array; the kernel must not);
  * rotate_iou_eval skips pairs whose circumscribed circles are apart: every test of the algorithm fails for them and the area is exactly 0;
  * compute_statistics_jit walks Python lists of the same float64 values (speed only), and sums `tmp` with np.sum as the golden run did
    (numba compiles that np.sum to a sequential loop; the two differ in the last bits, far inside the 1e-12 the similarity is held to).

Bound for an fp32 overlap against this float64 restatement (rotated_overlap_bound, image_overlap_bound)
  Both sides start from the same fp32 boxes (rotate_iou_gpu_eval casts first).  u = 2^-24, S = the largest |corner coordinate| of the pair, D = the
  larger box diagonal, L1, L2 = the lengths of two crossing edges.  First order in u, per pair, from the float64 polygon:
    corner vertex     c = fl(fl(fl(cos * cx) + fl(sin * cy)) + centre): sinf / cosf within 1 ulp (2 u) on factors <= D / 2, two products and one
                      sum at scale D / 2, the last sum rounds at scale S: per coordinate <= u (S + 4 D), as a vector e_c = sqrt(2) u (S + 4 D).
    crossing vertex   P = (Dx, Dy) / DH.  ABBA = A0 B1 - B0 A1 and CDDC are differences of products of size S^2: each is off by <= 2 u S^2 -- THE
                      dominant term, quadratic in the coordinate scale.  Dx = ABBA DC0 - BA0 CDDC inherits 2 u S^2 (|DC0| + |BA0|) plus three
                      roundings at u S L1 L2; DH = BA x DC has relative error <= 3 u, the quotient u; the moved corners move the true crossing by
                      <= e_c / sin(angle) each.  As a vector: e_x = (2 u S^2 (L1 + L2) + 3 sqrt(2) u S L1 L2 + 2 e_c L1 L2) / |DH| + 4 sqrt(2) u S,
                      written out in _crossing_error below.  A shallow crossing (small |DH|) is ill-conditioned and the bound says so.
    area              the fan's differences a - c cancel the scale S exactly (Sterbenz) or to u S, absorbed in e_c; moving vertex i by e_i changes
                      the polygon's area by <= |p(i+1) - p(i-1)| e_i / 2, so dA = sum_i |p(i+1) - p(i-1)| e_i / 2, plus 16 u A for the fan's own
                      products and sums.
    IoU               I / (A1 + A2 - I): d IoU / d I = (A1 + A2) / U^2 with U the union, plus 16 u for the last quotients.  Criterion 0 / 1: dA / A1 (A2);
                      criterion 2: dA.  3-D: the height overlap iw (error <= 4 u |y|) times the BEV area over the union volume, same chain.
  At S = 100 m the issue's rough 1e-4 is the 2 u S^2 / A term for a car seen square on; a pedestrian-sized box or a shallow crossing is several
  times worse, which is why the bound is evaluated per pair and not quoted as one number.  The bound assumes generic position: the fp32 and
  float64 runs see the same corners inside and the same edges crossing.  Pairs ON a test (identical boxes, a corner on an edge, touching edges)
  are exercised with binary-exact coordinates, where fp32 makes no rounding error at all, or carry a duplicate / collinear vertex, which adds no
  area.  image_overlap_bound: box sides are differences of pixel coordinates <= S, each off by <= u S (inputs exact): relative area error <=
  2 u S (1 / w + 1 / h) per box and for the intersection, IoU error <= 3 times the largest such term + 8 u.
  The fixture keeps every compared overlap at least max(FIXTURE_MARGIN, 4 x its own pair's bound) away from every min_overlap in use.
"""
import io as sysio
import math

import numpy as np

U32 = 2.0 ** -24
FIXTURE_MARGIN = 1e-3
CAP = 8                         # points of the intersection buffer; a candidate past it is dropped (the reference writes past its array)


def image_overlap_bound(box, qbox):
    """See the module header.  Boxes (x1, y1, x2, y2) in pixels."""
    box, qbox = np.asarray(box, dtype=np.float64), np.asarray(qbox, dtype=np.float64)
    S = max(np.abs(box).max(), np.abs(qbox).max())
    iw, ih = min(box[2], qbox[2]) - max(box[0], qbox[0]), min(box[3], qbox[3]) - max(box[1], qbox[1])
    if iw <= 0 or ih <= 0:
        return 8 * U32
    sides = [box[2] - box[0], box[3] - box[1], qbox[2] - qbox[0], qbox[3] - qbox[1], iw, ih]
    return 3 * 2 * U32 * S * 2 / min(sides) + 8 * U32


def _corners64(rbbox):
    c = np.zeros(8)
    rbbox_to_corners(c, np.asarray(rbbox, dtype=np.float64), np.float64)
    return c.reshape(4, 2)


def _crossing_error(A, B, C, D, S, e_c):
    """Vector error of the fp32 crossing point of segments AB and CD (module header, 'crossing vertex')."""
    BA, DC = B - A, D - C
    L1, L2 = np.hypot(*BA), np.hypot(*DC)
    DH = abs(BA[1] * DC[0] - BA[0] * DC[1])
    return (2 * U32 * S * S * (L1 + L2) + 3 * math.sqrt(2) * U32 * S * L1 * L2 + 2 * e_c * L1 * L2) / DH + 4 * math.sqrt(2) * U32 * S


def rotated_area_bound(rbox1, rbox2):
    """(bound on |fp32 - float64| of the intersection area, the float64 area) for one pair of (x, y, x_d, y_d, angle) boxes, generic position."""
    c1, c2 = _corners64(rbox1), _corners64(rbox2)
    S = max(np.abs(c1).max(), np.abs(c2).max())
    Dg = max(math.hypot(rbox1[2], rbox1[3]), math.hypot(rbox2[2], rbox2[3]))
    e_c = math.sqrt(2) * U32 * (S + 4 * Dg)
    pts = []
    for i in range(4):
        if point_in_quadrilateral(c1[i, 0], c1[i, 1], c2.reshape(-1), np.float64):
            pts.append((c1[i, 0], c1[i, 1], e_c))
        if point_in_quadrilateral(c2[i, 0], c2[i, 1], c1.reshape(-1), np.float64):
            pts.append((c2[i, 0], c2[i, 1], e_c))
    tmp = np.zeros(2)
    for i in range(4):
        for j in range(4):
            if line_segment_intersection(c1.reshape(-1), c2.reshape(-1), i, j, tmp, np.float64):
                pts.append((tmp[0], tmp[1], _crossing_error(c1[i], c1[(i + 1) % 4], c2[j], c2[(j + 1) % 4], S, e_c)))
    if len(pts) < 3:
        return 16 * U32 * Dg * Dg, 0.0
    p = np.array(pts)
    ctr = p[:, :2].mean(0)
    p = p[np.argsort(np.arctan2(p[:, 1] - ctr[1], p[:, 0] - ctr[0]), kind="stable")]
    n = len(p)
    A = 0.5 * abs(sum(p[i, 0] * p[(i + 1) % n, 1] - p[(i + 1) % n, 0] * p[i, 1] for i in range(n)))
    dA = sum(0.5 * np.hypot(*(p[(i + 1) % n, :2] - p[i - 1, :2])) * p[i, 2] for i in range(n))
    return dA + 16 * U32 * A, A


def rotated_overlap_bound(rbox1, rbox2, criterion=-1):
    """Bound on |kernel - restatement| of devRotateIoUEval(rbox1, rbox2, criterion); see the module header."""
    dA, A = rotated_area_bound(rbox1, rbox2)
    a1, a2 = rbox1[2] * rbox1[3], rbox2[2] * rbox2[3]
    if criterion == -1:
        U = a1 + a2 - A
        return dA * (a1 + a2) / (U * U) + 16 * U32
    if criterion == 0:
        return dA / a1 + 16 * U32
    if criterion == 1:
        return dA / a2 + 16 * U32
    return dA


def d3_overlap_bound(box, qbox, criterion=-1):
    """The same for d3_box_overlap of one pair of (x, y, z, l, h, w, ry) boxes."""
    box, qbox = np.asarray(box, dtype=np.float64), np.asarray(qbox, dtype=np.float64)
    dA, A = rotated_area_bound(qbox[[0, 2, 3, 5, 6]], box[[0, 2, 3, 5, 6]])
    iw = min(box[1], qbox[1]) - max(box[1] - box[4], qbox[1] - qbox[4])
    if iw <= 0 or A <= 0:
        return 16 * U32
    d_iw = 4 * U32 * max(abs(box[1]), abs(qbox[1]), abs(box[1] - box[4]), abs(qbox[1] - qbox[4]))
    v1, v2 = box[3] * box[4] * box[5], qbox[3] * qbox[4] * qbox[5]
    d_inc = iw * dA + d_iw * A
    if criterion == -1:
        U = v1 + v2 - iw * A
        return d_inc * (v1 + v2) / (U * U) + 16 * U32
    if criterion == 0:
        return d_inc / v1 + 16 * U32
    if criterion == 1:
        return d_inc / v2 + 16 * U32
    return 16 * U32                      # inc / inc


# ---------------------------------------------------------------------------------------------------------------------------------------
# rotate_iou.py, statement for statement; F is the float type every intermediate is rounded to (np.float64 here, np.float32 to predict the kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def trangle_area(a, b, c, F):
    return F(F(F(F(a[0] - c[0]) * F(b[1] - c[1])) - F(F(a[1] - c[1]) * F(b[0] - c[0]))) / F(2.0))


def area(int_pts, num_of_inter, F):
    area_val = F(0.0)
    for i in range(num_of_inter - 2):
        area_val = F(area_val + abs(trangle_area(int_pts[:2], int_pts[2 * i + 2:2 * i + 4], int_pts[2 * i + 4:2 * i + 6], F)))
    return area_val


def sort_vertex_in_convex_polygon(int_pts, num_of_inter, F):
    if num_of_inter > 0:
        center = np.zeros(2, dtype=F)
        for i in range(num_of_inter):
            center[0] = F(center[0] + int_pts[2 * i])
            center[1] = F(center[1] + int_pts[2 * i + 1])
        center[0] = F(center[0] / F(num_of_inter))
        center[1] = F(center[1] / F(num_of_inter))
        vs = np.zeros(16, dtype=F)
        for i in range(num_of_inter):
            v0 = F(int_pts[2 * i] - center[0])
            v1 = F(int_pts[2 * i + 1] - center[1])
            d = F(np.sqrt(F(F(v0 * v0) + F(v1 * v1))))
            with np.errstate(divide="ignore", invalid="ignore"):
                v0 = F(v0 / d)
                v1 = F(v1 / d)
            if v1 < 0:
                v0 = F(-2 - v0)
            vs[i] = v0
        for i in range(1, num_of_inter):
            if vs[i - 1] > vs[i]:
                temp = vs[i]
                tx = int_pts[2 * i]
                ty = int_pts[2 * i + 1]
                j = i
                while j > 0 and vs[j - 1] > temp:
                    vs[j] = vs[j - 1]
                    int_pts[j * 2] = int_pts[j * 2 - 2]
                    int_pts[j * 2 + 1] = int_pts[j * 2 - 1]
                    j -= 1
                vs[j] = temp
                int_pts[j * 2] = tx
                int_pts[j * 2 + 1] = ty


def line_segment_intersection(pts1, pts2, i, j, temp_pts, F):
    A0, A1 = pts1[2 * i], pts1[2 * i + 1]
    B0, B1 = pts1[2 * ((i + 1) % 4)], pts1[2 * ((i + 1) % 4) + 1]
    C0, C1 = pts2[2 * j], pts2[2 * j + 1]
    D0, D1 = pts2[2 * ((j + 1) % 4)], pts2[2 * ((j + 1) % 4) + 1]
    BA0, BA1 = F(B0 - A0), F(B1 - A1)
    DA0, CA0, DA1, CA1 = F(D0 - A0), F(C0 - A0), F(D1 - A1), F(C1 - A1)
    acd = F(DA1 * CA0) > F(CA1 * DA0)
    bcd = F(F(D1 - B1) * F(C0 - B0)) > F(F(C1 - B1) * F(D0 - B0))
    if acd != bcd:
        abc = F(CA1 * BA0) > F(BA1 * CA0)
        abd = F(DA1 * BA0) > F(BA1 * DA0)
        if abc != abd:
            DC0, DC1 = F(D0 - C0), F(D1 - C1)
            ABBA = F(F(A0 * B1) - F(B0 * A1))
            CDDC = F(F(C0 * D1) - F(D0 * C1))
            DH = F(F(BA1 * DC0) - F(BA0 * DC1))
            Dx = F(F(ABBA * DC0) - F(BA0 * CDDC))
            Dy = F(F(ABBA * DC1) - F(BA1 * CDDC))
            temp_pts[0] = F(Dx / DH)
            temp_pts[1] = F(Dy / DH)
            return True
    return False


def point_in_quadrilateral(pt_x, pt_y, corners, F):
    ab0, ab1 = F(corners[2] - corners[0]), F(corners[3] - corners[1])
    ad0, ad1 = F(corners[6] - corners[0]), F(corners[7] - corners[1])
    ap0, ap1 = F(pt_x - corners[0]), F(pt_y - corners[1])
    abab = F(F(ab0 * ab0) + F(ab1 * ab1))
    abap = F(F(ab0 * ap0) + F(ab1 * ap1))
    adad = F(F(ad0 * ad0) + F(ad1 * ad1))
    adap = F(F(ad0 * ap0) + F(ad1 * ap1))
    return abab >= abap and abap >= 0 and adad >= adap and adap >= 0


def quadrilateral_intersection(pts1, pts2, int_pts, F):
    num_of_inter = 0
    for i in range(4):
        if point_in_quadrilateral(pts1[2 * i], pts1[2 * i + 1], pts2, F) and num_of_inter < CAP:
            int_pts[num_of_inter * 2] = pts1[2 * i]
            int_pts[num_of_inter * 2 + 1] = pts1[2 * i + 1]
            num_of_inter += 1
        if point_in_quadrilateral(pts2[2 * i], pts2[2 * i + 1], pts1, F) and num_of_inter < CAP:
            int_pts[num_of_inter * 2] = pts2[2 * i]
            int_pts[num_of_inter * 2 + 1] = pts2[2 * i + 1]
            num_of_inter += 1
    temp_pts = np.zeros(2, dtype=F)
    for i in range(4):
        for j in range(4):
            if line_segment_intersection(pts1, pts2, i, j, temp_pts, F) and num_of_inter < CAP:
                int_pts[num_of_inter * 2] = temp_pts[0]
                int_pts[num_of_inter * 2 + 1] = temp_pts[1]
                num_of_inter += 1
    return num_of_inter


def rbbox_to_corners(corners, rbbox, F):
    angle = rbbox[4]
    a_cos = F(np.cos(angle))
    a_sin = F(np.sin(angle))
    center_x, center_y, x_d, y_d = rbbox[0], rbbox[1], rbbox[2], rbbox[3]
    corners_x = [F(-x_d / 2), F(-x_d / 2), F(x_d / 2), F(x_d / 2)]
    corners_y = [F(-y_d / 2), F(y_d / 2), F(y_d / 2), F(-y_d / 2)]
    for i in range(4):
        corners[2 * i] = F(F(F(a_cos * corners_x[i]) + F(a_sin * corners_y[i])) + center_x)
        corners[2 * i + 1] = F(F(F(-a_sin * corners_x[i]) + F(a_cos * corners_y[i])) + center_y)


def inter(rbbox1, rbbox2, F):
    corners1, corners2, intersection_corners = np.zeros(8, dtype=F), np.zeros(8, dtype=F), np.zeros(16, dtype=F)
    rbbox_to_corners(corners1, rbbox1, F)
    rbbox_to_corners(corners2, rbbox2, F)
    num_intersection = quadrilateral_intersection(corners1, corners2, intersection_corners, F)
    sort_vertex_in_convex_polygon(intersection_corners, num_intersection, F)
    return area(intersection_corners, num_intersection, F)


def devRotateIoUEval(rbox1, rbox2, criterion=-1, F=np.float64):
    rbox1, rbox2 = np.asarray(rbox1, dtype=F), np.asarray(rbox2, dtype=F)
    area1 = F(rbox1[2] * rbox1[3])
    area2 = F(rbox2[2] * rbox2[3])
    area_inter = inter(rbox1, rbox2, F)
    if criterion == -1:
        return F(area_inter / F(F(area1 + area2) - area_inter))
    elif criterion == 0:
        return F(area_inter / area1)
    elif criterion == 1:
        return F(area_inter / area2)
    return area_inter


def rotate_iou_eval(boxes, query_boxes, criterion=-1, F=np.float64):
    """(N, 5), (K, 5) -> (N, K): out[n, k] = devRotateIoUEval(query_boxes[k], boxes[n]) as rotate_iou_kernel_eval calls it."""
    boxes = np.asarray(boxes).astype(np.float32).astype(F).reshape(-1, 5)          # rotate_iou_gpu_eval casts to float32 first
    query_boxes = np.asarray(query_boxes).astype(np.float32).astype(F).reshape(-1, 5)
    out = np.zeros((len(boxes), len(query_boxes)), dtype=F)
    half_diag = lambda b: 0.5 * np.hypot(b[:, 2], b[:, 3])
    near = np.hypot(boxes[:, None, 0] - query_boxes[None, :, 0], boxes[:, None, 1] - query_boxes[None, :, 1]) <= 1.01 * (half_diag(boxes)[:, None] + half_diag(query_boxes)[None, :]) + 1e-3
    for n in range(len(boxes)):
        for k in range(len(query_boxes)):
            if near[n, k]:              # boxes whose circumscribed circles are apart share no point: every test fails, the area is exactly 0
                out[n, k] = devRotateIoUEval(query_boxes[k], boxes[n], criterion, F)
    return out


def image_box_overlap(boxes, query_boxes, criterion=-1):
    boxes, query_boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4), np.asarray(query_boxes, dtype=np.float64).reshape(-1, 4)
    N, K = boxes.shape[0], query_boxes.shape[0]
    overlaps = np.zeros((N, K))
    for k in range(K):
        qbox_area = ((query_boxes[k, 2] - query_boxes[k, 0]) * (query_boxes[k, 3] - query_boxes[k, 1]))
        for n in range(N):
            iw = (min(boxes[n, 2], query_boxes[k, 2]) - max(boxes[n, 0], query_boxes[k, 0]))
            if iw > 0:
                ih = (min(boxes[n, 3], query_boxes[k, 3]) - max(boxes[n, 1], query_boxes[k, 1]))
                if ih > 0:
                    if criterion == -1:
                        ua = ((boxes[n, 2] - boxes[n, 0]) * (boxes[n, 3] - boxes[n, 1]) + qbox_area - iw * ih)
                    elif criterion == 0:
                        ua = ((boxes[n, 2] - boxes[n, 0]) * (boxes[n, 3] - boxes[n, 1]))
                    elif criterion == 1:
                        ua = qbox_area
                    else:
                        ua = 1.0
                    overlaps[n, k] = iw * ih / ua
    return overlaps


def bev_box_overlap(boxes, qboxes, criterion=-1):
    return rotate_iou_eval(boxes, qboxes, criterion)


def d3_box_overlap(boxes, qboxes, criterion=-1):
    boxes, qboxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7), np.asarray(qboxes, dtype=np.float64).reshape(-1, 7)
    rinc = rotate_iou_eval(boxes[:, [0, 2, 3, 5, 6]], qboxes[:, [0, 2, 3, 5, 6]], 2)
    for i in range(boxes.shape[0]):
        for j in range(qboxes.shape[0]):
            if rinc[i, j] > 0:
                iw = (min(boxes[i, 1], qboxes[j, 1]) - max(boxes[i, 1] - boxes[i, 4], qboxes[j, 1] - qboxes[j, 4]))
                if iw > 0:
                    area1 = boxes[i, 3] * boxes[i, 4] * boxes[i, 5]
                    area2 = qboxes[j, 3] * qboxes[j, 4] * qboxes[j, 5]
                    inc = iw * rinc[i, j]
                    if criterion == -1:
                        ua = (area1 + area2 - inc)
                    elif criterion == 0:
                        ua = area1
                    elif criterion == 1:
                        ua = area2
                    else:
                        ua = inc
                    rinc[i, j] = inc / ua
                else:
                    rinc[i, j] = 0.0
    return rinc


def metric_boxes(anno, metric):
    """The columns calculate_iou_partly (eval.py:360-393) hands to each overlap, for one frame."""
    if metric == 0:
        return np.asarray(anno["bbox"], dtype=np.float64).reshape(-1, 4)
    loc, dims = np.asarray(anno["location"], dtype=np.float64).reshape(-1, 3), np.asarray(anno["dimensions"], dtype=np.float64).reshape(-1, 3)
    rots = np.asarray(anno["rotation_y"], dtype=np.float64).reshape(-1)
    if metric == 1:
        loc, dims = loc[:, [0, 2]], dims[:, [0, 2]]
    return np.concatenate([loc, dims, rots[..., np.newaxis]], axis=1)


OVERLAP_FN = {0: image_box_overlap, 1: bev_box_overlap, 2: d3_box_overlap}


def frame_overlaps(gt_annos, dt_annos, metric):
    """overlaps[i] of eval_class: (n_dt_i, n_gt_i), detections as rows (eval_class hands calculate_iou_partly the detections first)."""
    return [OVERLAP_FN[metric](metric_boxes(d, metric), metric_boxes(g, metric)) for g, d in zip(gt_annos, dt_annos)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# eval.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def get_thresholds(scores, num_gt, num_sample_pts=41):
    scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    current_recall = 0
    thresholds = []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        if i < (len(scores) - 1):
            r_recall = (i + 2) / num_gt
        else:
            r_recall = l_recall
        if (((r_recall - current_recall) < (current_recall - l_recall)) and (i < (len(scores) - 1))):
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def clean_data(gt_anno, dt_anno, current_class, difficulty):
    CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'truck']
    MIN_HEIGHT = [40, 25, 25]
    MAX_OCCLUSION = [0, 1, 2]
    MAX_TRUNCATION = [0.15, 0.3, 0.5]
    dc_bboxes, ignored_gt, ignored_dt = [], [], []
    current_cls_name = CLASS_NAMES[current_class].lower()
    num_gt = len(gt_anno["name"])
    num_dt = len(dt_anno["name"])
    num_valid_gt = 0
    for i in range(num_gt):
        bbox = gt_anno["bbox"][i]
        gt_name = gt_anno["name"][i].lower()
        height = bbox[3] - bbox[1]
        valid_class = -1
        if (gt_name == current_cls_name):
            valid_class = 1
        elif (current_cls_name == "Pedestrian".lower() and "Person_sitting".lower() == gt_name):
            valid_class = 0
        elif (current_cls_name == "Car".lower() and "Van".lower() == gt_name):
            valid_class = 0
        else:
            valid_class = -1
        ignore = False
        if ((gt_anno["occluded"][i] > MAX_OCCLUSION[difficulty]) or (gt_anno["truncated"][i] > MAX_TRUNCATION[difficulty])
                or (height <= MIN_HEIGHT[difficulty])):
            ignore = True
        if valid_class == 1 and not ignore:
            ignored_gt.append(0)
            num_valid_gt += 1
        elif (valid_class == 0 or (ignore and (valid_class == 1))):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if gt_anno["name"][i] == "DontCare":
            dc_bboxes.append(gt_anno["bbox"][i])
    for i in range(num_dt):
        if (dt_anno["name"][i].lower() == current_cls_name):
            valid_class = 1
        else:
            valid_class = -1
        height = abs(dt_anno["bbox"][i, 3] - dt_anno["bbox"][i, 1])
        if height < MIN_HEIGHT[difficulty]:
            ignored_dt.append(1)
        elif valid_class == 1:
            ignored_dt.append(0)
        else:
            ignored_dt.append(-1)
    return num_valid_gt, ignored_gt, ignored_dt, dc_bboxes


def compute_statistics_jit(overlaps, gt_datas, dt_datas, ignored_gt, ignored_det, dc_bboxes, metric, min_overlap, thresh=0, compute_fp=False,
                           compute_aos=False, compared=None):
    """The sequential loop.  `compared`, when a list, collects every overlap value the loop compares with min_overlap (for the fixture's margin check)."""
    det_size = dt_datas.shape[0]
    gt_size = gt_datas.shape[0]
    dt_bboxes = dt_datas[:, :4]
    # plain Python lists of Python floats: the same float64 values and the same statements, several times faster than numpy scalar indexing
    dt_scores = dt_datas[:, -1].tolist()
    dt_alphas = dt_datas[:, 4].tolist()
    gt_alphas = gt_datas[:, 4].tolist()
    ignored_gt, ignored_det = np.asarray(ignored_gt).tolist(), np.asarray(ignored_det).tolist()
    overlaps = np.asarray(overlaps, dtype=np.float64).reshape(det_size, gt_size).T.tolist()          # overlaps[i][j]: ground truth i, detection j
    min_overlap, thresh = float(min_overlap), float(thresh)

    assigned_detection = [False] * det_size
    ignored_threshold = [False] * det_size
    if compute_fp:
        for i in range(det_size):
            if (dt_scores[i] < thresh):
                ignored_threshold[i] = True
    NO_DETECTION = -10000000
    tp, fp, fn, similarity = 0, 0, 0, 0
    thresholds = np.zeros((gt_size, ))
    thresh_idx = 0
    delta = np.zeros((gt_size, ))
    delta_idx = 0
    for i in range(gt_size):
        if ignored_gt[i] == -1:
            continue
        det_idx = -1
        valid_detection = NO_DETECTION
        max_overlap = 0
        assigned_ignored_det = False

        for j in range(det_size):
            if (ignored_det[j] == -1):
                continue
            if (assigned_detection[j]):
                continue
            if (ignored_threshold[j]):
                continue
            overlap = overlaps[i][j]
            dt_score = dt_scores[j]
            if compared is not None:
                compared.append(overlap)
            if (not compute_fp and (overlap > min_overlap) and dt_score > valid_detection):
                det_idx = j
                valid_detection = dt_score
            elif (compute_fp and (overlap > min_overlap) and (overlap > max_overlap or assigned_ignored_det) and ignored_det[j] == 0):
                max_overlap = overlap
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = False
            elif (compute_fp and (overlap > min_overlap) and (valid_detection == NO_DETECTION) and ignored_det[j] == 1):
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = True

        if (valid_detection == NO_DETECTION) and ignored_gt[i] == 0:
            fn += 1
        elif ((valid_detection != NO_DETECTION) and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1)):
            assigned_detection[det_idx] = True
        elif valid_detection != NO_DETECTION:
            tp += 1
            thresholds[thresh_idx] = dt_scores[det_idx]
            thresh_idx += 1
            if compute_aos:
                delta[delta_idx] = gt_alphas[i] - dt_alphas[det_idx]
                delta_idx += 1
            assigned_detection[det_idx] = True
    if compute_fp:
        for i in range(det_size):
            if (not (assigned_detection[i] or ignored_det[i] == -1 or ignored_det[i] == 1 or ignored_threshold[i])):
                fp += 1
        nstuff = 0
        if metric == 0:
            overlaps_dt_dc = image_box_overlap(dt_bboxes, dc_bboxes, 0)
            for i in range(dc_bboxes.shape[0]):
                for j in range(det_size):
                    if (assigned_detection[j]):
                        continue
                    if (ignored_det[j] == -1 or ignored_det[j] == 1):
                        continue
                    if (ignored_threshold[j]):
                        continue
                    if compared is not None:
                        compared.append(overlaps_dt_dc[j, i])
                    if overlaps_dt_dc[j, i] > min_overlap:
                        assigned_detection[j] = True
                        nstuff += 1
        fp -= nstuff
        if compute_aos:
            tmp = np.zeros((fp + delta_idx, ))
            for i in range(delta_idx):
                tmp[i + fp] = (1.0 + np.cos(delta[i])) / 2.0
            if tp > 0 or fp > 0:
                similarity = np.sum(tmp)
            else:
                similarity = -1
    return tp, fp, fn, similarity, thresholds[:thresh_idx]


def _prepare_data(gt_annos, dt_annos, current_class, difficulty):
    gt_datas_list, dt_datas_list, ignored_gts, ignored_dets, dontcares = [], [], [], [], []
    total_num_valid_gt = 0
    for i in range(len(gt_annos)):
        num_valid_gt, ignored_gt, ignored_det, dc_bboxes = clean_data(gt_annos[i], dt_annos[i], current_class, difficulty)
        ignored_gts.append(np.array(ignored_gt, dtype=np.int64))
        ignored_dets.append(np.array(ignored_det, dtype=np.int64))
        dc_bboxes = np.zeros((0, 4)) if len(dc_bboxes) == 0 else np.stack(dc_bboxes, 0).astype(np.float64)
        dontcares.append(dc_bboxes)
        total_num_valid_gt += num_valid_gt
        gt_datas_list.append(np.concatenate([np.asarray(gt_annos[i]["bbox"], dtype=np.float64).reshape(-1, 4),
                                             np.asarray(gt_annos[i]["alpha"], dtype=np.float64)[..., np.newaxis]], 1))
        dt_datas_list.append(np.concatenate([np.asarray(dt_annos[i]["bbox"], dtype=np.float64).reshape(-1, 4),
                                             np.asarray(dt_annos[i]["alpha"], dtype=np.float64)[..., np.newaxis],
                                             np.asarray(dt_annos[i]["score"], dtype=np.float64)[..., np.newaxis]], 1))
    return gt_datas_list, dt_datas_list, ignored_gts, ignored_dets, dontcares, total_num_valid_gt


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, overlaps=None, detail=None, compared=None):
    """eval.py:448-553 with the per-frame overlaps (the diagonal blocks its parts are sliced into).  `overlaps`: use these blocks (the kernel's
    own, read back) in place of the float64 restatement's.  `detail`, when a dict, receives per combination (m, l, k) the true-positive scores in
    frame order, the thresholds and the (thresholds, 4) pr table."""
    assert len(gt_annos) == len(dt_annos)
    if overlaps is None:
        overlaps = frame_overlaps(gt_annos, dt_annos, metric)
    N_SAMPLE_PTS = 41
    num_minoverlap, num_class, num_difficulty = len(min_overlaps), len(current_classes), len(difficultys)
    precision = np.zeros([num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS])
    recall = np.zeros([num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS])
    aos = np.zeros([num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS])
    for m, current_class in enumerate(current_classes):
        for l, difficulty in enumerate(difficultys):
            gt_datas_list, dt_datas_list, ignored_gts, ignored_dets, dontcares, total_num_valid_gt = _prepare_data(gt_annos, dt_annos, current_class,
                                                                                                                   difficulty)
            for k, min_overlap in enumerate(min_overlaps[:, metric, m]):
                thresholdss = []
                for i in range(len(gt_annos)):
                    rets = compute_statistics_jit(overlaps[i], gt_datas_list[i], dt_datas_list[i], ignored_gts[i], ignored_dets[i], dontcares[i], metric,
                                                  min_overlap=min_overlap, thresh=0.0, compute_fp=False, compared=compared)
                    thresholdss += rets[4].tolist()
                thresholdss = np.array(thresholdss)
                thresholds = np.array(get_thresholds(thresholdss, total_num_valid_gt))
                pr = np.zeros([len(thresholds), 4])
                for i in range(len(gt_annos)):
                    for t, thresh in enumerate(thresholds):
                        tp, fp, fn, similarity, _ = compute_statistics_jit(overlaps[i], gt_datas_list[i], dt_datas_list[i], ignored_gts[i], ignored_dets[i],
                                                                           dontcares[i], metric, min_overlap=min_overlap, thresh=thresh, compute_fp=True,
                                                                           compute_aos=compute_aos, compared=compared)
                        pr[t, 0] += tp
                        pr[t, 1] += fp
                        pr[t, 2] += fn
                        if similarity != -1:
                            pr[t, 3] += similarity
                if detail is not None:
                    detail[(m, l, k)] = dict(tp_scores=thresholdss, thresholds=thresholds, pr=pr.copy())
                with np.errstate(divide="ignore", invalid="ignore"):
                    for i in range(len(thresholds)):
                        recall[m, l, k, i] = pr[i, 0] / (pr[i, 0] + pr[i, 2])
                        precision[m, l, k, i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
                        if compute_aos:
                            aos[m, l, k, i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
                for i in range(len(thresholds)):
                    precision[m, l, k, i] = np.max(precision[m, l, k, i:], axis=-1)
                    recall[m, l, k, i] = np.max(recall[m, l, k, i:], axis=-1)
                    if compute_aos:
                        aos[m, l, k, i] = np.max(aos[m, l, k, i:], axis=-1)
    return {"recall": recall, "precision": precision, "orientation": aos}


def get_mAP(prec):
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def get_mAP_R40(prec):
    sums = 0
    for i in range(1, prec.shape[-1]):
        sums = sums + prec[..., i]
    return sums / 40 * 100


def print_str(value, *arg, sstream=None):
    if sstream is None:
        sstream = sysio.StringIO()
    sstream.truncate(0)
    sstream.seek(0)
    print(value, *arg, file=sstream)
    return sstream.getvalue()


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, PR_detail_dict=None, overlaps=None):
    """`overlaps`: {metric: per-frame blocks}, computed once by the caller and shared between evaluations of the same annotations."""
    difficultys = [0, 1, 2]
    ov = overlaps or {}
    ret = eval_class(gt_annos, dt_annos, current_classes, difficultys, 0, min_overlaps, compute_aos, overlaps=ov.get(0))
    mAP_bbox = get_mAP(ret["precision"])
    mAP_bbox_R40 = get_mAP_R40(ret["precision"])
    if PR_detail_dict is not None:
        PR_detail_dict['bbox'] = ret['precision']
    mAP_aos = mAP_aos_R40 = None
    if compute_aos:
        mAP_aos = get_mAP(ret["orientation"])
        mAP_aos_R40 = get_mAP_R40(ret["orientation"])
        if PR_detail_dict is not None:
            PR_detail_dict['aos'] = ret['orientation']
    ret = eval_class(gt_annos, dt_annos, current_classes, difficultys, 1, min_overlaps, overlaps=ov.get(1))
    mAP_bev = get_mAP(ret["precision"])
    mAP_bev_R40 = get_mAP_R40(ret["precision"])
    if PR_detail_dict is not None:
        PR_detail_dict['bev'] = ret['precision']
    ret = eval_class(gt_annos, dt_annos, current_classes, difficultys, 2, min_overlaps, overlaps=ov.get(2))
    mAP_3d = get_mAP(ret["precision"])
    mAP_3d_R40 = get_mAP_R40(ret["precision"])
    if PR_detail_dict is not None:
        PR_detail_dict['3d'] = ret['precision']
    return mAP_bbox, mAP_bev, mAP_3d, mAP_aos, mAP_bbox_R40, mAP_bev_R40, mAP_3d_R40, mAP_aos_R40


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None, overlaps=None):
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])
    min_overlaps = np.stack([overlap_0_7, overlap_0_5], axis=0)
    class_to_name = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck'}
    name_to_class = {v: n for n, v in class_to_name.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    current_classes = [name_to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = min_overlaps[:, :, current_classes]
    result = ''
    compute_aos = False
    for anno in dt_annos:
        if anno['alpha'].shape[0] != 0:
            if anno['alpha'][0] != -10:
                compute_aos = True
            break
    mAPbbox, mAPbev, mAP3d, mAPaos, mAPbbox_R40, mAPbev_R40, mAP3d_R40, mAPaos_R40 = do_eval(
        gt_annos, dt_annos, current_classes, min_overlaps, compute_aos, PR_detail_dict=PR_detail_dict, overlaps=overlaps)
    ret_dict = {}
    for j, curcls in enumerate(current_classes):
        for i in range(min_overlaps.shape[0]):
            result += print_str((f"{class_to_name[curcls]} " "AP@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j])))
            result += print_str((f"bbox AP:{mAPbbox[j, 0, i]:.4f}, " f"{mAPbbox[j, 1, i]:.4f}, " f"{mAPbbox[j, 2, i]:.4f}"))
            result += print_str((f"bev  AP:{mAPbev[j, 0, i]:.4f}, " f"{mAPbev[j, 1, i]:.4f}, " f"{mAPbev[j, 2, i]:.4f}"))
            result += print_str((f"3d   AP:{mAP3d[j, 0, i]:.4f}, " f"{mAP3d[j, 1, i]:.4f}, " f"{mAP3d[j, 2, i]:.4f}"))
            if compute_aos:
                result += print_str((f"aos  AP:{mAPaos[j, 0, i]:.2f}, " f"{mAPaos[j, 1, i]:.2f}, " f"{mAPaos[j, 2, i]:.2f}"))
            result += print_str((f"{class_to_name[curcls]} " "AP_R40@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j])))
            result += print_str((f"bbox AP:{mAPbbox_R40[j, 0, i]:.4f}, " f"{mAPbbox_R40[j, 1, i]:.4f}, " f"{mAPbbox_R40[j, 2, i]:.4f}"))
            result += print_str((f"bev  AP:{mAPbev_R40[j, 0, i]:.4f}, " f"{mAPbev_R40[j, 1, i]:.4f}, " f"{mAPbev_R40[j, 2, i]:.4f}"))
            result += print_str((f"3d   AP:{mAP3d_R40[j, 0, i]:.4f}, " f"{mAP3d_R40[j, 1, i]:.4f}, " f"{mAP3d_R40[j, 2, i]:.4f}"))
            if compute_aos:
                result += print_str((f"aos  AP:{mAPaos_R40[j, 0, i]:.2f}, " f"{mAPaos_R40[j, 1, i]:.2f}, " f"{mAPaos_R40[j, 2, i]:.2f}"))
                if i == 0:
                    ret_dict['%s_aos/easy_R40' % class_to_name[curcls]] = mAPaos_R40[j, 0, 0]
                    ret_dict['%s_aos/moderate_R40' % class_to_name[curcls]] = mAPaos_R40[j, 1, 0]
                    ret_dict['%s_aos/hard_R40' % class_to_name[curcls]] = mAPaos_R40[j, 2, 0]
            if i == 0:
                ret_dict['%s_3d/easy_R40' % class_to_name[curcls]] = mAP3d_R40[j, 0, 0]
                ret_dict['%s_3d/moderate_R40' % class_to_name[curcls]] = mAP3d_R40[j, 1, 0]
                ret_dict['%s_3d/hard_R40' % class_to_name[curcls]] = mAP3d_R40[j, 2, 0]
                ret_dict['%s_bev/easy_R40' % class_to_name[curcls]] = mAPbev_R40[j, 0, 0]
                ret_dict['%s_bev/moderate_R40' % class_to_name[curcls]] = mAPbev_R40[j, 1, 0]
                ret_dict['%s_bev/hard_R40' % class_to_name[curcls]] = mAPbev_R40[j, 2, 0]
                ret_dict['%s_image/easy_R40' % class_to_name[curcls]] = mAPbbox_R40[j, 0, 0]
                ret_dict['%s_image/moderate_R40' % class_to_name[curcls]] = mAPbbox_R40[j, 1, 0]
                ret_dict['%s_image/hard_R40' % class_to_name[curcls]] = mAPbbox_R40[j, 2, 0]
    return result, ret_dict
