"""Rotated IoU / NMS / points-in-boxes: C oracle vs an independent polygon clipper (CPU); HIP vs oracle (GPU)."""
import numpy as np
import pytest
import torch

import box_reference as br
from box_reference import _clip_area, _corners, rand_boxes as _rand_boxes
from oracle import boxes as ob, pool_ops as opo


def test_oracle_overlap_vs_polygon_clipping_and_known_answer():
    rng = np.random.default_rng(0)
    a, b = _rand_boxes(rng, 40, 6.0), _rand_boxes(rng, 30, 6.0)
    ov = ob.boxes_overlap_bev(a, b)
    for i in range(len(a)):
        for j in range(len(b)):
            ref = _clip_area(_corners(a[i].astype(np.float64)), _corners(b[j].astype(np.float64)))
            # the reference counts corners within 1e-2 of the other box as inside: allow margin * perimeter
            assert abs(ov[i, j] - ref) <= 5e-4 + 0.02 * (a[i, 3] + a[i, 4] + b[j, 3] + b[j, 4]) * (ref < 0.5) + 1e-3 * ref, (i, j, ov[i, j], ref)
    # value the reference's own compiled iou3d_cpu.cpp returned in the survey session (0.4421)
    hand = np.array([[0, 0, 0, 4, 2, 1.5, 0], [1, 0.5, 0, 4, 2, 1.5, 0.3]], np.float32)
    iou = ob.boxes_iou_bev(hand, hand)
    assert abs(iou[0, 0] - 1) < 1e-6 and abs(iou[1, 0] - 0.4421) < 1e-4


def test_oracle_nms_and_points_in_boxes():
    rng = np.random.default_rng(1)
    b = _rand_boxes(rng, 200, 8.0)
    keep = ob.nms(b, 0.1)
    iou = ob.boxes_iou_bev(b[keep], b[keep])
    np.fill_diagonal(iou, 0)
    assert (iou <= 0.1 + 1e-6).all() and keep[0] == 0
    pts = rng.uniform(-10, 10, (2, 500, 3)).astype(np.float32)
    pts[:, :, 2] *= 0.2
    boxes = np.stack([_rand_boxes(rng, 12, 8.0), _rand_boxes(rng, 12, 8.0)])
    idx = ob.points_in_boxes(pts, boxes)
    assert idx.min() == -1 and idx.max() < 12 and (idx >= 0).sum() > 5


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_hip_overlap_iou_iou3d(cuda, hip_lib):
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils as u
    rng = np.random.default_rng(2)
    a, b = _rand_boxes(rng, 300, 12.0), _rand_boxes(rng, 77, 12.0)
    b[:5] = a[:5]                                     # identical boxes
    b[5, :] = a[5, :]; b[5, 0] += a[5, 3]             # touching along x (axis-aligned after rotation)
    ta, tb = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
    np.testing.assert_allclose(u.boxes_overlap_bev(ta, tb).cpu().numpy(), ob.boxes_overlap_bev(a, b), rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(u.boxes_iou_bev(ta, tb).cpu().numpy(), ob.boxes_iou_bev(a, b), rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(u.boxes_iou3d_gpu(ta, tb).cpu().numpy(), ob.boxes_iou3d(a, b), rtol=1e-3, atol=1e-4)
    # the one-launch 3-D IoU == the reference's chain of torch ops around the overlap kernel, bit for bit; batched over scenes, rows of 8 floats
    fused = u.boxes_iou3d_gpu(ta, tb)
    saved, u.FUSED_IOU3D = u.FUSED_IOU3D, False
    try:
        assert torch.equal(fused, u.boxes_iou3d_gpu(ta, tb))
    finally:
        u.FUSED_IOU3D = saved
    b8 = torch.cat([tb, torch.full((len(b), 1), 3.0, device=cuda)], dim=1)                  # ground-truth layout: a class column behind the box
    both = u.boxes_iou3d_batch(torch.stack([ta, ta.flip(0)]), torch.stack([b8, b8.flip(0)]))
    assert torch.equal(both[0], fused) and torch.equal(both[1], fused.flip(0).flip(1))
    assert u.boxes_iou3d_gpu(ta[:0], tb).shape == (0, 77) and u.boxes_iou3d_batch(ta[None], b8[None, :0]).shape == (1, 300, 0)
    assert u.boxes_iou_bev(ta[:0], tb).shape == (0, 77)
    cpu = u.boxes_iou_bev_cpu(a, b)                                   # numpy in / numpy out, like the reference's CPU entry point
    assert isinstance(cpu, np.ndarray) and np.array_equal(cpu, u.boxes_iou_bev(ta, tb).cpu().numpy())
    assert isinstance(u.boxes_iou_bev_cpu(torch.from_numpy(a), torch.from_numpy(b)), torch.Tensor)
    with pytest.raises(AssertionError):
        u.boxes_iou_bev_cpu(ta, tb)


@pytest.mark.gpu
@pytest.mark.parametrize("n,thr", [(50, 0.1), (700, 0.7), (4096, 0.8), (9000, 0.8)])
def test_hip_nms_matches_oracle(cuda, hip_lib, n, thr):
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils as u
    rng = np.random.default_rng(n)
    b = _rand_boxes(rng, n, 30.0)
    b[: n // 3, 0:2] = b[n // 3: 2 * (n // 3), 0:2][: n // 3] + rng.normal(0, 0.3, (n // 3, 2))   # clusters of near-duplicates
    s = rng.uniform(size=n).astype(np.float32)
    order = np.argsort(-s, kind="stable")
    keep, _ = u.nms_gpu(torch.from_numpy(b).to(cuda), torch.from_numpy(s).to(cuda), thr)
    ref = order[ob.nms(b[order], thr)]
    got = keep.cpu().numpy()
    # scores are distinct with probability 1, so the sort order is unambiguous
    assert np.array_equal(got, ref)
    keep_n, _ = u.nms_normal_gpu(torch.from_numpy(b).to(cuda), torch.from_numpy(s).to(cuda), thr)
    assert np.array_equal(keep_n.cpu().numpy(), order[ob.nms(b[order], thr, normal=True)])
    kp, _ = u.nms_gpu(torch.from_numpy(b).to(cuda), torch.from_numpy(s).to(cuda), thr, pre_maxsize=min(n, 512))
    assert np.array_equal(kp.cpu().numpy(), order[:512][ob.nms(b[order[:512]], thr)])
    # max_keep: the sweep stops early and returns exactly the prefix (what NMS_POST_MAXSIZE callers slice off anyway)
    for mk in (1, 37, 64, 65, len(ref), len(ref) + 10):
        km, _ = u.nms_gpu(torch.from_numpy(b).to(cuda), torch.from_numpy(s).to(cuda), thr, max_keep=mk)
        assert np.array_equal(km.cpu().numpy(), ref[:mk]), mk


@pytest.mark.gpu
def test_hip_points_in_boxes(cuda, hip_lib):
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as r
    rng = np.random.default_rng(3)
    pts = rng.uniform(-12, 12, (3, 5000, 3)).astype(np.float32)
    pts[:, :, 2] *= 0.15
    boxes = np.stack([_rand_boxes(rng, 40, 10.0) for _ in range(3)])
    boxes[2, 20:] = 0                                   # zero-padded boxes (gt_boxes padding)
    out = r.points_in_boxes_gpu(torch.from_numpy(pts).to(cuda), torch.from_numpy(boxes).to(cuda)).cpu().numpy()
    assert np.array_equal(out, ob.points_in_boxes(pts, boxes))


# ------------------------------------------------------------------------------------------ edges: float64 references (box_reference.py)
def _check_bev(case, overlap, iou, k, log):
    """Everything a BEV overlap / IoU result of one all-pairs call is held to.  Returns (failure messages, excluded (na,nb) bool): pairs that
    oracle_unstable flags or that the ORACLE leaves outside the float64 sandwich -- both known before `overlap` is looked at."""
    fails = []
    ov, io = np.asarray(overlap, np.float64), np.asarray(iou, np.float64)
    if not (np.isfinite(ov).all() and np.isfinite(io).all()):
        return ["%s: not finite" % case.name], np.zeros(ov.shape, bool)
    if (ov < 0).any():
        fails.append("%s: negative overlap %g" % (case.name, ov.min()))
    for what, got in (("overlap", ov), ("iou", io)):
        for why, sel in (("zero padding row", case.padding), ("bounding circles apart", case.apart)):
            if (got[sel] != 0).any():
                fails.append("%s: %s not exactly 0 for %d pairs (%s)" % (case.name, what, (got[sel] != 0).sum(), why))
    if case.name == "identical":
        worst = np.abs(np.diagonal(io) - 1).max()
        log.append("%-22s |IoU(box, copy) - 1| <= %.3g" % (case.name, worst))
        if worst > 1e-6:
            fails.append("%s: IoU of a box with its copy off 1 by %g" % (case.name, worst))
    oracle_out = case.sandwich_misses(case.overlap, br.K_ORACLE_MEASURED)
    tie = case.name == "margin_tie"                                     # 1-ulp nudges decide the corner count there: the sandwich only
    excluded = oracle_out if tie else oracle_out | case.unstable_overlap | case.unstable_iou
    if not tie:
        for what, got, ref, unstable, tol in (("overlap", ov, case.overlap, case.unstable_overlap, br.OVERLAP_TOL),
                                              ("iou", io, case.iou, case.unstable_iou, br.IOU_TOL)):
            err = np.abs(got - ref) / tol(ref.astype(np.float64))
            err[unstable] = 0
            log.append("%-22s %-7s vs oracle: worst error / tolerance %.3g" % (case.name, what, err.max()))
            if err.max() > 1:
                i, j = np.unravel_index(err.argmax(), err.shape)
                fails.append("%s: %s[%d,%d] = %r, oracle %r (%d pairs beyond tolerance)" % (case.name, what, i, j, got[i, j], ref[i, j], (err > 1).sum()))
    miss = case.sandwich_misses(ov, k) & ~oracle_out
    log.append("%-22s overlap vs float64: off the band worst |got - exact| / unit %.3g (allowed %.3g), in the band %d pairs" %
               (case.name, case.worst_ratio(ov), k, case.band.sum()))
    if miss.any():
        i, j = np.argwhere(miss)[0]
        fails.append("%s: overlap[%d,%d] = %r outside [%r, %r] +- %g (%d pairs)" % (case.name, i, j, ov[i, j], case.exact[i, j],
                                                                                    case.grown[i, j] if case.band[i, j] else case.exact[i, j], k * case.unit[i, j], miss.sum()))
    # IoU follows from the overlap: inside the same float64 bounds pushed through so / (sa + sb - so)
    s = k * case.unit
    lo, hi = np.clip(case.exact - s, 0, None), np.where(case.band, case.grown, case.exact) + s
    union_lo = np.clip(case.area_a + case.area_b - hi, 1e-8, None)
    union_hi = np.clip(case.area_a + case.area_b - lo, 1e-8, None)
    bad = ((io < lo / union_hi * (1 - 8 * br.EPS32) - 1e-7) | (io > hi / union_lo * (1 + 8 * br.EPS32) + 1e-7)) & ~oracle_out & (case.area_a + case.area_b - hi > 0)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        fails.append("%s: iou[%d,%d] = %r outside its float64 bounds [%r, %r] (%d pairs)" % (case.name, i, j, io[i, j], (lo / union_hi)[i, j], (hi / union_lo)[i, j], bad.sum()))
    return fails, excluded


def _check_caps(cases, excluded):
    fails, total, out = [], 0, 0
    for case, ex in zip(cases, excluded):
        total, out = total + ex.size, out + int(ex.sum())
        if case.paired and np.diagonal(ex).mean() > br.CAP_FAMILY_DIAGONAL:
            fails.append("%s: %d of %d paired entries excluded" % (case.name, np.diagonal(ex).sum(), len(case.a)))
    if out > br.CAP_ALL_PAIRS * total:
        fails.append("%d of %d pairs excluded" % (out, total))
    return fails


def test_clip_area_closed_forms():
    sq = lambda x, y, dx, dy, rz=0.0: np.array([x, y, 0, dx, dy, 1, rz], np.float32)
    assert br.clip_area(sq(0, 0, 4, 2), sq(1, 0.5, 4, 2)) == 3 * 1.5                          # axis-aligned: product of the interval overlaps
    assert br.clip_area(sq(0, 0, 4, 2), sq(4, 0, 4, 2)) == 0 and br.clip_area(sq(0, 0, 4, 2), sq(9, 0, 4, 2)) == 0
    assert br.clip_area(sq(0, 0, 4, 2), sq(0.5, 0.25, 1, 0.5)) == 0.5                          # nested
    assert br.clip_area(sq(0, 0, 4, 2), sq(4, 0, 4, 2), grow=0.25) == 0.5 * 2.5               # grown on every side
    assert abs(br.clip_area(sq(0, 0, 2, 2), sq(0, 0, 1, 1, np.pi / 4)) - 1) < 1e-12            # unit square turned 45 degrees inside a 2 x 2 square
    assert abs(br.clip_area(sq(0, 0, 1, 1), sq(0, 0, 1, 1, np.pi / 4)) - (2 * np.sqrt(2) - 2)) < 1e-7   # ... and against a unit square: a regular octagon
    assert br.clip_area(sq(0, 0, 0, 0), sq(0, 0, 4, 2)) == 0 and br.clip_area(sq(0, 0, 4, 2), sq(0, 0, 0, 0)) == 0
    rng = np.random.default_rng(7)
    a, b = _rand_boxes(rng, 30, 4.0), _rand_boxes(rng, 30, 4.0)                                # the vectorised clipper == the plain one
    plain = [_clip_area(_corners(x.astype(np.float64)), _corners(y.astype(np.float64))) for x, y in zip(a, b)]
    assert np.abs(br.clip_area(a, b) - plain).max() < 1e-12 and max(plain) > 1
    assert np.array_equal(np.diagonal(br.clip_area_pairs(a, b)), br.clip_area(a, b))
    assert br.corner_band(sq(0, 0, 4, 2), sq(4, 0, 4, 2)) and br.corner_band(sq(0, 0, 4, 2), sq(4.0101, 0, 4, 2))
    assert not br.corner_band(sq(0, 0, 4, 2), sq(4.0102, 0, 4, 2)) and not br.corner_band(sq(0, 0, 4, 2), sq(1, 0.5, 4, 2))


def test_oracle_meets_every_bound_on_the_edge_families():
    """The oracle in the kernel's place: the chosen inputs keep the reference algorithm inside its caps, and K_ORACLE_MEASURED is what it says."""
    cases = br.family_cases() + br.shape_cases()
    assert len(br.family_cases()) == 18 and all(len(c.a) == br.FAMILY_N for c in br.family_cases())
    log, fails, excluded = [], [], []
    for case in cases:
        f, ex = _check_bev(case, case.overlap, case.iou, br.K_ORACLE_MEASURED, log)
        fails += f
        excluded.append(ex)
        a3, b3 = br.set_heights(case.a, case.b)
        ref = br.iou3d_reference(a3, b3, case.overlap)
        assert np.abs(ob.boxes_iou3d(a3, b3) - ref).max() <= 1e-5
        if case.paired:
            m = np.arange(len(a3)) % 4
            assert (np.diagonal(ref)[m == 1] == 0).all() and (np.diagonal(ref)[m == 3] == 0).all()      # touching in z, dz = 0
    print("\n".join(log))
    fails += _check_caps(cases, excluded)
    assert not fails, "\n".join(fails)
    worst = max(c.worst_ratio(c.overlap) for c in cases)
    assert 0.9 * br.K_ORACLE_MEASURED <= worst <= br.K_ORACLE_MEASURED, worst


def test_oracle_nms_closed_forms():
    for n in (1, 2, 63, 64, 65, 129, 1026):
        boxes, keepers = br.nms_clusters(n)
        assert np.array_equal(ob.nms(boxes, 0.5), keepers) and np.array_equal(ob.nms(boxes, 0.5, normal=True), keepers)
        boxes, keepers = br.nms_chain(n)
        assert np.array_equal(ob.nms(boxes, 0.2), keepers) and np.array_equal(ob.nms(boxes, 0.2, normal=True), keepers)
    boxes, keepers = br.nms_clusters(3073)
    assert keepers.tolist() == [0, 63, 64, 65, 1023, 1024, 1025, 3071, 3072] and (boxes[3009:3071] == boxes[0]).all()
    assert br.nms_max_keeps(keepers, 3073) == [None, 1, 5, 6, 8, 9, 19]
    assert br.nms_max_keeps(br.nms_chain(3073)[1], 3073) == [None, 1, 512, 513, 1536, 1537, 1547]


def _point_scenes():
    """(name, margin, points (M,3), boxes (T,7)) of the heading-0 scenes that float32 decides exactly"""
    out = []
    for margin in (1e-5, 1e-2):
        out.append(("faces", margin, br.exact_face_points(margin), br.EXACT_BOXES))
        for name, boxes in br.FIRST_BOX_SCENES.items():
            out.append((name, margin, br.first_box_points(margin), boxes))
    return out


def test_in_box_truth_and_the_oracle_on_decidable_points():
    b = np.array([[0, 0, 0, 4, 2, 2, 0.0]], np.float32)                                       # hand cases (test_boundary.py's, and the z rule)
    p = np.array([[-1.9, -0.9, -0.9], [2.005, 0, 0], [2.02, 0, 0], [0, 0, 1], [0, 0, 1.0000001], [5, 0, 0]], np.float32)
    assert br.in_box_truth(p, b, 1e-2)[0].tolist() == [0, 0, -1, 0, -1, -1] and br.in_box_truth(p, b, 1e-5)[0].tolist() == [0, -1, -1, 0, -1, -1]
    assert abs(br.in_box_truth(p, b, 1e-2)[1][1] - (2 + float(np.float32(1e-2)) - float(p[1, 0]))) < 1e-15
    for name, margin, pts, boxes in _point_scenes():
        assert br.exact_or_far(pts, boxes, margin).all(), (name, margin)
        truth, _ = br.in_box_truth(pts, boxes, margin)
        assert (truth >= 0).any() and (truth < 0).any()
        if margin == 1e-5:
            assert np.array_equal(ob.points_in_boxes(pts[None], boxes[None])[0], truth), name
        else:
            want = np.stack([br.in_box_truth(pts, boxes[k:k + 1], margin)[0] == 0 for k in range(len(boxes))]).astype(np.int32)
            assert np.array_equal(opo.points_in_boxes_cpu(pts, boxes), want), name
    truth, _ = br.in_box_truth(br.exact_face_points(1e-5), br.EXACT_BOXES, 1e-5)
    assert 0.3 < (truth >= 0).mean() < 0.7       # both sides of the surfaces
    assert br.in_box_truth(br.first_box_points(1e-5), br.FIRST_BOX_SCENES["padding_first"], 1e-5)[0][:5].tolist() == [0, 3, 3, 3, 0]
    assert br.in_box_truth(br.first_box_points(1e-5), br.FIRST_BOX_SCENES["duplicates"], 1e-5)[0][6] == 0
    for margin in (1e-5, 1e-2):                                                               # general headings: at most 1 % undecidable
        rng = np.random.default_rng(11)
        pts, boxes = br.general_scene(rng, 24, 4000, margin)
        truth, dist = br.in_box_truth(pts, boxes, margin)
        near = dist <= br.decision_delta(pts, boxes)
        assert near.mean() <= 0.01 and (dist < 1.1e-3).mean() > 0.4 and 0.2 < (truth >= 0).mean() < 0.8, (near.mean(), (truth >= 0).mean())
        if margin == 1e-5:
            assert np.array_equal(ob.points_in_boxes(pts[None], boxes[None])[0][~near], truth[~near])


# ------------------------------------------------------------------------------------------ GPU: the kernels at those edges
@pytest.mark.gpu
def test_hip_bev_overlap_iou_edge_families(cuda, hip_lib):
    """k_boxes_pairs / overlap_area against the C oracle (stable pairs), against float64 (rounding bound off the corner band, sandwich inside)
    and the exact properties, on the 18 families (130 x 130 all-pairs calls) and the tile-edge shapes."""
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils as u
    cases = br.family_cases() + br.shape_cases()
    log, fails, excluded = [], [], []
    for case in cases:
        ta, tb = torch.from_numpy(case.a).to(cuda), torch.from_numpy(case.b).to(cuda)
        f, ex = _check_bev(case, u.boxes_overlap_bev(ta, tb).cpu().numpy(), u.boxes_iou_bev(ta, tb).cpu().numpy(), br.K_KERNEL, log)
        fails += f
        excluded.append(ex)
    print("\n".join(log))
    fails += _check_caps(cases, excluded)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_hip_iou3d_edge_families_and_heights(cuda, hip_lib):
    """k_boxes_iou3d on the same boxes with equal / touching / nested / zero heights: against the oracle's BEV overlap with heights and volumes in
    float64 (stable pairs); fused == unfused chain and batched == per scene, bit for bit."""
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils as u
    log, fails = [], []
    for case in br.family_cases() + br.shape_cases():
        a3, b3 = br.set_heights(case.a, case.b)
        ta, tb = torch.from_numpy(a3).to(cuda), torch.from_numpy(b3).to(cuda)
        fused = u.boxes_iou3d_gpu(ta, tb)
        got = fused.cpu().numpy().astype(np.float64)
        if not np.isfinite(got).all() or (got < 0).any():
            fails.append("%s: not finite or negative" % case.name)
            continue
        if case.name != "margin_tie":
            ref = br.iou3d_reference(a3, b3, case.overlap)
            err = np.abs(got - ref) / (1e-4 + 1e-3 * np.abs(ref))
            err[case.unstable_overlap | case.unstable_iou | case.sandwich_misses(case.overlap, br.K_ORACLE_MEASURED)] = 0
            log.append("%-22s iou3d vs oracle overlap + float64 heights: worst error / tolerance %.3g" % (case.name, err.max()))
            if err.max() > 1:
                i, j = np.unravel_index(err.argmax(), err.shape)
                fails.append("%s: iou3d[%d,%d] = %r, reference %r (%d pairs beyond tolerance)" % (case.name, i, j, got[i, j], ref[i, j], (err > 1).sum()))
        if case.paired:
            m = np.arange(len(a3)) % 4
            if (np.diagonal(got)[(m == 1) | (m == 3)] != 0).any():
                fails.append("%s: touching in z or dz = 0 not exactly 0" % case.name)
        if (got[case.padding] != 0).any() or (got[case.apart] != 0).any():
            fails.append("%s: zero padding row or far pair not exactly 0" % case.name)
        saved, u.FUSED_IOU3D = u.FUSED_IOU3D, False
        try:
            if not torch.equal(fused, u.boxes_iou3d_gpu(ta, tb)):
                fails.append("%s: fused launch != unfused chain" % case.name)
        finally:
            u.FUSED_IOU3D = saved
        b8 = torch.cat([tb, torch.full((len(b3), 1), 3.0, device=cuda)], dim=1)
        both = u.boxes_iou3d_batch(torch.stack([ta, ta.flip(0)]), torch.stack([b8, b8.flip(0)]))
        if not (torch.equal(both[0], fused) and torch.equal(both[1], u.boxes_iou3d_gpu(ta.flip(0), tb.flip(0)))):
            fails.append("%s: stacked scenes != per-scene calls" % case.name)
    print("\n".join(log))
    assert not fails, "\n".join(fails)


def _nms_inputs(kind, n):
    """(boxes in input order, scores, boxes in score order, expected keep list as input indices, ... as sorted positions, threshold)"""
    sorted_boxes, keepers = br.nms_clusters(n) if kind == "clusters" else br.nms_chain(n)
    perm = np.random.default_rng(n).permutation(n)                   # sorted position i sits at input row perm[i]
    boxes, scores = np.zeros_like(sorted_boxes), np.zeros(n, np.float32)
    boxes[perm] = sorted_boxes
    scores[perm] = np.linspace(0.99, 0.01, n, dtype=np.float32) if n > 1 else np.float32(0.5)
    assert len(np.unique(scores)) == n
    return boxes, scores, sorted_boxes, perm[keepers], keepers, 0.5 if kind == "clusters" else 0.2


NMS_SIZES = (1, 2, 63, 64, 65, 128, 129, 2048, 2049, 3073)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NMS_SIZES)
def test_hip_nms_closed_forms(cuda, hip_lib, n):
    """k_nms_mask / k_nms_sweep on inputs whose keep list is known in closed form, at the block, path and chunk edges, every call twice on the
    same workspace; max_keep reached in the first, second and third chunk of a chunked sweep."""
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils as u
    for kind in ("clusters", "chain"):
        boxes, scores, _, want, keepers, thr = _nms_inputs(kind, n)
        tb, ts = torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda)
        for fn in (u.nms_gpu, u.nms_normal_gpu):
            mks = br.nms_max_keeps(keepers, n)
            for mk in mks + [1, None]:                                # ... and a call that stops early right before a full sweep
                for _ in range(2):
                    got = fn(tb, ts, thr, max_keep=mk)[0].cpu().numpy()
                    assert np.array_equal(got, want[:mk]), (kind, fn.__name__, mk, got[:12], want[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("n", (65, 129))
def test_hip_nms_mask_words_closed_form(cuda, hip_lib, n):
    """k_nms_mask by itself: the words on and right of the diagonal, read back from the workspace, against the closed form -- bit (row, col) is
    set iff col > row and both are the same cluster (neighbours of the chain).  The sweep cannot tell a set bit on the diagonal from a clear one
    (it looks at a row's word only after keeping the row), so no keep list shows whether the ballot stops at col > row."""
    from seevcn_amd import _lib
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils as u
    cb = (n + 63) // 64
    for kind in ("clusters", "chain"):
        boxes, thr = (br.nms_clusters(n)[0], 0.5) if kind == "clusters" else (br.nms_chain(n)[0], 0.2)
        same = (boxes[:, None, :] == boxes[None, :, :]).all(2) if kind == "clusters" else np.abs(np.arange(n)[:, None] - np.arange(n)[None]) == 1
        bits = same & (np.arange(n)[None] > np.arange(n)[:, None])
        want = np.zeros((n, cb), np.uint64)
        for c in range(n):
            want[:, c // 64] |= bits[:, c].astype(np.uint64) << np.uint64(c % 64)
        tb, ts = torch.from_numpy(boxes).to(cuda), torch.linspace(0.99, 0.01, n, device=cuda)          # already in score order
        for fn in (u.nms_gpu, u.nms_normal_gpu):
            fn(tb, ts, thr)
            scratch = _lib.workspace.scratch("nms", hip_lib.sv_nms_scratch_bytes(n), cuda)
            got = scratch[:n * cb * 8].cpu().numpy().view(np.uint64).reshape(n, cb)
            for rb in range(cb):
                rows = slice(rb * 64, min(n, rb * 64 + 64))
                assert np.array_equal(got[rows, rb:], want[rows, rb:]), (kind, fn.__name__, rb)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NMS_SIZES)
def test_hip_nms_padded_closed_forms(cuda, hip_lib, n):
    """nms_gpu_padded (the route of every RoI head's proposal layer): slots below, equal to and above the survivors, sorted and unsorted input."""
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils as u
    for kind in ("clusters", "chain"):
        boxes, scores, sorted_boxes, want, keepers, thr = _nms_inputs(kind, n)
        k = len(keepers)
        for presorted, b, s, expect in ((False, boxes, scores, want), (True, sorted_boxes, -np.sort(-scores), keepers)):
            tb, ts = torch.from_numpy(b).to(cuda), torch.from_numpy(s).to(cuda)
            for slots in sorted({max(k - 1, 1), k, k + 5, n + 3}):
                for normal in (False, True):
                    for _ in range(2):
                        idx, valid = u.nms_gpu_padded(tb, ts, thr, slots, normal=normal, presorted=presorted)
                        assert idx.shape == (slots,) and idx.dtype == torch.int64 and valid.shape == (slots,) and valid.dtype == torch.bool
                        full = np.zeros(slots, np.int64)
                        full[:min(k, slots)] = expect[:slots]
                        assert np.array_equal(valid.cpu().numpy(), np.arange(slots) < k), (kind, presorted, slots, normal)
                        assert np.array_equal(idx.cpu().numpy(), full), (kind, presorted, slots, normal)
        if n >= 129:                                                  # pre_maxsize: only the first rows of the sorted order take part
            pre = n - 64
            idx, valid = u.nms_gpu_padded(torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda), thr, k + 2, pre_maxsize=pre)
            kp = int((keepers < pre).sum())
            assert np.array_equal(valid.cpu().numpy(), np.arange(k + 2) < kp) and np.array_equal(idx.cpu().numpy()[:kp], want[:kp]) and not idx[kp:].any()


@pytest.mark.gpu
def test_hip_nms_padded_empty_and_class_agnostic(cuda, hip_lib):
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils as u
    from seevcn_amd.pcdet.models.model_utils import model_nms_utils as m
    for presorted in (False, True):
        idx, valid = u.nms_gpu_padded(torch.zeros((0, 7), device=cuda), torch.zeros((0,), device=cuda), 0.5, 6, presorted=presorted)
        assert idx.tolist() == [0] * 6 and valid.tolist() == [False] * 6
    for n in (65, 2049, 3073):
        boxes, scores, _, want, keepers, thr = _nms_inputs("clusters", n)
        tb, ts = torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda)
        for pre in (4096, n - 1):
            kp = int((keepers < pre).sum())
            for post in (kp - 1, kp, kp + 5):
                cfg = {"NMS_TYPE": "nms_gpu", "NMS_THRESH": thr, "NMS_PRE_MAXSIZE": pre, "NMS_POST_MAXSIZE": post}
                for _ in range(2):
                    sel, sel_scores = m.class_agnostic_nms(ts, tb, cfg)
                    psel, valid = m.class_agnostic_nms_padded(ts, tb, cfg)
                    assert np.array_equal(sel.cpu().numpy(), want[:min(kp, post)]) and torch.equal(sel_scores, ts[sel])
                    assert psel.shape == (post,) and valid.tolist() == [i < kp for i in range(post)]
                    assert torch.equal(psel[valid], sel)
    z, v = m.class_agnostic_nms_padded(torch.zeros((0,), device=cuda), torch.zeros((0, 7), device=cuda), {"NMS_TYPE": "nms_gpu", "NMS_THRESH": 0.5,
                                                                                                           "NMS_PRE_MAXSIZE": 9, "NMS_POST_MAXSIZE": 4})
    assert z.tolist() == [0] * 4 and v.tolist() == [False] * 4


def _hip_in_boxes(r, cuda, pts, boxes, margin):
    """first containing box (margin 1e-5: points_in_boxes_gpu) or the (N, M) matrix (margin 1e-2: points_in_boxes_cpu) of one scene"""
    if margin == 1e-5:
        return r.points_in_boxes_gpu(torch.from_numpy(pts[None]).to(cuda), torch.from_numpy(boxes[None]).to(cuda)).cpu().numpy()[0]
    return r.points_in_boxes_cpu(pts, boxes)


@pytest.mark.gpu
def test_hip_points_in_boxes_on_the_faces_and_first_box(cuda, hip_lib):
    """Heading 0, exact float32 differences: k_points_in_boxes (margin 1e-5) and k_points_in_boxes_matrix (1e-2) must equal the float64 truth bit
    for bit on and one float32 step beside every face; nested / duplicated / zero-padding boxes decide which box is first."""
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as r
    for name, margin, pts, boxes in _point_scenes():
        if margin == 1e-5:
            assert np.array_equal(_hip_in_boxes(r, cuda, pts, boxes, margin), br.in_box_truth(pts, boxes, margin)[0]), (name, margin)
        else:
            want = np.stack([br.in_box_truth(pts, boxes[k:k + 1], margin)[0] == 0 for k in range(len(boxes))]).astype(np.int32)
            assert np.array_equal(_hip_in_boxes(r, cuda, pts, boxes, margin), want), (name, margin)


@pytest.mark.gpu
def test_hip_points_in_boxes_general_headings(cuda, hip_lib):
    """Any heading (pi/2, pi, 7.5 pi among them), half of the points within 1e-3 of a face: equal to the float64 truth wherever the point is
    further than 64 eps32 (1 + max|coordinate|) from every decision surface."""
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as r
    rng = np.random.default_rng(11)
    pts, boxes = br.general_scene(rng, 24, 4000, 1e-5)
    truth, dist = br.in_box_truth(pts, boxes, 1e-5)
    far = dist > br.decision_delta(pts, boxes)
    got = _hip_in_boxes(r, cuda, pts, boxes, 1e-5)
    print("first-box test: %d of %d points decidable, %d of the others differ" % (far.sum(), len(far), (got != truth)[~far].sum()))
    assert np.array_equal(got[far], truth[far]), np.flatnonzero((got != truth) & far)[:10]
    rng = np.random.default_rng(11)
    pts, boxes = br.general_scene(rng, 9, 1500, 1e-2)
    for nb in (1, 9):
        got = _hip_in_boxes(r, cuda, pts, boxes[:nb], 1e-2)
        for k in range(nb):
            inside, dist = br.in_box_truth(pts, boxes[k:k + 1], 1e-2)
            far = dist > br.decision_delta(pts, boxes)
            assert np.array_equal(got[k][far], (inside == 0)[far].astype(np.int32)), (nb, k)


@pytest.mark.gpu
def test_hip_points_in_boxes_shapes_and_box_limit(cuda, hip_lib):
    """M on either side of the 256-point block, B = 1 and 3, T = 0, 1 and 2048 (the documented limit of the LDS staging); T = 2049 is refused."""
    from seevcn_amd.pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as r
    from seevcn_amd import _lib
    rng = np.random.default_rng(12)
    for t in (0, 1, 2048):
        scenes = [br.grid_scene(rng, t, 257) for _ in range(3)]
        pts, boxes = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]).reshape(3, t, 7)
        truth = np.stack([br.in_box_truth(p, b, 1e-5)[0] for p, b in scenes])
        far = np.stack([br.in_box_truth(p, b, 1e-5)[1] > br.decision_delta(p, b) for p, b in scenes])
        assert far.mean() >= 0.99 and (t == 0 or ((truth == t - 1).sum(1) >= 40).all())              # the last staged box is hit in every scene
        for nb in (1, 3):
            for m in (1, 255, 256, 257):
                got = r.points_in_boxes_gpu(torch.from_numpy(pts[:nb, :m]).to(cuda), torch.from_numpy(boxes[:nb]).to(cuda)).cpu().numpy()
                assert got.shape == (nb, m) and np.array_equal(got[far[:nb, :m]], truth[:nb, :m][far[:nb, :m]]), (t, nb, m)
    with pytest.raises(_lib.SeevcnHipError, match="2048"):
        r.points_in_boxes_gpu(torch.zeros((1, 4, 3), device=cuda), torch.zeros((1, 2049, 7), device=cuda))
