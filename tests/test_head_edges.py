"""The dense-head kernels of csrc/head.hip at their edges (k_anchor_decode, k_assign, k_center_targets, k_sigmoid_focal, k_weighted_smooth_l1)
against the references of head_reference.py: discrete results equal the fp32 spec bit for bit, float results lie within 4 K_REF eps32 scale of
float64.  The kernels are called the way the modules call them; the C entries directly where a module cannot express the case (anchor layouts
with a set owning two slots, the box-count limits)."""
import copy
import types

import numpy as np
import pytest
import torch

import head_reference as hr
from seevcn_amd.pcdet import model_cfgs as C

pytestmark = pytest.mark.gpu
F = np.float32


def _t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ------------------------------------------------------------------------------------------------ target assignment
def _assign_raw(hip_lib, cuda, case, gt=None):
    """one call into sentinel-filled buffers -> (rc, labels, targets, weights) as device tensors"""
    import seevcn_amd._lib as L
    gt = _t(case.gt if gt is None else gt, cuda)
    B, G, A = gt.shape[0], gt.shape[1], len(case.anchors)
    anchors, offs, cls = _t(case.anchors, cuda), _t(case.offs, cuda), _t(case.set_class, cuda)
    mthr, uthr = _t(case.mthr, cuda), _t(case.uthr, cuda)
    labels = torch.full((B, A), -9, dtype=torch.int32, device=cuda)
    targets = torch.full((B, A, 7 + case.sincos + case.E), float("nan"), device=cuda)
    weights = torch.full((B, A), float("nan"), device=cuda)
    scratch = torch.full((max(B * G, 1),), float("nan"), device=cuda)
    gp = L.ptr(gt) if G else None
    if case.coded:
        rc = hip_lib.sv_assign_targets_axis_aligned_coded(L.ptr(anchors), A, case.E, case.sincos, case.set_major, case.per_loc, len(case.set_class), L.ptr(offs),
                                                          L.ptr(cls), L.ptr(mthr), L.ptr(uthr), gp, B, G, L.ptr(scratch), L.ptr(labels), L.ptr(targets),
                                                          L.ptr(weights), L.stream())
    else:
        rc = hip_lib.sv_assign_targets_axis_aligned(L.ptr(anchors), A, case.per_loc, len(case.set_class), L.ptr(offs), L.ptr(cls), L.ptr(mthr), L.ptr(uthr), gp,
                                                    B, G, L.ptr(scratch), L.ptr(labels), L.ptr(targets), L.ptr(weights), L.stream())
    torch.cuda.synchronize()
    return rc, labels, targets, weights


def _assign_twice(hip_lib, cuda, case):
    """two calls into fresh buffers: bit-identical (the atomics are maxima)"""
    import seevcn_amd._lib as L
    runs = []
    for _ in range(2):
        rc, labels, targets, weights = _assign_raw(hip_lib, cuda, case)
        L.check(rc, "sv_assign_targets_axis_aligned" + ("_coded" if case.coded else ""))
        runs.append((labels.cpu().numpy(), targets.cpu().numpy(), weights.cpu().numpy()))
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), case.name + ": two calls differ"
    return runs[0]


def _assign_module(cuda, case):
    """the hand-built scene through AxisAlignedTargetAssigner.assign_targets: one (1, 1, n, 1, 1, width) anchor tensor per set"""
    from seevcn_amd.pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner
    S = len(case.set_class)
    names = ["k%d" % c for c in range(1, 8)]                                    # k7: a class without anchors
    cfg = dict(ANCHOR_GENERATOR_CONFIG=[dict(class_name=names[int(c) - 1], matched_threshold=float(m), unmatched_threshold=float(u))
                                        for c, m, u in zip(case.set_class, case.mthr, case.uthr)],
               TARGET_ASSIGNER_CONFIG=dict(), USE_MULTIHEAD=bool(case.set_major))
    coder = types.SimpleNamespace(encode_angle_by_sincos=bool(case.sincos))
    assigner = AxisAlignedTargetAssigner(cfg, names, coder)
    if case.set_major:
        runs = [case.anchors[case.offs[s]:case.offs[s + 1]] for s in range(S)]
    else:
        runs = [case.anchors.reshape(-1, S, case.anchors.shape[1])[:, s] for s in range(S)]
    pad = np.zeros((1, case.sincos), F)                                         # a sin/cos coder's anchors carry one zero column more than a box
    all_anchors = [_t(np.concatenate([r, np.repeat(pad, len(r), 0)], 1).reshape(1, 1, len(r), 1, 1, -1), cuda) for r in runs]
    out = assigner.assign_targets(all_anchors, _t(case.gt, cuda))
    return out["box_cls_labels"].cpu().numpy(), out["box_reg_targets"].cpu().numpy(), out["reg_weights"].cpu().numpy()


def test_assign_dyadic_families_equal_the_fp32_spec_and_float64(cuda, hip_lib):
    """Every dyadic call (the hand-built scene in both layouts, the shapes A x B x G of both entries), each run twice: labels and reg_weights equal
    the fp32 spec and -- off the three members whose IoU (3/5, 9/20, 7/20) rounds onto a threshold of the configs, where fp32 rules -- the float64
    evaluation; the matched box shows in the targets (ties: the first row's box, whose z differs from the later ones')."""
    fails, worst = [], 0.0
    for case in hr.assign_cases():
        labels, targets, weights = _assign_twice(hip_lib, cuda, case)
        f, w = case.check(labels, targets, weights, hr.K_KERNEL["encode"])
        fails += f
        worst = max(worst, w)
        lab64 = case.spec64[0]
        skip = hr.dyadic_f64_exceptions(case) if case.expect else np.zeros_like(lab64, bool)
        if ((labels != lab64) & ~skip).any():
            fails.append("%s: %d labels differ from the float64 evaluation" % (case.name, int(((labels != lab64) & ~skip).sum())))
        for (b, a), (lab, row) in case.expect.items():                          # the hand-derived members, named one by one
            if labels[b, a] != lab:
                fails.append("%s: anchor %d: label %d, derived by hand %d" % (case.name, a, labels[b, a], lab))
        if case.expect:
            lm, tm, wm = _assign_module(cuda, case)
            if not (np.array_equal(lm, labels) and np.array_equal(tm.view(np.int32), targets.view(np.int32)) and np.array_equal(wm, weights)):
                fails.append("%s: AxisAlignedTargetAssigner and the C entry differ" % case.name)
    print("assignment, dyadic families (%d calls): worst target error / (eps32 scale) = %.3g of %.3g" % (len(hr.assign_cases()), worst, hr.K_KERNEL["encode"]))
    assert not fails, "\n".join(fails)


def test_assign_refuses_more_boxes_than_the_limit_and_leaves_the_outputs_alone(cuda, hip_lib):
    import seevcn_amd._lib as L
    for coded, limit in ((False, 128), (True, 256)):
        case = hr.dyadic_random("limit", 257, 1, limit, 400, coded=coded, E=2 if coded else 0)
        _, labels, _, _ = _assign_raw(hip_lib, cuda, case)                      # at the limit: accepted
        assert np.array_equal(labels.cpu().numpy(), case.spec["labels"])
        over = np.concatenate([case.gt, case.gt[:, :1]], axis=1)
        rc, labels, targets, weights = _assign_raw(hip_lib, cuda, case, gt=over)
        with pytest.raises(L.SeevcnHipError, match="at most %d" % limit):
            L.check(rc, "assign")
        assert bool((labels == -9).all()) and bool(torch.isnan(targets).all()) and bool(torch.isnan(weights).all())


def test_assign_random_family_labels_by_margin_and_targets_within_the_bound(cuda, hip_lib):
    """Arbitrary fp32 boxes: labels equal the float64 decision wherever the float64 IoU is farther than 8 eps32 IoU from the thresholds and from
    the runner-up (at most 1 % of the anchors are not), and the fp32 spec everywhere; targets within the bound of the float64 encode."""
    case = hr.random_assign_case()
    labels, targets, weights = _assign_twice(hip_lib, cuda, case)
    decided = hr.decided_by_margin(case)
    assert (~decided).mean() <= hr.UNDECIDED_CAP
    assert np.array_equal(labels[decided], case.spec64[0][decided])
    fails, worst = case.check(labels, targets, weights, hr.K_KERNEL["encode"])
    print("assignment, random family: %d positives, %.3g %% undecided by the margin, worst target error / (eps32 scale) = %.3g of %.3g" %
          (int((labels > 0).sum()), 100 * (~decided).mean(), worst, hr.K_KERNEL["encode"]))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ decode
def _decode(cuda, case):
    """through AnchorHeadTemplate.generate_predicted_boxes on a stand-in for the head: its anchors, config and coder flags"""
    from seevcn_amd.pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
    anchors = _t(case.anchors, cuda)
    stub = types.SimpleNamespace(model_cfg=dict(NUM_DIR_BINS=case.num_bins, DIR_OFFSET=case.dir_offset, DIR_LIMIT_OFFSET=case.dir_limit_offset),
                                 _anchors_on=lambda device: anchors, _coded=case.coded, _sincos=case.sincos, use_multihead=False)
    B, A = case.enc.shape[:2]
    cls = torch.zeros((B, A, 1), device=cuda)
    dirs = None if case.dir_logits is None else _t(case.dir_logits, cuda)
    _, out = AnchorHeadTemplate.generate_predicted_boxes(stub, B, cls, _t(case.enc, cuda), dirs)
    return out.cpu().numpy()


def test_decode_bins_boundaries_codes_and_shapes(cuda, hip_lib):
    """Direction bins 1, 2, 3, 4 and 9 with headings on the floor's edge (the fp32 spec chooses the period count, float64 on that branch is the
    value), tied logits, no logits, the sin/cos code in every quadrant, on the axes and at (0, 0), extras, zero-size anchors, |t| up to 10,
    B * A of 1, 255 and 257."""
    fails, worst = [], 0.0
    for case in hr.decode_cases():
        f, w = case.check(_decode(cuda, case), hr.K_KERNEL["decode"])
        fails += f
        worst = max(worst, w if np.isfinite(w) else 1e30)
    print("decode (%d calls): worst error / (eps32 scale) = %.3g of %.3g" % (len(hr.decode_cases()), worst, hr.K_KERNEL["decode"]))
    assert not fails, "\n".join(fails)


def test_decode_grid_stride_loop(cuda, hip_lib):
    case = hr.stride_decode_case()
    assert case.enc.shape[0] * case.enc.shape[1] == 524288 + 300
    fails, worst = case.check(_decode(cuda, case), hr.K_KERNEL["decode"])
    print("decode, 524588 elements: worst error / (eps32 scale) = %.3g of %.3g" % (worst, hr.K_KERNEL["decode"]))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ centre targets
def _center(cuda, case):
    """through CenterHead.assign_targets, twice: bit-identical"""
    from seevcn_amd.pcdet.models import dense_heads
    cfg = copy.deepcopy(C.CENTER_HEAD)
    cfg["CLASS_NAMES_EACH_HEAD"] = case.each_head
    cfg["TARGET_ASSIGNER_CONFIG"] = dict(FEATURE_MAP_STRIDE=case.stride, NUM_MAX_OBJS=case.num_max_objs, GAUSSIAN_OVERLAP=case.overlap, MIN_RADIUS=case.min_radius)
    head = dense_heads.__all__["CenterHead"](model_cfg=cfg, input_channels=8, num_class=len(case.class_names), class_names=case.class_names,
                                             grid_size=np.array([case.W * case.stride, case.H * case.stride, 40]),
                                             point_cloud_range=np.array(case.pc_range, np.float32), voxel_size=case.voxel, predict_boxes_when_training=False)
    runs = []
    for _ in range(2):
        td = head.assign_targets(_t(case.gt, cuda), feature_map_size=(case.H, case.W))
        runs.append({k: [x.cpu().numpy() for x in td[k]] for k in ("heatmaps", "target_boxes", "inds", "masks")})
    for k in runs[0]:
        for a, b in zip(runs[0][k], runs[1][k]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: two calls differ in %s" % (case.name, k)
    return runs[0]


def _run_center(cuda, cases):
    fails, worst, worst_ulp = [], 0.0, 0.0
    for c in cases:
        for case in (c, c.swapped()):
            f, w, u = case.check(_center(cuda, case), hr.K_KERNEL["center_boxes"])
            fails += f
            worst, worst_ulp = max(worst, w), max(worst_ulp, u)
    return fails, worst, worst_ulp


def test_center_targets_ranking_slots_centres_and_windows(cuda, hip_lib):
    """Non-square map (24 x 40, voxel_x != voxel_y) and the same with x and y exchanged: classes interleaved over three heads with 63 .. 600 boxes,
    num_max_objs 5 and 500, a dx = 0 box in the middle, box_dim 8 and 10, one head with one class, no boxes; centres on cell corners, at 0, at
    W - 0.5 and outside on every side; windows clipped at every border; two radii on one cell; two classes on one cell."""
    cases = [c for c in hr.center_cases() if not c.name.startswith("radius family")]
    fails, worst, ulp = _run_center(cuda, cases)
    print("centre targets (%d calls): worst target_boxes error / (eps32 scale) = %.3g of %.3g, heat map within %.3g ulp of the float64 Gaussian" %
          (2 * len(cases), worst, hr.K_KERNEL["center_boxes"], ulp))
    assert not fails, "\n".join(fails)


def test_center_targets_radius_family(cuda, hip_lib):
    """Sizes within 3 ulps of those at which the radius is an integer 2 .. 12 (overlap 0.1, 0.5, 0.7).  Every box is a class of its own, so its
    Gaussian has a heat-map channel to itself, compared cell by cell with the oracle's at the integer radius of the fp32 chain in the reference's
    operation order; test_head_reference.py shows that a radius one off changes the channel of every single member."""
    cases = [c for c in hr.center_cases() if c.name.startswith("radius family")]
    assert sum(c.gt.shape[1] for c in cases) >= 200
    fails, worst, ulp = _run_center(cuda, cases)
    print("centre targets, radius family (%d sizes): worst target_boxes error / (eps32 scale) = %.3g, heat map within %.3g ulp" %
          (sum(c.gt.shape[1] for c in cases), worst, ulp))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ losses
def _loss(cuda, case):
    """value and gradient through the loss modules of loss_utils (weights absent: the focal module's own autograd function, which is what it calls)"""
    from seevcn_amd.pcdet.utils import loss_utils
    assert loss_utils.FUSED_LOSS
    x = case.x.to(cuda).requires_grad_(True)
    t, go = case.t.to(cuda), case.go.to(cuda)
    w = None if case.w is None else case.w.to(cuda)
    if case.kind == "focal":
        if w is None:
            out = loss_utils._FocalFunction.apply(x, t, None, case.kw["alpha"], case.kw["gamma"])
        else:
            out = loss_utils.SigmoidFocalClassificationLoss(gamma=case.kw["gamma"], alpha=case.kw["alpha"])(x, t, w)
    else:
        cw = None if case.kw.get("cw") is None else case.kw["cw"].tolist()
        mod = loss_utils.WeightedL1Loss(code_weights=cw) if case.kw["beta"] == 0.0 else loss_utils.WeightedSmoothL1Loss(beta=case.kw["beta"], code_weights=cw)
        out = mod(x, t, w)
    assert out.shape == x.shape
    # the fused kernel ran, not the module's torch chain (whose values would meet every bound below by themselves)
    assert type(out.grad_fn).__name__ == ("_FocalFunctionBackward" if case.kind == "focal" else "_SmoothL1FunctionBackward"), type(out.grad_fn).__name__
    out.backward(go)
    return out.detach().cpu().numpy(), x.grad.cpu().numpy()


def _run_losses(cuda, cases, kind):
    fails, worst_v, worst_g = [], 0.0, 0.0
    for case in cases:
        v, g = _loss(cuda, case)
        if not (np.isfinite(v).all() and np.isfinite(g).all()):
            fails.append("%s: a value or gradient is not finite" % case.name)
        rv, rg = case.ratios(v, g)
        worst_v, worst_g = max(worst_v, min(rv, 1e30)), max(worst_g, min(rg, 1e30))
        if not rv <= hr.K_KERNEL[kind]:
            fails.append("%s: value error / (eps32 scale) = %.3g > %.3g" % (case.name, rv, hr.K_KERNEL[kind]))
        if not rg <= hr.K_KERNEL[kind + "_grad"]:
            fails.append("%s: gradient error / (eps32 scale) = %.3g > %.3g" % (case.name, rg, hr.K_KERNEL[kind + "_grad"]))
        if not case.documented_zero(g):
            fails.append("%s: gradient not 0 where float64's is infinite (gamma < 1 at pt = 0)" % case.name)
        if kind == "smooth_l1":
            # the smooth-L1 value is made of - * / abs and comparisons only, every one correctly rounded on both sides: the fp32 chain's bits
            v32 = case.chain32()[0].numpy()
            if not np.array_equal(v.view(np.int32), v32.view(np.int32)):
                fails.append("%s: %d values differ in bits from the reference's fp32 chain" % (case.name, int((v.view(np.int32) != v32.view(np.int32)).sum())))
    return fails, worst_v, worst_g


def test_focal_loss_saturation_gamma_alpha_weights_and_shapes(cuda, hip_lib):
    """Logits +-0, +-1e-8, +-8, +-16.7, +-30, +-88, +-104 and random under targets 0, 1 and 0.3; gamma 2, 1.5, 0.5, 0; alpha 0.25, 0.5; weights absent,
    zero, random; C 1, 3, 10; rows 1, 255, 257: value and gradient finite and within the bound of the reference's chain in float64 with autograd."""
    fails, wv, wg = _run_losses(cuda, hr.focal_cases(), "focal")
    print("focal loss (%d calls): worst error / (eps32 scale): value %.3g of %.3g, gradient %.3g of %.3g" %
          (len(hr.focal_cases()), wv, hr.K_KERNEL["focal"], wg, hr.K_KERNEL["focal_grad"]))
    assert not fails, "\n".join(fails)


def test_smooth_l1_loss_beta_edges_code_weights_nan_and_shapes(cuda, hip_lib):
    """|d| exactly beta with beta 1/9, 1, 1e-5 and each moved one ulp either way, a beta at which the two branches differ in bits at |d| = beta (so
    that `<` shows against `<=`), float32(1e-5) given as a double (below 1e-5: the reference takes |d|), beta 0 through WeightedL1Loss, NaN targets (value and gradient 0),
    +-0 differences, code weights with a zero and a negative one, weights absent / zero / random, rows 1, 255, 257."""
    fails, wv, wg = _run_losses(cuda, hr.smooth_l1_cases(), "smooth_l1")
    print("smooth-L1 loss (%d calls): worst error / (eps32 scale): value %.3g of %.3g, gradient %.3g of %.3g" %
          (len(hr.smooth_l1_cases()), wv, hr.K_KERNEL["smooth_l1"], wg, hr.K_KERNEL["smooth_l1_grad"]))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind", ["focal", "smooth_l1"])
def test_loss_grid_stride_loops(cuda, hip_lib, kind):
    case = hr.stride_loss_inputs(kind)
    assert case.x.numel() == 1048576 + 300
    fails, wv, wg = _run_losses(cuda, [case], kind)
    print("%s, 1048876 elements: worst error / (eps32 scale): value %.3g, gradient %.3g" % (case.name, wv, wg))
    assert not fails, "\n".join(fails)
