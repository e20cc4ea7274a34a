"""Multi-head anchor family without a GPU: the numpy restatement (tests/multihead_reference.py) against the golden made by the reference's
own AnchorHeadMulti / AxisAlignedTargetAssigner / ResidualCoder / multi_classes_nms (tests/golden/make_multihead_golden.py), the restated
yaml files, and the module's construction (state_dict keys, shapes, parameter count of the reference module)."""
import json
import os

import numpy as np
import pytest
import torch

import multihead_inputs as I
import multihead_reference as MR
from seevcn_amd.pcdet import model_cfgs as C
from seevcn_amd.pcdet.models import dense_heads
from seevcn_amd.pcdet.models.dense_heads.anchor_head_multi import AnchorHeadMulti, SingleHead

CASES, build_head, golden = I.CASES, I.build_head, I.golden


def _thresholds():
    return [a["matched_threshold"] for a in I.ANCHORS], [a["unmatched_threshold"] for a in I.ANCHORS]


@pytest.mark.parametrize("case", ["coded", "plain"])
def test_set_major_anchors_and_assignment_match_the_reference(golden_dir, case):
    g = golden(golden_dir)
    _, _, extra, sincos = CASES[case]
    sets = MR.set_major_anchors(I.ANCHORS, I.GRID, I.PC_RANGE, width=7 + extra)
    flat = np.concatenate(sets)
    ref_anchors = g[f"{case}_anchors"]
    assert ref_anchors.shape == (144, 7 + extra + sincos)                                 # the reference's anchors carry code_size columns
    np.testing.assert_allclose(flat, ref_anchors[:, :7 + extra], rtol=0, atol=2e-5)
    assert not ref_anchors[:, 7:].any()
    np.testing.assert_array_equal(flat[24 * 0 + 6 * 1 + 2, :7], g["car_anchor"])          # [size, rot, z, y, x]: rot 0, y 1, x 2
    matched, unmatched = _thresholds()
    labels, targets, weights = MR.assign_targets(sets, [1, 2, 3], matched, unmatched, g[f"{case}_gt_boxes"], sincos)
    assert np.array_equal(labels, g[f"{case}_box_cls_labels"])
    np.testing.assert_allclose(targets, g[f"{case}_box_reg_targets"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(weights, g[f"{case}_reg_weights"])
    # what the inputs were built to reach
    assert not labels[1].any() and not (labels[0] == 3).any()                             # a scene without boxes; a scene without class C
    on_anchor = 24 * 0 + 6 * 1 + 2
    assert labels[0, on_anchor] == 1 and np.abs(targets[0, on_anchor, :6]).max() == 0     # the box that lies on an anchor
    cars = np.nonzero(labels[0, :48] == 1)[0]
    ov = MR.oh.iou_normal(MR.oh.nearest_bev(flat[cars, :7]), MR.oh.nearest_bev(g[f"{case}_gt_boxes"][0, 1:2, :7]))[:, 0]
    assert ((ov > 0) & (ov < unmatched[0])).any()                                         # a positive by forced match only
    assert int((labels[0, 48:] == 2).sum()) >= 1 and int((labels == -1).sum()) == 0


@pytest.mark.parametrize("case", ["coded", "plain"])
def test_coded_decode_matches_the_reference(golden_dir, case):
    g = golden(golden_dir)
    cfg, _, extra, sincos = CASES[case]
    head = build_head(case).eval()
    feat = torch.from_numpy(I.features())
    with torch.no_grad():
        x = head.shared_conv(feat) if head.shared_conv is not None else feat
        rets = [h(x) for h in head.rpn_heads]
    enc = torch.cat([r["box_preds"] for r in rets], dim=1).numpy()
    anchors = np.concatenate(MR.set_major_anchors(I.ANCHORS, I.GRID, I.PC_RANGE, width=7 + extra))
    boxes = MR.decode(enc, anchors[None], sincos)
    if case == "plain":
        dirs = torch.cat([r["dir_cls_preds"] for r in rets], dim=1).numpy()
        boxes[..., 6] = MR.oh.generate_predicted_boxes(enc, anchors, dirs, cfg["DIR_OFFSET"], cfg["DIR_LIMIT_OFFSET"], cfg["NUM_DIR_BINS"])[..., 6]
        np.testing.assert_allclose(torch.cat([r["cls_preds"] for r in rets], dim=1).numpy(), g["plain_batch_cls_preds"], rtol=1e-4, atol=1e-5)
    else:
        for i, r in enumerate(rets):
            np.testing.assert_allclose(r["cls_preds"].numpy(), g[f"coded_batch_cls_preds_{i}"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(boxes, g[f"{case}_batch_box_preds"], rtol=1e-4, atol=1e-4)
    # the torch coder the package ships, on the reference's anchors (one zero column more than a box when the heading is coded as sin/cos)
    ref_anchors = torch.from_numpy(g[f"{case}_anchors"])
    dec = head.box_coder.decode_torch(torch.from_numpy(enc), ref_anchors[None].expand(enc.shape[0], -1, -1))
    np.testing.assert_allclose(dec.numpy()[..., :6], boxes[..., :6], rtol=1e-5, atol=1e-5)
    gt = torch.from_numpy(g[f"{case}_gt_boxes"][0, :4, :-1])                              # encode_torch: every positive's target codes one of the boxes
    for p in np.nonzero(g[f"{case}_box_cls_labels"][0] > 0)[0]:
        enc_p = head.box_coder.encode_torch(gt, ref_anchors[p:p + 1].expand(4, -1)).numpy()
        assert np.abs(enc_p - g[f"{case}_box_reg_targets"][0, p]).max(axis=1).min() < 1e-5


def test_batched_class_wise_nms_matches_the_reference(golden_dir):
    g = golden(golden_dir)
    scores = [MR.sigmoid(g["post_logits_0"]), MR.sigmoid(g["post_logits_1"])]
    sizes = g["coded_label_mapping_sizes"]
    mapping = np.split(g["coded_label_mapping"], np.cumsum(sizes)[:-1])
    assert [m.tolist() for m in mapping] == [[1], [2, 3]]
    nms = I.POST["NMS_CONFIG"]
    res = MR.multi_classes_nms_batch(scores, g["post_boxes_in"], mapping, I.POST["SCORE_THRESH"], nms["NMS_PRE_MAXSIZE"], nms["NMS_POST_MAXSIZE"],
                                     nms["NMS_THRESH"])
    for i, (boxes, sc, labels, _) in enumerate(res):
        assert np.array_equal(labels, g[f"post_pred_labels_{i}"])                          # the keep lists: exact
        np.testing.assert_array_equal(boxes, g[f"post_pred_boxes_{i}"])
        np.testing.assert_allclose(sc, g[f"post_pred_scores_{i}"], rtol=1e-5, atol=1e-6)
    counts = [np.bincount(g[f"post_pred_labels_{i}"], minlength=4).tolist() for i in range(2)]
    assert counts[1][3] == 0 and counts[0][2] == nms["NMS_POST_MAXSIZE"] and 0 < counts[0][1] < nms["NMS_POST_MAXSIZE"]


def test_model_cfgs_restate_the_yaml(golden_dir):
    with open(os.path.join(golden_dir, "multihead_model_cfgs.json")) as f:
        parsed = json.load(f)
    assert C.second_multihead_model_cfg() == C.second_multihead_model_cfg("nuscenes") == parsed["nuscenes_models/cbgs_second_multihead.yaml"]
    assert C.second_multihead_model_cfg("kitti") == parsed["kitti_models/second_multihead.yaml"]
    assert C.pp_multihead_model_cfg() == parsed["nuscenes_models/cbgs_pp_multihead.yaml"]
    assert C.second_model_cfg()["BACKBONE_2D"] is C.SECOND_BACKBONE_2D and C.second_multihead_model_cfg()["BACKBONE_2D"] is not C.SECOND_BACKBONE_2D


@pytest.mark.parametrize("case", ["coded", "plain"])
def test_anchor_head_multi_builds_with_the_reference_state_dict(golden_dir, case):
    g = golden(golden_dir)
    head = build_head(case)
    assert type(head) is AnchorHeadMulti is dense_heads.__all__["AnchorHeadMulti"] and all(type(h) is SingleHead for h in head.rpn_heads)
    sd = head.state_dict()
    assert list(sd.keys()) == g[f"{case}_state_keys"].tolist()
    assert [str(tuple(v.shape)) for v in sd.values()] == g[f"{case}_state_shapes"].tolist()
    assert sum(p.numel() for p in head.parameters()) == int(g[f"{case}_param_count"])
    assert [h.head_label_indices.tolist() for h in head.rpn_heads] == [[1], [2, 3]]
    assert head.separate_multihead == (case == "coded") and head.use_multihead
    assert [h.num_class for h in head.rpn_heads] == ([1, 2] if case == "coded" else [3, 3])
    assert [h.num_anchors_per_location for h in head.rpn_heads] == [2, 4] and head.box_coder.code_size == (10 if case == "coded" else 7)
    assert (head.rpn_heads[0].conv_dir_cls is None) == (case == "coded") and (head.shared_conv is None) == (case == "plain")
    assert type(head.reg_loss_func).__name__ == ("WeightedL1Loss" if case == "coded" else "WeightedSmoothL1Loss")


def test_yaml_sized_heads_build_and_what_stays_unbuilt_still_refuses():
    from seevcn_amd.pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner
    from seevcn_amd.pcdet.utils import box_coder_utils, loss_utils
    cfg = C.second_multihead_model_cfg()["DENSE_HEAD"]
    head = dense_heads.__all__["AnchorHeadMulti"](model_cfg=cfg, input_channels=512, num_class=10, class_names=C.NUSC_CLASS_NAMES,
                                                  grid_size=np.array([1024, 1024, 40]), point_cloud_range=np.array([-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], np.float32))
    assert len(head.rpn_heads) == 6 and [h.num_anchors_per_location for h in head.rpn_heads] == [2, 4, 4, 2, 4, 4]
    assert sorted(head.rpn_heads[1].conv_box.keys()) == ["conv_angle", "conv_height", "conv_reg", "conv_size", "conv_velo"]
    assert sum(int(np.prod(a.shape[:-1])) for a in head.anchors) == 10 * 2 * 128 * 128
    for key, value in (("POS_FRACTION", 0.5), ("NORM_BY_NUM_EXAMPLES", True)):
        bad = dict(cfg, TARGET_ASSIGNER_CONFIG=dict(cfg["TARGET_ASSIGNER_CONFIG"], **{key: value}))
        with pytest.raises(NotImplementedError):
            AxisAlignedTargetAssigner(bad, C.NUSC_CLASS_NAMES, box_coder_utils.ResidualCoder())
    with pytest.raises(NotImplementedError):
        AxisAlignedTargetAssigner(cfg, C.NUSC_CLASS_NAMES, box_coder_utils.ResidualCoder(), match_height=True)
    # WeightedL1Loss: nan targets take the prediction, then code weights, then anchor weights
    loss = loss_utils.WeightedL1Loss(code_weights=[1.0, 2.0])
    x, t = torch.tensor([[[1.0, -2.0], [0.5, 0.5]]]), torch.tensor([[[0.0, float("nan")], [1.5, -0.5]]])
    np.testing.assert_allclose(loss(x, t, torch.tensor([[2.0, 0.5]])).numpy(), [[[2.0, 0.0], [0.5, 1.0]]])
