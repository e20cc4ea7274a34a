"""AnchorHeadMulti on the GPU: coded target assignment and decode (sv_assign_targets_axis_aligned_coded, sv_anchor_decode_coded), losses, eval
outputs and class-wise post-processing (sv_nms_segments) against the golden made by the reference's own modules
(tests/golden/make_multihead_golden.py); the new entries in the old layout against the old entries bit for bit; a detector end to end."""
import os

import numpy as np
import pytest
import torch

import multihead_inputs as I
import multihead_reference as MR
from seeding import seeded_state_dict
from tolerances import assert_close_per_channel
from seevcn_amd.pcdet import model_cfgs as C

pytestmark = pytest.mark.gpu
build_head, golden = I.build_head, I.golden


def _close(got, want, name):
    """the project's 1e-3 relative bound (oracle/tolerances.py), per column"""
    assert_close_per_channel(got, want, rtol=1e-3, atol_frac=1e-4, name=name)


@pytest.mark.parametrize("case", ["coded", "plain"])
def test_hip_multihead_train_forward_targets_and_losses(golden_dir, cuda, hip_lib, case):
    g = golden(golden_dir)
    head = build_head(case).to(cuda).train()
    feat = torch.from_numpy(I.features()).to(cuda)
    dd = head({"spatial_features_2d": feat, "gt_boxes": torch.from_numpy(g[f"{case}_gt_boxes"]).to(cuda), "batch_size": I.BATCH})
    fr = head.forward_ret_dict
    assert np.array_equal(fr["box_cls_labels"].cpu().numpy(), g[f"{case}_box_cls_labels"])                 # labels: exact
    _close(fr["box_reg_targets"].cpu().numpy(), g[f"{case}_box_reg_targets"], "box_reg_targets")
    np.testing.assert_array_equal(fr["reg_weights"].cpu().numpy(), g[f"{case}_reg_weights"])
    assert isinstance(fr["cls_preds"], list) == isinstance(fr["box_preds"], list) == (case == "coded")
    assert ("dir_cls_preds" in fr) == (case == "plain")
    assert dd["batch_box_preds"].shape == g[f"{case}_batch_box_preds"].shape and dd["cls_preds_normalized"] is False
    loss, tb = head.get_loss()
    keys = ("rpn_loss", "rpn_loss_cls", "rpn_loss_loc") + (("rpn_loss_dir",) if case == "plain" else ())
    assert set(tb) == set(keys)
    for k in keys:
        want = float(g[f"{case}_{k}"])
        assert abs(float(tb[k]) - want) <= 1e-3 * abs(want), (k, float(tb[k]), want)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())


@pytest.mark.parametrize("case", ["coded", "plain"])
def test_hip_multihead_eval_outputs(golden_dir, cuda, hip_lib, case):
    g = golden(golden_dir)
    head = build_head(case).to(cuda).eval()
    with torch.no_grad():
        dd = head({"spatial_features_2d": torch.from_numpy(I.features()).to(cuda), "batch_size": I.BATCH})
    if case == "coded":
        assert isinstance(dd["batch_cls_preds"], list) and [m.tolist() for m in dd["multihead_label_mapping"]] == [[1], [2, 3]]
        for i, c in enumerate(dd["batch_cls_preds"]):
            _close(c.cpu().numpy(), g[f"coded_batch_cls_preds_{i}"], f"batch_cls_preds[{i}]")
    else:
        assert "multihead_label_mapping" not in dd
        _close(dd["batch_cls_preds"].cpu().numpy(), g["plain_batch_cls_preds"], "batch_cls_preds")
    _close(dd["batch_box_preds"].cpu().numpy(), g[f"{case}_batch_box_preds"], "batch_box_preds")
    assert dd["cls_preds_normalized"] is False


def test_hip_coded_entries_in_the_old_layout_equal_the_old_entries_bit_for_bit(golden_dir, cuda, hip_lib):
    """set_major 0, no extras, no sin/cos: sv_assign_targets_axis_aligned_coded and sv_anchor_decode_coded against sv_assign_targets_axis_aligned
    and sv_anchor_decode on the inputs of second_head.npz (SECOND's single head: 211 200 anchors, 24 boxes per scene)."""
    import seevcn_amd._lib as L
    from seevcn_amd.pcdet.models import dense_heads
    g = np.load(os.path.join(golden_dir, "second_head.npz"))
    feat = (np.random.default_rng(int(g["feat_seed"])).normal(size=(2, 16, 200, 176)) * 0.5).astype(np.float32)
    head = dense_heads.__all__["AnchorHeadSingle"](model_cfg=C.SECOND_DENSE_HEAD, input_channels=16, num_class=3, class_names=C.CLASS_NAMES,
                                                   grid_size=np.array([1408, 1600, 40]), point_cloud_range=np.array(C.KITTI_RANGE, np.float32))
    head.load_state_dict(seeded_state_dict(head, seed=3))
    head = head.to(cuda).train()
    gt = torch.from_numpy(g["gt_boxes"]).to(cuda)
    dd = head({"spatial_features_2d": torch.from_numpy(feat).to(cuda), "gt_boxes": gt, "batch_size": 2})
    fr = head.forward_ret_dict
    t = head.target_assigner._device_tables(head.anchors)
    B, G, A = gt.shape[0], gt.shape[1], t["anchors"].shape[0]
    labels = torch.full((B, A), -9, dtype=torch.int32, device=cuda)
    targets = torch.full((B, A, 7), float("nan"), device=cuda)
    weights = torch.full((B, A), float("nan"), device=cuda)
    scratch = torch.empty((B * G,), device=cuda)
    rc = hip_lib.sv_assign_targets_axis_aligned_coded(L.ptr(t["anchors"]), A, 0, 0, 0, t["per_loc"], 3, L.ptr(t["offs"]), L.ptr(t["cls"]), L.ptr(t["mthr"]),
                                                      L.ptr(t["uthr"]), L.ptr(gt.contiguous()), B, G, L.ptr(scratch), L.ptr(labels), L.ptr(targets),
                                                      L.ptr(weights), L.stream())
    L.check(rc, "sv_assign_targets_axis_aligned_coded")
    assert torch.equal(labels, fr["box_cls_labels"]) and int((labels > 0).sum()) == int(g["num_pos"])
    assert torch.equal(targets.view(torch.int32), fr["box_reg_targets"].view(torch.int32))
    assert torch.equal(weights.view(torch.int32), fr["reg_weights"].view(torch.int32))
    anchors = head._anchors_on(cuda)
    enc = fr["box_preds"].reshape(B, A, 7).contiguous()
    dirs = fr["dir_cls_preds"].reshape(B, A, 2).contiguous()
    out = torch.full((B, A, 7), float("nan"), device=cuda)
    rc = hip_lib.sv_anchor_decode_coded(L.ptr(anchors), A, 0, 0, L.ptr(enc), L.ptr(dirs), B, 2, float(C.SECOND_DENSE_HEAD["DIR_OFFSET"]),
                                        float(C.SECOND_DENSE_HEAD["DIR_LIMIT_OFFSET"]), L.ptr(out), L.stream())
    L.check(rc, "sv_anchor_decode_coded")
    assert torch.equal(out.view(torch.int32), dd["batch_box_preds"].view(torch.int32))


def _post_inputs(g, cuda):
    return {"batch_size": I.BATCH, "batch_box_preds": torch.from_numpy(g["post_boxes_in"]).to(cuda),
            "batch_cls_preds": [torch.from_numpy(g["post_logits_0"]).to(cuda), torch.from_numpy(g["post_logits_1"]).to(cuda)],
            "multihead_label_mapping": [torch.tensor([1], device=cuda), torch.tensor([2, 3], device=cuda)], "cls_preds_normalized": False}


def test_hip_multi_classes_post_processing(golden_dir, cuda, hip_lib):
    from seevcn_amd.pcdet.models.detectors.detector3d_template import Detector3DTemplate
    from seevcn_amd.pcdet.models.model_utils import model_nms_utils
    g = golden(golden_dir)
    det = Detector3DTemplate(dict(POST_PROCESSING=I.POST), 3, C.SyntheticDatasetInfo())
    bd = _post_inputs(g, cuda)
    pred_dicts, recall = det.post_processing(bd)
    assert len(pred_dicts) == I.BATCH and recall == {}
    scores = [MR.sigmoid(g["post_logits_0"]), MR.sigmoid(g["post_logits_1"])]
    nms = I.POST["NMS_CONFIG"]
    restated = MR.multi_classes_nms_batch(scores, g["post_boxes_in"], [[1], [2, 3]], I.POST["SCORE_THRESH"], nms["NMS_PRE_MAXSIZE"], nms["NMS_POST_MAXSIZE"],
                                          nms["NMS_THRESH"])
    for i, d in enumerate(pred_dicts):
        assert set(d) == {"pred_boxes", "pred_scores", "pred_labels"}
        assert np.array_equal(d["pred_labels"].cpu().numpy(), g[f"post_pred_labels_{i}"])                   # exact
        sel = restated[i][3]                                                                                 # the anchors the reference selected
        np.testing.assert_array_equal(d["pred_boxes"].cpu().numpy(), g["post_boxes_in"][i, sel])            # = the gathered inputs
        np.testing.assert_array_equal(d["pred_boxes"].cpu().numpy(), g[f"post_pred_boxes_{i}"])
        lab = torch.from_numpy(restated[i][2]).to(cuda)                                                      # scores = the sigmoid of the logit of (anchor, class)
        at = torch.from_numpy(sel).to(cuda)
        own = torch.where(lab == 1, torch.sigmoid(bd["batch_cls_preds"][0][i, at.clamp(max=47), 0]),
                          torch.sigmoid(bd["batch_cls_preds"][1][i, (at - 48).clamp(min=0), (lab - 2).clamp(min=0)]))
        assert torch.equal(d["pred_scores"], own)
        _close(d["pred_scores"].cpu().numpy()[:, None], g[f"post_pred_scores_{i}"][:, None], "pred_scores")
        # the batched path against the per-class loop over nms_gpu
        start, parts = 0, []
        for cls, mapping in zip(bd["batch_cls_preds"], bd["multihead_label_mapping"]):
            s, l, b = model_nms_utils.multi_classes_nms(torch.sigmoid(cls[i]), bd["batch_box_preds"][i, start:start + cls.shape[1]], nms, I.POST["SCORE_THRESH"])
            parts.append((s, mapping[l], b))
            start += cls.shape[1]
        for k, key in enumerate(("pred_scores", "pred_labels", "pred_boxes")):
            assert torch.equal(d[key], torch.cat([p[k] for p in parts])), key
    # the single-tensor form keeps the reference's mapping arange(1, num_class): its width check then refuses num_class columns
    with pytest.raises(AssertionError):
        det.post_processing(dict(bd, batch_cls_preds=torch.zeros((I.BATCH, 144, 3), device=cuda)))


def test_hip_second_multihead_detector_train_and_eval(cuda, hip_lib):
    """SECONDNet from second_multihead_model_cfg (10 classes in 6 heads, 9-d boxes) on a grid cut down to a 16 x 16 BEV map."""
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.models import detectors
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=60)
    gt10 = np.concatenate([gt[..., :7], np.zeros(gt.shape[:2] + (2,), np.float32), gt[..., 7:]], -1)
    gt10[..., 7:9] = np.random.default_rng(0).normal(size=gt10[..., 7:9].shape) * (gt10[..., 9:] > 0)
    ds = C.SyntheticDatasetInfo(class_names=C.NUSC_CLASS_NAMES, point_cloud_range=C.KITTI_RANGE, voxel_size=(0.55, 0.625, 0.1))
    cfg = dict(C.second_multihead_model_cfg(), VFE=dict(NAME="DynMeanVFE"))
    net = detectors.build_detector(cfg, num_class=10, dataset=ds)
    sd = seeded_state_dict(net, seed=6)
    sd.update({k: v for k, v in net.state_dict().items() if k.endswith("head_label_indices")})
    net.load_state_dict(sd)
    net = net.to(cuda)
    assert type(net.dense_head).__name__ == "AnchorHeadMulti" and sum(int(np.prod(a.shape[:-1])) for a in net.dense_head.anchors) == 10 * 2 * 16 * 16
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt10).to(cuda)}
    net.train()
    ret, tb, _ = net(dict(batch))
    assert torch.isfinite(ret["loss"]) and set(tb) >= {"loss_rpn", "rpn_loss_cls", "rpn_loss_loc", "rpn_loss"} and "rpn_loss_dir" not in tb
    ret["loss"].backward()
    for k, p in net.dense_head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    net.eval()
    with torch.no_grad():
        bd = dict(batch)
        for m in net.module_list:
            bd = m(bd)
        pred_dicts, recall = net.post_processing(bd)
    assert len(pred_dicts) == 2 and "gt" in recall
    for d in pred_dicts:
        assert set(d) == {"pred_boxes", "pred_scores", "pred_labels"} and d["pred_boxes"].shape[1] == 9
        assert d["pred_boxes"].shape[0] == d["pred_scores"].shape[0] == d["pred_labels"].shape[0] <= 10 * 83
        if len(d["pred_labels"]):
            assert 1 <= int(d["pred_labels"].min()) and int(d["pred_labels"].max()) <= 10 and float(d["pred_scores"].min()) >= 0.1
