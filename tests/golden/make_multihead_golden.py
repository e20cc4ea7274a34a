"""Generate tests/golden/multihead_head.npz by running the REFERENCE's own AnchorHeadMulti (dense_heads/anchor_head_multi.py with
anchor_head_template.py, target_assigner/axis_aligned_target_assigner.py, utils/box_coder_utils.py ResidualCoder) and the MULTI_CLASSES_NMS branch
of Detector3DTemplate.post_processing over model_nms_utils.multi_classes_nms on CPU (the NMS extension stub is the oracle's), on the inputs of
multihead_inputs.py; and tests/golden/multihead_model_cfgs.json, the MODEL sections of the three multihead yaml files as parsed.

Run only in the build container (needs the reference):  python tests/golden/make_multihead_golden.py
"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refimport as R  # noqa: E402

R.import_pcdet()
from easydict import EasyDict  # noqa: E402  (stub)
from pcdet.models.dense_heads.anchor_head_multi import AnchorHeadMulti  # noqa: E402
from pcdet.models.detectors.detector3d_template import Detector3DTemplate  # noqa: E402
from oracle import boxes as ob  # noqa: E402
import multihead_inputs as I  # noqa: E402

out = {}
feat = torch.from_numpy(I.features())
gt10 = None
for case, cfg, seed in (("coded", I.HEAD_CODED, 11), ("plain", I.HEAD_PLAIN, 12)):
    torch.manual_seed(0)
    head = AnchorHeadMulti(model_cfg=EasyDict(cfg), input_channels=I.IN_CHANNELS, num_class=3, class_names=I.CLASS_NAMES, grid_size=I.GRID,
                           point_cloud_range=np.array(I.PC_RANGE, np.float32), predict_boxes_when_training=True)
    head.load_state_dict(I.seeded_head_state(head, seed))
    if gt10 is None:
        car = head.anchors[0][0, 1, 2, 0, 0, :7].numpy().copy()            # the Car anchor at y index 1, x index 2, rotation 0
        gt10 = I.gt_boxes(car)
        out["car_anchor"] = car
    gt = gt10 if case == "coded" else np.concatenate([gt10[..., :7], gt10[..., 9:]], -1)
    head.train()
    dd = head({'spatial_features_2d': feat, 'gt_boxes': torch.from_numpy(gt.copy()), 'batch_size': I.BATCH})
    loss, tb = head.get_loss()
    fr = head.forward_ret_dict
    out[f"{case}_param_count"] = np.int64(sum(p.numel() for p in head.parameters()))
    out[f"{case}_state_keys"] = np.array(list(head.state_dict().keys()))
    out[f"{case}_state_shapes"] = np.array([str(tuple(v.shape)) for v in head.state_dict().values()])
    out[f"{case}_anchors"] = torch.cat([a.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, a.shape[-1]) for a in head.anchors], 0).numpy()
    out[f"{case}_gt_boxes"] = gt
    for k in ("box_cls_labels", "box_reg_targets", "reg_weights"):
        out[f"{case}_{k}"] = fr[k].numpy()
    for k in ("rpn_loss", "rpn_loss_cls", "rpn_loss_loc") + (("rpn_loss_dir",) if case == "plain" else ()):
        out[f"{case}_{k}"] = np.float32(loss.item() if k == "rpn_loss" else tb[k])
    head.load_state_dict(I.seeded_head_state(head, seed))                    # the train-mode pass moved the BatchNorm running statistics
    head.eval()
    with torch.no_grad():
        de = head({'spatial_features_2d': feat, 'batch_size': I.BATCH})
    cls = de['batch_cls_preds']
    if isinstance(cls, list):
        for i, c in enumerate(cls):
            out[f"{case}_batch_cls_preds_{i}"] = c.numpy()
        out[f"{case}_label_mapping"] = np.concatenate([m.numpy() for m in de['multihead_label_mapping']])
        out[f"{case}_label_mapping_sizes"] = np.array([len(m) for m in de['multihead_label_mapping']])
    else:
        out[f"{case}_batch_cls_preds"] = cls.numpy()
        assert 'multihead_label_mapping' not in de
    out[f"{case}_batch_box_preds"] = de['batch_box_preds'].numpy()
    assert de['cls_preds_normalized'] is False
    print(case, "loss", loss.item(), tb, "pos", int((fr['box_cls_labels'] > 0).sum()), "ignore", int((fr['box_cls_labels'] < 0).sum()))
    if case == "coded":
        mapping = de['multihead_label_mapping']
        anchors9 = out["coded_anchors"][:, :9]

# ---- post-processing on crafted predictions of the coded case: distinct scores, boxes = jittered anchors; drawn again until no pair of one
# scene has an oracle IoU within 1e-3 of the NMS threshold, so that every suppression is decided
nms_thresh = I.POST['NMS_CONFIG']['NMS_THRESH']
rng = np.random.default_rng(5)
while True:
    boxes = np.repeat(anchors9[None], I.BATCH, 0).copy()
    boxes[..., 0:2] += rng.normal(size=boxes[..., 0:2].shape).astype(np.float32) * 0.6
    boxes[..., 3:6] *= np.exp(rng.normal(size=boxes[..., 3:6].shape) * 0.1).astype(np.float32)
    boxes[..., 6] += rng.normal(size=boxes[..., 6].shape).astype(np.float32) * 0.3
    boxes[..., 7:9] = rng.normal(size=boxes[..., 7:9].shape).astype(np.float32)
    iou = np.stack([ob.boxes_iou_bev(b[:, :7], b[:, :7]) for b in boxes])
    if np.abs(iou - nms_thresh).min() > 1e-3:
        break
logits = [rng.normal(size=(I.BATCH, 48, 1)).astype(np.float32) * 1.5 - 2.0, rng.normal(size=(I.BATCH, 96, 2)).astype(np.float32) * 1.5]
logits[1][1, :, 1] = -6.0                                                     # scene 1: no Cyclist passes the score threshold
for lg in logits:
    s = torch.sigmoid(torch.from_numpy(lg)).numpy()
    assert len(np.unique(s)) == s.size - (96 - 1 if lg.shape[2] == 2 else 0) or lg.shape[2] == 1 and len(np.unique(s)) == s.size
self_ns = SimpleNamespace(model_cfg=EasyDict(POST_PROCESSING=I.POST), num_class=3, generate_recall_record=Detector3DTemplate.generate_recall_record)
bd = {'batch_size': I.BATCH, 'batch_box_preds': torch.from_numpy(boxes), 'batch_cls_preds': [torch.from_numpy(x) for x in logits],
      'multihead_label_mapping': mapping, 'cls_preds_normalized': False}
pred_dicts, _ = Detector3DTemplate.post_processing(self_ns, bd)
out["post_boxes_in"] = boxes
out["post_logits_0"], out["post_logits_1"] = logits
for i, d in enumerate(pred_dicts):
    out[f"post_pred_boxes_{i}"] = d['pred_boxes'].numpy()
    out[f"post_pred_scores_{i}"] = d['pred_scores'].numpy()
    out[f"post_pred_labels_{i}"] = d['pred_labels'].numpy()
    print("scene", i, "kept", len(d['pred_labels']), np.bincount(d['pred_labels'].numpy(), minlength=4))
np.savez_compressed(os.path.join(HERE, "multihead_head.npz"), **out)
print(os.path.getsize(os.path.join(HERE, "multihead_head.npz")), "bytes")

# ---- the yaml MODEL sections, as data
cfgs = {}
for name in ("nuscenes_models/cbgs_second_multihead.yaml", "kitti_models/second_multihead.yaml", "nuscenes_models/cbgs_pp_multihead.yaml"):
    with open(os.path.join(R.REF, "detector3d", "tools", "cfgs", name)) as f:
        cfgs[name] = yaml.safe_load(f)["MODEL"]
with open(os.path.join(HERE, "multihead_model_cfgs.json"), "w") as f:
    json.dump(cfgs, f, indent=1)
