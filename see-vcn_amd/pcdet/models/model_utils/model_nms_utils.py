import torch

from .... import _lib
from ...ops.iou3d_nms import iou3d_nms_utils
from ...utils.common_utils import cfg_get


def class_agnostic_nms(box_scores, box_preds, nms_config, score_thresh=None):
    """score threshold -> top-k (NMS_PRE_MAXSIZE) -> NMS_TYPE(NMS_THRESH) -> first NMS_POST_MAXSIZE; returns indices into the
    original arrays and their scores (reference model_utils/model_nms_utils.py:6-25)."""
    src_box_scores = box_scores
    if score_thresh is not None:
        scores_mask = (box_scores >= score_thresh)
        box_scores = box_scores[scores_mask]
        box_preds = box_preds[scores_mask]
    selected = []
    if box_scores.shape[0] > 0:
        box_scores_nms, indices = torch.topk(box_scores, k=min(cfg_get(nms_config, 'NMS_PRE_MAXSIZE'), box_scores.shape[0]))
        boxes_for_nms = box_preds[indices]
        keep_idx, _ = getattr(iou3d_nms_utils, cfg_get(nms_config, 'NMS_TYPE'))(boxes_for_nms[:, 0:7], box_scores_nms,
                                                                                 cfg_get(nms_config, 'NMS_THRESH'),
                                                                                 max_keep=cfg_get(nms_config, 'NMS_POST_MAXSIZE'))
        selected = indices[keep_idx[:cfg_get(nms_config, 'NMS_POST_MAXSIZE')]]
    if score_thresh is not None:
        original_idxs = scores_mask.nonzero().view(-1)
        selected = original_idxs[selected]
    return selected, src_box_scores[selected]


def class_agnostic_nms_padded(box_scores, box_preds, nms_config):
    """class_agnostic_nms without a score threshold as a fixed-size result: (selected (NMS_POST_MAXSIZE,) indices into the original arrays,
    valid (NMS_POST_MAXSIZE,) bool); the survivors come first, in score order.  No device -> host read."""
    post = cfg_get(nms_config, 'NMS_POST_MAXSIZE')
    if box_scores.shape[0] == 0:
        z = torch.zeros((post,), dtype=torch.int64, device=box_scores.device)
        return z, z.bool()
    box_scores_nms, indices = torch.topk(box_scores, k=min(cfg_get(nms_config, 'NMS_PRE_MAXSIZE'), box_scores.shape[0]))
    # torch.topk returns its values in descending order: the NMS need not sort them again
    keep, valid = iou3d_nms_utils.nms_gpu_padded(box_preds[indices][:, 0:7], box_scores_nms, cfg_get(nms_config, 'NMS_THRESH'), post,
                                                 normal=cfg_get(nms_config, 'NMS_TYPE') == 'nms_normal_gpu', presorted=True)
    return indices[keep], valid


def multi_classes_nms(cls_scores, box_preds, nms_config, score_thresh=None):
    """cls_scores (N, num_class), box_preds (N, 7 + C) -> (pred_scores, pred_labels 0-based, pred_boxes): class_agnostic_nms class by class, the
    survivors of class k before those of class k + 1 (reference model_utils/model_nms_utils.py:28-66).  One NMS call and one device -> host
    read per class; a whole batch goes through multi_classes_nms_batch."""
    pred_scores, pred_labels, pred_boxes = [], [], []
    post = cfg_get(nms_config, 'NMS_POST_MAXSIZE')
    for k in range(cls_scores.shape[1]):
        if score_thresh is not None:
            scores_mask = (cls_scores[:, k] >= score_thresh)
            box_scores = cls_scores[scores_mask, k]
            cur_box_preds = box_preds[scores_mask]
        else:
            box_scores = cls_scores[:, k]
            cur_box_preds = box_preds
        selected = []
        if box_scores.shape[0] > 0:
            box_scores_nms, indices = torch.topk(box_scores, k=min(cfg_get(nms_config, 'NMS_PRE_MAXSIZE'), box_scores.shape[0]))
            keep_idx, _ = getattr(iou3d_nms_utils, cfg_get(nms_config, 'NMS_TYPE'))(cur_box_preds[indices][:, 0:7], box_scores_nms,
                                                                                     cfg_get(nms_config, 'NMS_THRESH'), max_keep=post)
            selected = indices[keep_idx[:post]]
        pred_scores.append(box_scores[selected])
        pred_labels.append(box_scores.new_ones(len(selected)).long() * k)
        pred_boxes.append(cur_box_preds[selected])
    return torch.cat(pred_scores, dim=0), torch.cat(pred_labels, dim=0), torch.cat(pred_boxes, dim=0)


def multi_classes_nms_batch(batch_cls_preds, batch_box_preds, multihead_label_mapping, nms_config, score_thresh=None, normalized=False):
    """Class-wise NMS of a whole batch: per scene the concatenation, head by head, of multi_classes_nms(head's scores, head's boxes) with the
    labels mapped through multihead_label_mapping (reference detector3d_template.py:224-249) -- as ONE segmented NMS (sv_nms_segments: a
    segment per scene x class) and ONE device -> host read (the survivor counts).
    batch_cls_preds: [(B, A_h, C_h)] per head, the heads' anchors consecutive in batch_box_preds (B, sum A_h, 7 + C); multihead_label_mapping:
    [(C_h,)] label of each head's classes.  Returns a list of B dicts pred_boxes / pred_scores / pred_labels."""
    lib = _lib.load()
    _lib.require_cuda(batch_box_preds, *batch_cls_preds)
    B, A, width = batch_box_preds.shape
    dev = batch_box_preds.device
    pre_cfg, post = int(cfg_get(nms_config, 'NMS_PRE_MAXSIZE')), int(cfg_get(nms_config, 'NMS_POST_MAXSIZE'))
    assert post >= 1 and pre_cfg >= 1
    pre = min(pre_cfg, max(int(c.shape[1]) for c in batch_cls_preds))
    vals, idxs, start = [], [], 0
    for cls, mapping in zip(batch_cls_preds, multihead_label_mapping):
        assert cls.shape[2] == len(mapping)
        scores = (cls if normalized else torch.sigmoid(cls)).transpose(1, 2)                        # (B, C_h, A_h)
        if score_thresh is not None:
            scores = scores.masked_fill(scores < score_thresh, float('-inf'))
        k = min(pre, int(cls.shape[1]))
        v, i = torch.topk(scores, k=k, dim=-1)                                                      # sorted: descending scores
        if k < pre:
            v = torch.nn.functional.pad(v, (0, pre - k), value=float('-inf'))
            i = torch.nn.functional.pad(i, (0, pre - k), value=0)
        vals.append(v)
        idxs.append(i + start)
        start += int(cls.shape[1])
    assert start == A, "the heads' anchors must add up to the boxes"
    vals, idxs = torch.cat(vals, dim=1), torch.cat(idxs, dim=1)                                     # (B, C, pre): segment s = scene * C + class
    labels = torch.cat([m.reshape(-1) for m in multihead_label_mapping]).to(dev)
    C = int(vals.shape[1])
    S = B * C
    counts = (vals > float('-inf')).sum(-1).to(torch.int32).reshape(S).contiguous()
    flat_idx = (idxs + torch.arange(B, device=dev).view(B, 1, 1) * A).reshape(S, pre)                # rows of the (B * A, width) boxes
    all_boxes = batch_box_preds.reshape(B * A, width)
    seg_boxes = all_boxes[:, 0:7][flat_idx.reshape(-1)].reshape(S, pre, 7).contiguous().float()
    keep = torch.empty((S, post), dtype=torch.int64, device=dev)
    num_out = torch.empty((S,), dtype=torch.int32, device=dev)
    scratch = _lib.workspace.scratch("nms_segments", lib.sv_nms_segments_scratch_bytes(S, pre), dev)
    normal = cfg_get(nms_config, 'NMS_TYPE') == 'nms_normal_gpu'
    _lib.launch("sv_nms_segments", _lib.ptr(seg_boxes), _lib.ptr(counts), S, pre, float(cfg_get(nms_config, 'NMS_THRESH')), int(normal), post,
                _lib.ptr(scratch), _lib.ptr(keep), _lib.ptr(num_out))
    kept = _lib.host_ints([num_out])                                                                # the one device -> host read
    # survivors of segment s: keep[s, :kept[s]]; their flat slots, in the output order, are known on the host
    slots = torch.tensor([s * keep.shape[1] + j for s in range(S) for j in range(kept[s])], dtype=torch.int64).to(dev, non_blocking=True)
    local = keep.reshape(-1)[slots]
    seg = torch.div(slots, keep.shape[1], rounding_mode='floor')
    rows = flat_idx[seg, local]
    out_boxes, out_scores, out_labels = all_boxes[rows], vals.reshape(S, pre)[seg, local], labels[seg % C]
    pred_dicts, at = [], 0
    for b in range(B):
        n = sum(kept[b * C:(b + 1) * C])
        pred_dicts.append({'pred_boxes': out_boxes[at:at + n], 'pred_scores': out_scores[at:at + n], 'pred_labels': out_labels[at:at + n]})
        at += n
    return pred_dicts
