"""numpy restatement of the multi-head anchor family: head-major anchors, coded box encode / decode, set-major target assignment and
batched class-wise NMS over the oracle's NMS.  Test infrastructure; pinned by tests/golden/multihead_head.npz (outputs of the reference's
AnchorHeadMulti, AxisAlignedTargetAssigner, ResidualCoder and multi_classes_nms)."""
import numpy as np

from oracle import boxes as ob, heads as oh

F = np.float32


def set_major_anchors(anchor_cfgs, grid_size, pc_range, width=7):
    """[(A_s, width)] per class, each in the order [size, rot, z, y, x] (axis_aligned_target_assigner.py:69); columns past 7 are zero."""
    out = []
    for c in anchor_cfgs:
        flat, per = oh.generate_anchors([c], grid_size, pc_range)                # [(z, y, x), size * rot]
        a = flat.reshape(-1, per[0], 7).transpose(1, 0, 2).reshape(-1, 7)
        out.append(np.concatenate([a, np.zeros((len(a), width - 7), F)], axis=1))
    return out


def encode(boxes, anchors, sincos):
    """ResidualCoder.encode_torch (box_coder_utils.py:13-43): boxes (N, 7 + E), anchors (N, 7 + E) -> (N, 7 + sincos + E)"""
    t = oh.encode(boxes[:, :7], anchors[:, :7])
    rg, ra = boxes[:, 6], anchors[:, 6]
    ang = [np.cos(rg) - np.cos(ra), np.sin(rg) - np.sin(ra)] if sincos else [rg - ra]
    return np.concatenate([t[:, :6], np.stack(ang, 1), boxes[:, 7:] - anchors[:, 7:]], axis=1).astype(F)


def decode(enc, anchors, sincos):
    """ResidualCoder.decode_torch (box_coder_utils.py:45-77): enc (..., 7 + sincos + E), anchors (..., 7 + E) -> (..., 7 + E)"""
    out = oh.decode(enc[..., :7], anchors[..., :7])
    if sincos:
        out[..., 6] = np.arctan2(enc[..., 7] + np.sin(anchors[..., 6]), enc[..., 6] + np.cos(anchors[..., 6]))
    return np.concatenate([out, enc[..., 7 + sincos:] + anchors[..., 7:]], -1).astype(F)


def assign_targets(set_anchors, set_classes, matched, unmatched, gt_boxes, sincos):
    """AxisAlignedTargetAssigner.assign_targets with use_multihead (:36-130): per scene the sets' results concatenated set by set.
    set_anchors [(A_s, 7 + E)], gt_boxes (B, G, 8 + E) -> labels (B, A) int32, targets (B, A, 7 + sincos + E), weights (B, A)"""
    B, width = gt_boxes.shape[0], set_anchors[0].shape[1]
    A = sum(len(a) for a in set_anchors)
    labels, targets, weights = np.zeros((B, A), np.int32), np.zeros((B, A, width + sincos), F), np.zeros((B, A), F)
    for b in range(B):
        gt, at = gt_boxes[b], 0
        for s, anchors in enumerate(set_anchors):
            sl = slice(at, at + len(anchors))
            at += len(anchors)
            g = gt[gt[:, -1].astype(int) == set_classes[s]]
            if len(g) == 0:
                continue                                                         # all background
            ov = oh.iou_normal(oh.nearest_bev(anchors[:, :7]), oh.nearest_bev(g[:, :7]))
            arg = ov.argmax(1)
            mx = ov[np.arange(len(anchors)), arg]
            gmax = ov.max(0)
            gmax[gmax == 0] = -1
            force = (ov == gmax[None]).any(1)
            lab = np.full(len(anchors), -1, np.int32)
            lab[force] = set_classes[s]
            lab[mx >= F(matched[s])] = set_classes[s]
            fg = lab > 0
            lab[mx < F(unmatched[s])] = 0
            lab[force] = set_classes[s]
            labels[b, sl] = lab
            t = np.zeros((len(anchors), width + sincos), F)
            t[fg] = encode(g[arg[fg], :-1], anchors[fg], sincos)
            targets[b, sl] = t
            weights[b, sl] = (lab > 0).astype(F)
    return labels, targets, weights


def sigmoid(x):
    return (1.0 / (1.0 + np.exp(-x.astype(F)))).astype(F)


def multi_classes_nms_batch(head_scores, boxes, mappings, score_thresh, pre, post, nms_thresh, normal=False):
    """detector3d_template.py:224-249 over model_nms_utils.multi_classes_nms (:28-66), scene by scene, head by head, class by class.
    head_scores [(B, A_h, C_h)] SIGMOID scores, boxes (B, A, 7 + E), mappings [(C_h,)] -> per scene (boxes, scores, labels, anchor indices)"""
    out = []
    for b in range(boxes.shape[0]):
        sel, sc, lb, start = [], [], [], 0
        for scores, mapping in zip(head_scores, mappings):
            n = scores.shape[1]
            for k in range(scores.shape[2]):
                s = scores[b, :, k]
                cand = np.nonzero(s >= F(score_thresh))[0]
                order = cand[np.argsort(-s[cand], kind="stable")][:pre]
                keep = order[ob.nms(boxes[b, start + order, :7], nms_thresh, normal=normal)][:post]
                sel.append(start + keep), sc.append(s[keep]), lb.append(np.full(len(keep), mapping[k], np.int64))
            start += n
        sel = np.concatenate(sel)
        out.append((boxes[b, sel], np.concatenate(sc), np.concatenate(lb), sel))
    return out
