import numpy as np
import torch

from ..... import _lib
from ....utils.common_utils import cfg_get


class AxisAlignedTargetAssigner(object):
    """Drop-in for the reference AxisAlignedTargetAssigner (target_assigner/axis_aligned_target_assigner.py:8-210) on the
    fused HIP kernel sv_assign_targets_axis_aligned: no (anchors x gt) IoU matrix, no python loop over batch x class.
    Built: the deterministic branch every config uses (POS_FRACTION -1, MATCH_HEIGHT False, NORM_BY_NUM_EXAMPLES False).  Multihead
    (head-major anchors), boxes wider than 7 and the sin/cos heading code go through sv_assign_targets_axis_aligned_coded."""

    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        super().__init__()
        anchor_generator_cfg = cfg_get(model_cfg, 'ANCHOR_GENERATOR_CONFIG')
        anchor_target_cfg = cfg_get(model_cfg, 'TARGET_ASSIGNER_CONFIG')
        self.box_coder = box_coder
        self.match_height = match_height
        self.class_names = np.array(class_names)
        self.anchor_class_names = [c['class_name'] for c in anchor_generator_cfg]
        pos_fraction = cfg_get(anchor_target_cfg, 'POS_FRACTION', -1.0)
        self.pos_fraction = pos_fraction if pos_fraction >= 0 else None
        self.sample_size = cfg_get(anchor_target_cfg, 'SAMPLE_SIZE', 512)
        self.norm_by_num_examples = cfg_get(anchor_target_cfg, 'NORM_BY_NUM_EXAMPLES', False)
        self.matched_thresholds = {c['class_name']: c['matched_threshold'] for c in anchor_generator_cfg}
        self.unmatched_thresholds = {c['class_name']: c['unmatched_threshold'] for c in anchor_generator_cfg}
        self.use_multihead = cfg_get(model_cfg, 'USE_MULTIHEAD', False)
        if self.pos_fraction is not None or self.match_height or self.norm_by_num_examples:
            raise NotImplementedError("only the deterministic nearest-BEV branch is built (POS_FRACTION<0, MATCH_HEIGHT False, "
                                      "NORM_BY_NUM_EXAMPLES False)")
        self.sincos = int(bool(getattr(box_coder, 'encode_angle_by_sincos', False)))
        self._dev = {}

    def _device_tables(self, all_anchors):
        dev = all_anchors[0].device
        key = (dev, tuple(a.data_ptr() for a in all_anchors))
        if key not in self._dev:
            per_set = [int(a.shape[3] * a.shape[4]) for a in all_anchors]
            full = int(all_anchors[0].shape[-1])
            width = full - self.sincos                               # a sin/cos coder's anchors carry one zero column more than a box
            set_class = np.array([int(np.nonzero(self.class_names == n)[0][0]) + 1 for n in self.anchor_class_names], np.int32)
            if self.use_multihead:                                   # each set one run [size, rot, z, y, x]; offsets count anchors (reference :69)
                offs = np.concatenate([[0], np.cumsum([int(a.numel() // full) for a in all_anchors])]).astype(np.int32)
                anchors = torch.cat([a.permute(3, 4, 0, 1, 2, 5).reshape(-1, full) for a in all_anchors], dim=0)[:, :width].contiguous().float()
            else:
                offs = np.concatenate([[0], np.cumsum(per_set)]).astype(np.int32)
                anchors = torch.cat([a.reshape(*a.shape[:3], -1, full) for a in all_anchors], dim=-2).reshape(-1, full)[:, :width].contiguous().float()
            self._dev[key] = dict(
                anchors=anchors, per_loc=int(sum(per_set)),
                offs=torch.from_numpy(offs).to(dev), cls=torch.from_numpy(set_class).to(dev),
                mthr=torch.tensor([self.matched_thresholds[n] for n in self.anchor_class_names], dtype=torch.float32, device=dev),
                uthr=torch.tensor([self.unmatched_thresholds[n] for n in self.anchor_class_names], dtype=torch.float32, device=dev))
        return self._dev[key]

    def assign_targets(self, all_anchors, gt_boxes_with_classes):
        """all_anchors: [(nz,ny,nx,n_size,n_rot,7+E), ...] per class; gt_boxes (B, M, 8+E) -> dict of (B,A[,code_size]) tensors"""
        _lib.require_cuda(gt_boxes_with_classes, *all_anchors)
        t = self._device_tables(all_anchors)
        gt = gt_boxes_with_classes.contiguous().float()
        B, G = gt.shape[0], gt.shape[1]
        A, width = t['anchors'].shape
        extra = width - 7
        assert gt.shape[2] == 8 + extra, "gt_boxes must be [box (7 + extras), class] rows of the anchors' width + 1"
        dev = gt.device
        labels = torch.empty((B, A), dtype=torch.int32, device=dev)
        targets = torch.empty((B, A, 7 + self.sincos + extra), dtype=torch.float32, device=dev)
        weights = torch.empty((B, A), dtype=torch.float32, device=dev)
        scratch = torch.empty((max(B * G, 1),), dtype=torch.float32, device=dev)
        if not (self.use_multihead or extra or self.sincos):
            _lib.launch("sv_assign_targets_axis_aligned", _lib.ptr(t['anchors']), A, t['per_loc'], len(all_anchors), _lib.ptr(t['offs']), _lib.ptr(t['cls']),
                        _lib.ptr(t['mthr']), _lib.ptr(t['uthr']), _lib.ptr(gt) if G else None, B, G, _lib.ptr(scratch), _lib.ptr(labels), _lib.ptr(targets),
                        _lib.ptr(weights))
        else:
            _lib.launch("sv_assign_targets_axis_aligned_coded", _lib.ptr(t['anchors']), A, extra, self.sincos, int(bool(self.use_multihead)), t['per_loc'],
                        len(all_anchors), _lib.ptr(t['offs']), _lib.ptr(t['cls']), _lib.ptr(t['mthr']), _lib.ptr(t['uthr']), _lib.ptr(gt) if G else None, B, G,
                        _lib.ptr(scratch), _lib.ptr(labels), _lib.ptr(targets), _lib.ptr(weights))
        return {'box_cls_labels': labels, 'box_reg_targets': targets, 'reg_weights': weights}
