"""Validation metrics of the VCN with the reference's names (see/surface_completion/models/vcn/utils/metrics.py).

The reference's Metrics.get evaluates the 6 enabled items over the whole batch and the four num_pts levels by masking the batch and recomputing
every metric per group, one .item() each: 30 values, 30 host reads, the Chamfer search ten times.  Here sv_vc_metrics_objects computes every
per-object quantity once into a (B, COLUMNS) table and sv_vc_metrics_levels folds it into the 30 values: two library calls and one host read
whatever B is.  The arithmetic is stated in tests/vc_metrics_reference.py; csrc/vc_metrics.hip states the summation orders.
"""
import logging

import numpy as np
import torch

from ... import _lib as L
from ... import data_pipeline as P

_counted = P.Counted()
COUNTERS, reset_counters, call, read = _counted.counters, _counted.reset, _counted.call, _counted.read

COLUMNS = 24          # SV_VCM_COLS
MAX_ROWS = 4096       # predicted rows an object (the cloud and its sort live in LDS)
MAX_OBJECTS = 4096    # objects a call of sv_vc_metrics_levels
# table columns (include/seevcn_hip.h)
COL_SUMS, COL_STRIPPED, COL_NZ1, COL_NZ2, COL_BOX, COL_IOU, COL_NUM_OOB, COL_NUM_PC, COL_OOB, COL_ROT, COL_TRANS = 0, 4, 8, 9, 10, 16, 17, 18, 19, 20, 21


def objects_table(coarse, complete, gt_boxes, reg_rot=None, reg_centre=None):
    """The per-object table (B, COLUMNS) fp32 of sv_vc_metrics_objects (integer columns: view(torch.int32)); one library call, no read.
    complete None: the Chamfer columns are skipped."""
    L.require_cuda(gt_boxes)                                   # it is moved to coarse's device below: ptr() would not see where it came from
    as32 = lambda t: None if t is None else t.detach().float().contiguous()
    coarse, complete, gt_boxes, reg_rot, reg_centre = as32(coarse), as32(complete), as32(gt_boxes), as32(reg_rot), as32(reg_centre)
    B, n = coarse.shape[0], coarse.shape[1]
    assert coarse.dim() == 3 and coarse.shape[2] == 3 and gt_boxes.shape == (B, 7), "coarse (B,N,3), gt_boxes (B,7)"
    assert complete is None or (complete.dim() == 3 and complete.shape[0] == B and complete.shape[2] == 3), "complete (B,M,3)"
    assert reg_rot is None or reg_rot.shape == (B, 3, 3), "reg_rot (B,3,3)"
    assert reg_centre is None or reg_centre.shape == (B, 3), "reg_centre (B,3)"
    m = 0 if complete is None else complete.shape[1]
    table = torch.empty((B, COLUMNS), dtype=torch.float32, device=coarse.device)
    call("sv_vc_metrics_objects", L.ptr(coarse), L.ptr(complete), L.ptr(gt_boxes.to(coarse.device)), L.ptr(reg_rot), L.ptr(reg_centre), B, n, m, L.ptr(table))
    return table


def _num_pts_device(num_pts, device):
    """in_dict['num_pts'] as (B,) int32 on the device: a list, a numpy array or a tensor."""
    if isinstance(num_pts, torch.Tensor):
        return num_pts.reshape(-1).to(device=device, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.asarray(num_pts).reshape(-1).astype(np.int32)).to(device)


class Metrics(object):
    ITEMS = [{
        'name': 'F-Score', 'enabled': False, 'eval_func': 'cls._get_f_score', 'is_greater_better': True, 'init_value': 0
    }, {
        'name': 'CDL1', 'enabled': True, 'eval_func': 'cls._get_chamfer_distancel1', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'CDL2', 'enabled': True, 'eval_func': 'cls._get_chamfer_distancel2', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'CDL1_PARTIAL', 'enabled': False, 'eval_func': 'cls._get_chamfer_distancel1_partial', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'CDL2_PARTIAL', 'enabled': False, 'eval_func': 'cls._get_chamfer_distancel2_partial', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'OUT_OF_BOX', 'enabled': True, 'eval_func': 'cls._get_oob_error', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'IOU_3D_Error', 'enabled': False, 'eval_func': 'cls._get_iou_3d_error', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'IOU_3D', 'enabled': True, 'eval_func': 'cls._get_box_iou3d', 'is_greater_better': True, 'init_value': 0
    }, {
        'name': 'IOU_BEV', 'enabled': False, 'eval_func': 'cls._get_box_iou_bev', 'is_greater_better': True, 'init_value': 0
    }, {
        'name': 'Rotation_Error', 'enabled': True, 'eval_func': 'cls._get_rotation_error', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'Translation_Error', 'enabled': True, 'eval_func': 'cls._get_translation_error', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'Axis_Alignment', 'enabled': False, 'eval_func': 'cls._get_axis_alignment', 'is_greater_better': False, 'init_value': 32767
    }, {
        'name': 'Coherence', 'enabled': False, 'eval_func': 'cls._get_coherence', 'is_greater_better': True, 'init_value': 0
    }, {
        'name': 'Cosine_Similarity', 'enabled': False, 'eval_func': 'cls._get_cosine_similarity', 'is_greater_better': True, 'init_value': 0
    }]
    levels = {}
    levels['L1'] = {'min': 201, 'max': 1000000}  # arbitrary max
    levels['L2'] = {'min': 81, 'max': 200}
    levels['L3'] = {'min': 31, 'max': 80}
    levels['L4'] = {'min': 5, 'max': 30}

    # the items the kernels compute, in ITEMS order; the order of sv_vc_metrics_levels' output
    BUILT = ('CDL1', 'CDL2', 'OUT_OF_BOX', 'IOU_3D', 'Rotation_Error', 'Translation_Error')

    @classmethod
    def _check_enabled(cls):
        enabled = [it['name'] for it in cls.ITEMS if it['enabled']]
        for name in enabled:
            if name not in cls.BUILT:
                raise NotImplementedError('Metric %s is not built: the device route computes %s' % (name, ', '.join(cls.BUILT)))
        return enabled

    @classmethod
    def get_device(cls, pred, gt, eval_by_num_pts=True):
        """The values of get() as a device tensor, (30,) or (6,) fp32, without a host read.  pred: 'coarse' (B,N,3) and optionally 'reg_rot' /
        'reg_rot_0' (B,3,3), 'reg_centre' / 'reg_centre_0' (B,3); gt: 'complete' (B,M,3), 'gt_boxes' (B,7), 'num_pts' (B).  pred['pred_box'] is not read: the kernel
        computes get_bbox_from_keypoints(coarse, gt_boxes) itself (table columns 10 .. 15).  pred['pred_box_widened'] (B,7), when present, replaces
        that box in IOU_3D: test_vc's +0.25 on the width, through sv_boxes_iou3d_batch on B sets of one box (one more library call)."""
        enabled = cls._check_enabled()
        coarse = pred['coarse']
        reg_rot = pred.get('reg_rot', pred.get('reg_rot_0'))
        reg_centre = pred.get('reg_centre', pred.get('reg_centre_0'))
        table = objects_table(coarse, gt['complete'], gt['gt_boxes'], reg_rot, reg_centre)
        if pred.get('pred_box_widened') is not None:
            table[:, COL_IOU] = _diagonal_iou3d(pred['pred_box_widened'], gt['gt_boxes'].to(coarse.device))
        B = coarse.shape[0]
        num_pts = _num_pts_device(gt['num_pts'], coarse.device)
        assert num_pts.numel() == B, "num_pts: one count an object"
        out = torch.empty(30, dtype=torch.float32, device=coarse.device)
        call("sv_vc_metrics_levels", L.ptr(table), L.ptr(num_pts), B, L.ptr(out))
        if len(enabled) != len(cls.BUILT):
            out = out.view(6, 5)[[cls.BUILT.index(name) for name in enabled]].reshape(-1)
        return out if eval_by_num_pts else out.view(-1, 5)[:, 0].contiguous()

    @classmethod
    def get(cls, pred, gt, eval_by_num_pts=True):
        """The reference's list of Python floats: 30 values in names() order, or the 6 whole-batch values.  Two library calls, one host read."""
        return [float(v) for v in read(cls.get_device(pred, gt, eval_by_num_pts))]

    @classmethod
    def items(cls, eval_by_num_pts=True):
        if eval_by_num_pts:
            items = []
            for it in cls.ITEMS:
                if it['enabled']:
                    items.append(it)
                    base_name = it['name']
                    for level in cls.levels.keys():
                        it_copy = {key: value for key, value in it.items()}
                        it_copy['name'] = base_name + f'_{level}'
                        it_copy['min_pts'] = cls.levels[level]['min']
                        it_copy['max_pts'] = cls.levels[level]['max']
                        items.append(it_copy)
            return items
        else:
            return [i for i in cls.ITEMS if i['enabled']]

    @classmethod
    def names(cls, eval_by_num_pts=True):
        return [i['name'] for i in cls.items()]

    def __init__(self, metric_name, values):
        self._items = Metrics.items()
        self._values = [item['init_value'] for item in self._items]
        self.metric_name = metric_name

        if type(values).__name__ == 'list':
            self._values = values
        elif type(values).__name__ == 'dict':
            metric_indexes = {}
            for idx, item in enumerate(self._items):
                item_name = item['name']
                metric_indexes[item_name] = idx
            for k, v in values.items():
                if k not in metric_indexes:
                    logging.warning('Ignore Metric[Name=%s] due to disability.' % k)
                    continue
                self._values[metric_indexes[k]] = v
        else:
            raise Exception('Unsupported value type: %s' % type(values))

    def state_dict(self):
        _dict = dict()
        for i in range(len(self._items)):
            item = self._items[i]['name']
            value = self._values[i]
            _dict[item] = value

        return _dict

    def __repr__(self):
        return str(self.state_dict())

    def better_than(self, other):
        if other is None:
            return True

        _index = -1
        for i, _item in enumerate(self._items):
            if _item['name'] == self.metric_name:
                _index = i
                break
        if _index == -1:
            raise Exception('Invalid metric name to compare.')

        _metric = self._items[i]
        _value = self._values[_index]
        other_value = other._values[_index]
        return _value > other_value if _metric['is_greater_better'] else _value < other_value


def _diagonal_iou3d(boxes_a, boxes_b):
    """(B,7), (B,7) -> (B,) 3-D IoU of pair i with pair i: B box sets of one box each through sv_boxes_iou3d_batch (no B x B matrix)."""
    a, b = boxes_a.detach().float().contiguous(), boxes_b.detach().float().contiguous()
    out = torch.empty(len(a), dtype=torch.float32, device=a.device)
    call("sv_boxes_iou3d_batch", L.ptr(a), 1, 7, L.ptr(b), 1, 7, len(a), L.ptr(out))
    return out
