"""Generate tests/golden/parta2_heads.npz by running the REFERENCE's own PointIntraPartOffsetHead and PartA2FCHead (+ RoIHeadTemplate,
ProposalTargetLayer) on the CPU, PartA2.yaml head configuration with reduced sizes (pool 6, two scenes, 32 RoIs, DP_RATIO 0), and record the
state_dict names and shapes of the reference's UNetV2 and both heads.  The compiled ops under those classes are served by the oracle
(tests/golden/_refimport.py:_install_oracle_ops); what the reference takes from spconv and from roiaware_pool3d_cuda.forward gets test-side
stand-ins here, set on the stub modules after import: a submanifold convolution as a dense conv3d read back at the active cells, a minimal
SparseConvTensor with .dense(), SparseSequential, and the numpy restatement of tests/roiaware_pool_reference.py (pinned against the kernels in
tests/test_roiaware_pool.py).

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_parta2_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refimport as R  # noqa: E402

R.import_pcdet()
import roiaware_pool_reference as RP  # noqa: E402


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, **kw):
        self.features, self.indices = features, indices
        self.spatial_shape, self.batch_size = [int(s) for s in spatial_shape], int(batch_size)

    def replace_feature(self, f):
        return SparseConvTensor(f, self.indices, self.spatial_shape, self.batch_size)

    def dense(self):
        out = self.features.new_zeros((self.batch_size, self.features.shape[1], *self.spatial_shape))
        i = self.indices.long()
        out[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = self.features
        return out


class SparseModule(nn.Module):
    pass


class _Conv(SparseModule):
    """Parameters in the spconv 2.x layout (C_out, kz, ky, kx, C_in); only the submanifold kind computes here."""
    subm = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None, **kw):
        super().__init__()
        k = [kernel_size] * 3 if isinstance(kernel_size, int) else list(kernel_size)
        self.weight = nn.Parameter(torch.zeros(out_channels, *k, in_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self.kernel_size = k

    def forward(self, x):
        assert self.subm, "only submanifold convolutions run in the golden"
        y = torch.nn.functional.conv3d(x.dense(), self.weight.permute(0, 4, 1, 2, 3), self.bias, padding=[k // 2 for k in self.kernel_size])
        i = x.indices.long()
        return x.replace_feature(y[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]])


class SubMConv3d(_Conv):
    subm = True


class SparseConv3d(_Conv):
    pass


class SparseInverseConv3d(_Conv):
    pass


class SparseSequential(SparseModule):
    def __init__(self, *mods):
        super().__init__()
        for k, m in enumerate(mods):
            self.add_module(str(k), m)

    def __getitem__(self, k):
        return list(self._modules.values())[k]

    def forward(self, x):
        for m in self._modules.values():
            if isinstance(m, SparseModule):
                x = m(x)
            elif isinstance(x, SparseConvTensor):
                x = x.replace_feature(m(x.features))
            else:
                x = m(x)
        return x


for modname in ("spconv", "spconv.pytorch"):
    for cls in (SparseConvTensor, SparseModule, SubMConv3d, SparseConv3d, SparseInverseConv3d, SparseSequential):
        setattr(sys.modules[modname], cls.__name__, cls)


def roiaware_forward(rois, pts, pts_feature, argmax, pts_idx_of_voxels, pooled_features, pool_method):
    n, ox, oy, oz, cap = pts_idx_of_voxels.shape
    lists = RP.assign(rois.numpy(), pts.numpy(), (ox, oy, oz), cap)
    pooled, arg = RP.pool(lists, pts_feature.detach().numpy(), "max" if pool_method == 0 else "avg")
    pooled_features.copy_(torch.from_numpy(pooled.astype(np.float32)))
    if arg is not None:
        argmax.copy_(torch.from_numpy(arg))
    pts_idx_of_voxels.copy_(torch.from_numpy(np.where(lists == RP.UNSET, 0, lists)))
    return 1


sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"].forward = roiaware_forward
from easydict import EasyDict  # noqa: E402
from pcdet.models.backbones_3d.spconv_unet import UNetV2  # noqa: E402
from pcdet.models.dense_heads.point_intra_part_head import PointIntraPartOffsetHead  # noqa: E402
from pcdet.models.roi_heads.partA2_head import PartA2FCHead  # noqa: E402
from seevcn_amd.pcdet import model_cfgs as C  # noqa: E402
from parta2_inputs import POINT_CHANNELS, SMALL, make_inputs  # noqa: E402

torch.set_num_threads(8)
inp = make_inputs()
point_cfg, roi_cfg = C.parta2_cfg(**SMALL)
ph = PointIntraPartOffsetHead(num_class=1, input_channels=POINT_CHANNELS, model_cfg=EasyDict(point_cfg), predict_boxes_when_training=True)
ph.load_state_dict(R.seeded_state_dict(ph, seed=11))
rh = PartA2FCHead(input_channels=POINT_CHANNELS, model_cfg=EasyDict(roi_cfg), num_class=1)
rh.load_state_dict(R.seeded_state_dict(rh, seed=13))
unet = UNetV2(EasyDict({}), 4, [24, 24, 40], voxel_size=[0.1, 0.1, 0.1], point_cloud_range=[0, 0, 0, 1, 1, 1])


def batch():
    return {'batch_size': 2, 'gt_boxes': torch.from_numpy(inp['gt_boxes']), 'point_coords': torch.from_numpy(inp['point_coords']),
            'point_features': torch.from_numpy(inp['point_features']), 'batch_cls_preds': torch.from_numpy(inp['batch_cls_preds']),
            'batch_box_preds': torch.from_numpy(inp['batch_box_preds']), 'cls_preds_normalized': False}


out = {}
for prefix, mod in (("names_unet", unet), ("names_point_head", ph), ("names_roi_head", rh)):
    sd = mod.state_dict()
    out[prefix] = np.array(list(sd.keys()))
    out[prefix + "_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
ph.train()
rh.train()
bd = ph(batch())
point_loss, tb = ph.get_loss()
fr = ph.forward_ret_dict
out.update(point_cls_labels=fr['point_cls_labels'].numpy(), point_part_labels=fr['point_part_labels'].numpy(),
           point_cls_scores=bd['point_cls_scores'].detach().numpy(), point_part_offset=bd['point_part_offset'].detach().numpy(),
           point_loss=np.float32(point_loss.item()), **{k: np.float32(v) for k, v in tb.items()})
print("train: point", tb, int((fr['point_cls_labels'] > 0).sum()), "foreground of", len(fr['point_cls_labels']))
np.random.seed(7)
torch.manual_seed(7)
bd = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in bd.items()}
rh(bd)
rcnn_loss, tb = rh.get_loss()
fr = rh.forward_ret_dict
out.update(train_rois=fr['rois'].numpy(), train_roi_labels=fr['roi_labels'].numpy(), gt_of_rois=fr['gt_of_rois'].numpy(),
           gt_iou_of_rois=fr['gt_iou_of_rois'].numpy(), reg_valid_mask=fr['reg_valid_mask'].numpy(), rcnn_cls_labels=fr['rcnn_cls_labels'].numpy(),
           rcnn_cls=fr['rcnn_cls'].detach().numpy(), rcnn_reg=fr['rcnn_reg'].detach().numpy(), **{k: np.float32(v) for k, v in tb.items()})
print("train: rcnn", tb)
ph.eval()
rh.eval()
with torch.no_grad():
    bd = rh(ph(batch()))
out.update(eval_rois=bd['rois'].numpy(), eval_roi_labels=bd['roi_labels'].numpy(), eval_batch_cls_preds=bd['batch_cls_preds'].numpy(),
           eval_batch_box_preds=bd['batch_box_preds'].numpy())
np.savez_compressed(os.path.join(HERE, "parta2_heads.npz"), **out)
print("points", inp['point_coords'].shape, "eval rois", bd['rois'].shape, os.path.getsize(os.path.join(HERE, "parta2_heads.npz")))
