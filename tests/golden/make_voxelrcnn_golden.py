"""Generate tests/golden/voxelrcnn_head.npz by running the REFERENCE's own VoxelRCNNHead (+ RoIHeadTemplate, ProposalTargetLayer,
NeighborVoxelSAModuleMSG, VoxelQueryAndGrouping) on CPU, voxel_rcnn_car.yaml head configuration with reduced sizes.  The compiled CUDA ops under
those classes are served by the oracle (tests/golden/_refimport.py:_install_oracle_ops); voxel_query_wrapper, which the oracle does not have, by
the restatement in tests/voxel_pool_reference.py (pinned against the kernel in tests/test_voxel_pool.py).

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_voxelrcnn_golden.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refimport as R  # noqa: E402

R.import_pcdet()
import voxel_pool_reference as VR  # noqa: E402


def voxel_query_wrapper(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx):
    VR.voxel_query([z_range, y_range, x_range], radius, nsample, xyz.numpy(), new_xyz.numpy(), new_coords.numpy(), point_indices.numpy(), idx=idx.numpy())
    return 1


sys.modules["pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"].voxel_query_wrapper = voxel_query_wrapper
from easydict import EasyDict  # noqa: E402
from pcdet.models.roi_heads.voxelrcnn_head import VoxelRCNNHead  # noqa: E402
from seevcn_amd.pcdet import model_cfgs as C  # noqa: E402
from voxelrcnn_inputs import SMALL, TAPS, VOXEL_SIZE, make_inputs  # noqa: E402

torch.set_num_threads(8)
inp = make_inputs()
rh = VoxelRCNNHead(backbone_channels={k: v[1] for k, v in TAPS.items()}, model_cfg=EasyDict(C.voxelrcnn_cfg(**SMALL)),
                   point_cloud_range=np.array(C.KITTI_RANGE, np.float32), voxel_size=VOXEL_SIZE, num_class=1)
rh.load_state_dict(R.seeded_state_dict(rh, seed=13))


def batch():
    return {
        'batch_size': 2, 'gt_boxes': torch.from_numpy(inp['gt_boxes']),
        'multi_scale_3d_features': {k: SimpleNamespace(indices=torch.from_numpy(inp[k + '_indices']), features=torch.from_numpy(inp[k + '_features']),
                                                       spatial_shape=TAPS[k][2], batch_size=2) for k in TAPS},
        'multi_scale_3d_strides': {k: v[0] for k, v in TAPS.items()},
        'batch_cls_preds': torch.from_numpy(inp['batch_cls_preds']), 'batch_box_preds': torch.from_numpy(inp['batch_box_preds']),
        'cls_preds_normalized': False,
    }


out = {}
rh.train()
np.random.seed(7)
torch.manual_seed(7)
rh(batch())
rcnn_loss, tb = rh.get_loss()
fr = rh.forward_ret_dict
out.update(train_rois=fr['rois'].numpy(), gt_of_rois=fr['gt_of_rois'].numpy(), gt_iou_of_rois=fr['gt_iou_of_rois'].numpy(),
           reg_valid_mask=fr['reg_valid_mask'].numpy(), rcnn_cls_labels=fr['rcnn_cls_labels'].numpy(), rcnn_cls=fr['rcnn_cls'].detach().numpy(),
           rcnn_reg=fr['rcnn_reg'].detach().numpy(), **{k: np.float32(v) for k, v in tb.items()})
print("train: rcnn", tb)
rh.eval()
with torch.no_grad():
    bd = rh(batch())
out.update(eval_rois=bd['rois'].numpy(), eval_roi_labels=bd['roi_labels'].numpy(), eval_batch_cls_preds=bd['batch_cls_preds'].numpy(),
           eval_batch_box_preds=bd['batch_box_preds'].numpy())
np.savez_compressed(os.path.join(HERE, "voxelrcnn_head.npz"), **out)
print("eval rois", bd['rois'].shape, os.path.getsize(os.path.join(HERE, "voxelrcnn_head.npz")))
