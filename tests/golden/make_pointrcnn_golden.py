"""Generate tests/golden/pointrcnn_heads.npz by running the REFERENCE's own PointNet2MSG, PointHeadBox, PointRCNNHead and PointResidualCoder on
the CPU: the state_dict names and shapes of the three modules at pointrcnn.yaml's sizes, the coder's encode / decode values with and without
mean sizes, and PointHeadBox's labels and losses on the seeded inputs of pointrcnn_inputs.py.  The compiled ops under those classes are served
by the oracle (tests/golden/_refimport.py:_install_oracle_ops: points-in-boxes); _refimport makes `.cuda()` an identity, which is all that
PointResidualCoder's constructor needs.  Only recorded results are written.

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_pointrcnn_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refimport as R  # noqa: E402

R.import_pcdet()
from easydict import EasyDict  # noqa: E402
from pcdet.models.backbones_3d.pointnet2_backbone import PointNet2MSG  # noqa: E402
from pcdet.models.dense_heads.point_head_box import PointHeadBox  # noqa: E402
from pcdet.models.roi_heads.pointrcnn_head import PointRCNNHead  # noqa: E402
from pcdet.utils.box_coder_utils import PointResidualCoder  # noqa: E402
from seevcn_amd.pcdet import model_cfgs as C  # noqa: E402
import pointrcnn_inputs as I  # noqa: E402

torch.set_num_threads(8)
out = {}
backbone_cfg, point_cfg, roi_cfg = C.pointrcnn_cfg()
mods = (("names_backbone", PointNet2MSG(EasyDict(backbone_cfg), 4)),
        ("names_point_head", PointHeadBox(num_class=3, input_channels=128, model_cfg=EasyDict(point_cfg), predict_boxes_when_training=True)),
        ("names_roi_head", PointRCNNHead(input_channels=128, model_cfg=EasyDict(roi_cfg), num_class=1)),
        ("names_roi_head_bn", PointRCNNHead(input_channels=128, model_cfg=EasyDict(C.pointrcnn_cfg(use_bn=True)[2]), num_class=1)))
for prefix, mod in mods:
    sd = mod.state_dict()
    out[prefix] = np.array(list(sd.keys()))
    out[prefix + "_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    print(prefix, len(sd))

boxes, points, classes, enc = I.make_coder_inputs()
for tag, coder in (("mean", PointResidualCoder(use_mean_size=True, mean_size=I.MEAN_SIZE)), ("plain", PointResidualCoder(use_mean_size=False))):
    out["coder_enc_" + tag] = coder.encode_torch(torch.from_numpy(boxes.copy()), torch.from_numpy(points), torch.from_numpy(classes)).numpy()
    out["coder_dec_" + tag] = coder.decode_torch(torch.from_numpy(enc), torch.from_numpy(points), torch.from_numpy(classes)).numpy()

inp = I.make_head_inputs()
_, small_point_cfg, _ = C.pointrcnn_cfg(**I.SMALL)
ph = PointHeadBox(num_class=3, input_channels=I.POINT_CHANNELS, model_cfg=EasyDict(small_point_cfg), predict_boxes_when_training=True)
ph.load_state_dict(R.seeded_state_dict(ph, seed=17))
ph.train()
bd = ph({'batch_size': 2, 'gt_boxes': torch.from_numpy(inp['gt_boxes']), 'point_coords': torch.from_numpy(inp['point_coords']),
         'point_features': torch.from_numpy(inp['point_features'])})
loss, tb = ph.get_loss()
fr = ph.forward_ret_dict
out.update(point_cls_labels=fr['point_cls_labels'].numpy(), point_box_labels=fr['point_box_labels'].numpy(),
           point_cls_scores=bd['point_cls_scores'].detach().numpy(), batch_box_preds=bd['batch_box_preds'].detach().numpy(),
           point_loss=np.float32(loss.item()), **{k: np.float32(v) for k, v in tb.items()})
labels = fr['point_cls_labels'].numpy()
print("point head:", tb, {int(v): int((labels == v).sum()) for v in np.unique(labels)})
path = os.path.join(HERE, "pointrcnn_heads.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
