"""Voxel R-CNN second stage: VoxelRCNNHead (+ RoIHeadTemplate, ProposalTargetLayer, NeighborVoxelSAModuleMSG) against a golden produced by the
reference's own classes (tests/golden/make_voxelrcnn_golden.py; CUDA ops of the reference served by the oracle and the voxel-query restatement),
and the whole detector built from the registries."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from seeding import seeded_state_dict
from seevcn_amd.pcdet import model_cfgs as C
from voxelrcnn_inputs import SMALL, TAPS, VOXEL_SIZE, make_inputs

RTOL = 1e-3


def _ok(a, b, rtol=RTOL, atol_frac=1e-4, name=""):
    from tolerances import assert_close_per_channel
    assert_close_per_channel(a, b, rtol=rtol, atol_frac=atol_frac, name=name)
    return True


@pytest.mark.gpu
def test_hip_voxelrcnn_head_matches_reference_golden(golden_dir, cuda, hip_lib, monkeypatch):
    from seevcn_amd.pcdet.models import roi_heads
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules
    g = np.load(os.path.join(golden_dir, "voxelrcnn_head.npz"))
    inp = make_inputs()
    rh = roi_heads.__all__["VoxelRCNNHead"](backbone_channels={k: v[1] for k, v in TAPS.items()}, model_cfg=C.voxelrcnn_cfg(**SMALL),
                                            point_cloud_range=np.array(C.KITTI_RANGE, np.float32), voxel_size=VOXEL_SIZE, num_class=1)
    rh.load_state_dict(seeded_state_dict(rh, seed=13))
    rh.to(cuda)
    t = lambda a: torch.from_numpy(a).to(cuda)

    def batch():
        return {"batch_size": 2, "gt_boxes": t(inp["gt_boxes"]),
                "multi_scale_3d_features": {k: SimpleNamespace(indices=t(inp[k + "_indices"]), features=t(inp[k + "_features"]), spatial_shape=TAPS[k][2],
                                                               batch_size=2) for k in TAPS},
                "multi_scale_3d_strides": {k: v[0] for k, v in TAPS.items()},
                "batch_cls_preds": t(inp["batch_cls_preds"]), "batch_box_preds": t(inp["batch_box_preds"]), "cls_preds_normalized": False}

    rh.train()
    np.random.seed(7)
    torch.manual_seed(7)
    rh(batch())
    fr = rh.forward_ret_dict
    np.testing.assert_allclose(fr["rois"].cpu().numpy(), g["train_rois"], rtol=0, atol=0)           # same NMS survivors, same random sample
    np.testing.assert_allclose(fr["gt_iou_of_rois"].cpu().numpy(), g["gt_iou_of_rois"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(fr["gt_of_rois"].cpu().numpy(), g["gt_of_rois"], rtol=1e-4, atol=1e-4)
    assert np.array_equal(fr["reg_valid_mask"].cpu().numpy(), g["reg_valid_mask"])
    np.testing.assert_allclose(fr["rcnn_cls_labels"].cpu().numpy(), g["rcnn_cls_labels"], rtol=1e-3, atol=1e-4)
    # behind train-mode BatchNorm over 64 RoIs and a 20736-term fp32 contraction: the bounds of test_hip_pvrcnn_heads_match_reference_golden
    assert _ok(fr["rcnn_cls"].detach().cpu().numpy(), g["rcnn_cls"], atol_frac=1e-3, name="rcnn_cls")
    assert _ok(fr["rcnn_reg"].detach().cpu().numpy(), g["rcnn_reg"], atol_frac=1e-3, name="rcnn_reg")
    loss, tb = rh.get_loss()
    for k in ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss_corner", "rcnn_loss"):
        assert abs(tb[k] - float(g[k])) < 1e-3 * abs(float(g[k])), (k, tb[k], float(g[k]))
    loss.backward()
    assert torch.isfinite(rh.shared_fc_layer[0].weight.grad).all() and torch.isfinite(rh.roi_grid_pool_layers[0].mlps_in[0][0].weight.grad).all()
    # eval: once on the fused route, once on the module tree, both held to the golden
    rh.eval()
    for off in (False, True):
        monkeypatch.setattr(voxel_pool_modules, "FUSED_VOXEL_POOL_OFF", off)
        with torch.no_grad():
            bd = rh(batch())
        name = "module tree" if off else "fused"
        np.testing.assert_allclose(bd["rois"].cpu().numpy(), g["eval_rois"], rtol=0, atol=0)
        assert np.array_equal(bd["roi_labels"].cpu().numpy(), g["eval_roi_labels"])
        assert _ok(bd["batch_cls_preds"].cpu().numpy(), g["eval_batch_cls_preds"], atol_frac=1e-3, name=f"eval batch_cls_preds ({name})")
        assert _ok(bd["batch_box_preds"].cpu().numpy(), g["eval_batch_box_preds"], name=f"eval batch_box_preds ({name})")


@pytest.mark.gpu
def test_hip_voxelrcnn_detector_train_step_and_eval(cuda, hip_lib):
    """Full VoxelRCNN built from the registries at reduced sizes: one train step (finite loss and gradients down to the backbone), one eval pass under
    no_grad through the backbone's eval launch list, where the head reads the taps' features lazily."""
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.models import detectors
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=100)
    gt = gt.copy()
    gt[:, :, 7] = np.where(gt[:, :, 3] > 0, 1, 0)                                            # one class
    cfg = C.voxelrcnn_model_cfg(dynamic_vfe=True, roi_per_image=32, nms_post_train=128, nms_pre_train=2048)
    net = detectors.build_detector(cfg, num_class=1, dataset=C.SyntheticDatasetInfo(class_names=C.VOXELRCNN_CLASS_NAMES))
    net.load_state_dict(seeded_state_dict(net, seed=6))
    net = net.to(cuda).train()
    np.random.seed(0)
    torch.manual_seed(0)
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda)}
    ret, tb, _ = net(dict(batch))
    assert torch.isfinite(ret["loss"]) and {"rpn_loss", "rcnn_loss"} <= set(tb)
    ret["loss"].backward()
    for w in (net.roi_head.shared_fc_layer[0].weight, net.backbone_3d.conv3[1][0].weight):
        assert w.grad is not None and torch.isfinite(w.grad).all()
    net.eval()
    with torch.no_grad():
        preds, recall = net(dict(batch))
    assert net.backbone_3d.last_eval_route == 'chain'
    assert len(preds) == 2 and "gt" in recall
    for p in preds:
        n = p["pred_boxes"].shape[0]
        assert p["pred_boxes"].shape == (n, 7) and p["pred_scores"].shape == (n,) and p["pred_labels"].shape == (n,)
        assert torch.isfinite(p["pred_boxes"]).all() and bool((p["pred_labels"] == 1).all())
