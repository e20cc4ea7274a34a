"""VoxelBackBone8xFocal from the registry and the Voxel R-CNN detector built on it (model_cfgs.voxelrcnn_focal_model_cfg: the MODEL section of
kitti_models/voxel_rcnn_car_focal_multimodal.yaml with USE_IMG: False): one train step, one eval pass, and the size of the expanded taps against
VoxelBackBone8x on the same input."""
import numpy as np
import pytest
import torch

from seeding import seeded_state_dict
from seevcn_amd.pcdet import model_cfgs as C


def test_registry_resolves_focal_backbone_and_cfg():
    from seevcn_amd.pcdet.models import backbones_3d
    from seevcn_amd.pcdet.models.backbones_3d.spconv_backbone_focal import SparseSequentialBatchdict, VoxelBackBone8xFocal
    assert backbones_3d.__all__["VoxelBackBone8xFocal"] is VoxelBackBone8xFocal
    cfg = C.voxelrcnn_focal_model_cfg()
    plain = C.voxelrcnn_model_cfg()
    assert cfg["BACKBONE_3D"] == dict(NAME="VoxelBackBone8xFocal", USE_IMG=False)
    assert {k: v for k, v in cfg.items() if k != "BACKBONE_3D"} == {k: v for k, v in plain.items() if k != "BACKBONE_3D"}
    m = VoxelBackBone8xFocal(cfg["BACKBONE_3D"], 4, [1408, 1600, 40])
    assert m.sparse_shape == [41, 1600, 1408] and m.num_point_features == 128
    assert m.backbone_channels == {"x_conv1": 16, "x_conv2": 32, "x_conv3": 64, "x_conv4": 64}
    assert all(isinstance(getattr(m, n), SparseSequentialBatchdict) for n in ("conv1", "conv2", "conv3", "conv4"))
    keys = set(m.state_dict())
    for stage, slot, key in (("conv1", 1, "focal1"), ("conv2", 3, "focal2"), ("conv3", 3, "focal3")):
        layer = getattr(m, stage)[slot]
        assert layer.conv.indice_key == key and layer.conv_imp.indice_key == key + "_imp" and layer.conv_enlarge is None
        assert layer.topk is True and layer.threshold == 0.5 and layer.mask_multi is False and layer.skip_mask_kernel is False
        assert {f"{stage}.{slot}.conv.weight", f"{stage}.{slot}.bn1.weight", f"{stage}.{slot}.conv_imp.weight"} <= keys
    assert tuple(m.conv2[3].conv_imp.weight.shape) == (27, 3, 3, 3, 32)
    with pytest.raises(NotImplementedError, match="DeepLabV3"):
        VoxelBackBone8xFocal(dict(NAME="VoxelBackBone8xFocal", USE_IMG=True), 4, [1408, 1600, 40])
    with pytest.raises(NotImplementedError, match="kernel_size"):
        VoxelBackBone8xFocal(dict(NAME="VoxelBackBone8xFocal", KERNEL_SIZE=5), 4, [1408, 1600, 40])


def _scene_batch(cuda):
    import seevcn_amd.synth as synth
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=100)
    gt = gt.copy()
    gt[:, :, 7] = np.where(gt[:, :, 3] > 0, 1, 0)                                            # one class
    return {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda)}


@pytest.mark.gpu
def test_hip_voxelrcnn_focal_detector_train_step_and_eval(cuda, hip_lib):
    from seevcn_amd.pcdet.models import detectors
    cfg = C.voxelrcnn_focal_model_cfg(dynamic_vfe=True, roi_per_image=32, nms_post_train=128, nms_pre_train=2048)
    net = detectors.build_detector(cfg, num_class=1, dataset=C.SyntheticDatasetInfo(class_names=C.VOXELRCNN_CLASS_NAMES))
    net.load_state_dict(seeded_state_dict(net, seed=6))
    net = net.to(cuda).train()
    np.random.seed(0)
    torch.manual_seed(0)
    batch = _scene_batch(cuda)
    ret, tb, _ = net(dict(batch))
    assert torch.isfinite(ret["loss"]) and {"rpn_loss", "rcnn_loss", "loss_box_of_pts"} <= set(tb)
    assert isinstance(tb["loss_box_of_pts"], float) and tb["loss_box_of_pts"] > 0
    ret["loss"].backward()
    bb = net.backbone_3d
    for layer in (bb.conv1[1], bb.conv2[3], bb.conv3[3]):
        for name, p in layer.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any()), name
    net.eval()
    with torch.no_grad():
        preds, recall = net(dict(batch))
    assert len(preds) == 2 and "gt" in recall
    for p in preds:
        n = p["pred_boxes"].shape[0]
        assert p["pred_boxes"].shape == (n, 7) and p["pred_scores"].shape == (n,) and p["pred_labels"].shape == (n,)
        assert torch.isfinite(p["pred_boxes"]).all() and bool((p["pred_labels"] == 1).all())


@pytest.mark.gpu
def test_hip_focal_backbone_taps_against_plain_backbone(cuda, hip_lib):
    """multi_scale_3d_features of the focal backbone have at least the rows of VoxelBackBone8x's at conv1-3 on the same input, and exactly as many
    when nothing is foreground (threshold mode, THRESHOLD 2.0)."""
    from seevcn_amd.pcdet.models import backbones_3d
    from seevcn_amd.pcdet.ops import voxel_ops
    batch = _scene_batch(cuda)
    pts = batch["points"]
    feats, coords, _ = voxel_ops.voxelize_dynamic(pts.contiguous(), C.KITTI_RANGE, [0.05, 0.05, 0.1], [1408, 1600, 40], 2)
    rows = {}
    for name, cfg in (("plain", {}), ("focal", dict(USE_IMG=False)), ("nothing", dict(USE_IMG=False, TOPK=False, THRESHOLD=2.0))):
        m = backbones_3d.__all__["VoxelBackBone8x" if name == "plain" else "VoxelBackBone8xFocal"](cfg, feats.shape[1], [1408, 1600, 40])
        m.load_state_dict(seeded_state_dict(m, seed=4))
        m = m.to(cuda).eval()
        with torch.no_grad():
            bd = m({"batch_size": 2, "voxel_features": feats, "voxel_coords": coords})
        rows[name] = {k: int(v.indices.shape[0]) for k, v in bd["multi_scale_3d_features"].items()}
        assert bd["encoded_spconv_tensor_stride"] == 8 and bd["multi_scale_3d_strides"] == {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8}
        for k, v in bd["multi_scale_3d_features"].items():
            assert v.features.shape == (rows[name][k], m.backbone_channels[k]) and torch.isfinite(v.features).all()
    print(rows)
    for k in ("x_conv1", "x_conv2", "x_conv3"):
        assert rows["focal"][k] >= rows["plain"][k] and rows["nothing"][k] == rows["plain"][k]
    assert rows["focal"]["x_conv1"] > rows["plain"]["x_conv1"]
    assert rows["nothing"]["x_conv4"] == rows["plain"]["x_conv4"]
