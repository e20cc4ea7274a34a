"""Part-A2: UNetV2 against the float64 restatement of tests/unet_reference.py (eval values, train-mode gradients), the registries and
state_dict names, and the detector built from the registries (one train step, one eval pass)."""
import functools
import os

import numpy as np
import pytest
import torch

import unet_reference as UR
from oracle.tolerances import assert_close_per_channel
from seeding import seeded_state_dict
from seevcn_amd.pcdet import model_cfgs as C
from parta2_inputs import POINT_CHANNELS, SMALL, make_inputs

GRID_SIZE = [24, 24, 40]                 # x, y, z: the sparse shape [41, 24, 24] goes 41 -> 21 -> 11 -> 5 -> 2 along z
RANGE = [0.0, -1.2, -3.0, 2.4, 1.2, 1.0]
VOXEL = [0.1, 0.1, 0.1]


def _unet():
    from seevcn_amd.pcdet.models import backbones_3d
    m = backbones_3d.__all__["UNetV2"]({}, 4, np.array(GRID_SIZE), voxel_size=VOXEL, point_cloud_range=np.array(RANGE, np.float32))
    sd = seeded_state_dict(m, seed=4)
    m.load_state_dict(sd)
    return m, sd


@functools.lru_cache(maxsize=None)
def _voxels():
    """Two scenes, a few hundred voxels each, clustered so that every level keeps neighbours; rows of a scene in a seeded random order."""
    rng = np.random.default_rng(8)
    rows = []
    for b in range(2):
        centres = rng.uniform([4, 3, 3], [37, 21, 21], (6, 3))
        p = np.concatenate([c + rng.normal(0, 1.6, (90, 3)) for c in centres])
        p = np.unique(np.clip(np.round(p), 0, [40, 23, 23]).astype(np.int32), axis=0)
        p = p[rng.permutation(len(p))]
        rows.append(np.concatenate([np.full((len(p), 1), b, np.int32), p], 1))
    coords = np.concatenate(rows).astype(np.int32)
    feats = rng.standard_normal((len(coords), 4)).astype(np.float32)
    return coords, feats


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_registries_and_state_dict_names():
    from seevcn_amd.pcdet.models import backbones_3d, dense_heads, detectors, roi_heads
    assert "UNetV2" in backbones_3d.__all__ and "PointIntraPartOffsetHead" in dense_heads.__all__
    assert "PartA2FCHead" in roi_heads.__all__ and "PartA2Net" in detectors.__all__
    m, sd = _unet()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert m.num_point_features == 16 and m.sparse_shape == [41, 24, 24]
    # the reference's names (spconv_unet.py:64-132) and the spconv 2.x weight layout (C_out, kz, ky, kx, C_in)
    assert shapes["conv_input.0.weight"] == (16, 3, 3, 3, 4) and shapes["conv1.0.0.weight"] == (16, 3, 3, 3, 16)
    assert shapes["conv4.0.0.weight"] == (64, 3, 3, 3, 64) and shapes["conv_out.0.weight"] == (128, 3, 1, 1, 64)
    assert shapes["conv_up_t4.conv1.weight"] == (64, 3, 3, 3, 64) and "conv_up_t4.conv1.bias" not in shapes
    assert shapes["conv_up_m4.0.weight"] == (64, 3, 3, 3, 128) and shapes["conv_up_m2.0.weight"] == (32, 3, 3, 3, 64)
    assert shapes["inv_conv4.0.weight"] == (64, 3, 3, 3, 64) and shapes["inv_conv3.0.weight"] == (32, 3, 3, 3, 64)
    assert shapes["inv_conv2.0.weight"] == (16, 3, 3, 3, 32) and shapes["conv5.0.0.weight"] == (16, 3, 3, 3, 16)
    assert shapes["inv_conv2.1.running_var"] == (16,) and shapes["conv_up_t1.bn2.weight"] == (16,)
    convs = [k for k in shapes if k.endswith(".weight") and len(shapes[k]) == 5]
    assert len(convs) == 12 + 4 * 3 + 3 + 1 and len(shapes) == len(convs) + 5 * len(convs)      # every conv has one BatchNorm1d behind it
    no_encoded = backbones_3d.__all__["UNetV2"]({"RETURN_ENCODED_TENSOR": False}, 4, np.array(GRID_SIZE), voxel_size=VOXEL, point_cloud_range=RANGE)
    assert no_encoded.conv_out is None


def test_detector_builds_from_registries():
    from seevcn_amd.pcdet.models import detectors
    cfg = C.parta2_model_cfg(pool_size=6, roi_per_image=32)
    assert cfg["BACKBONE_3D"]["NAME"] == "UNetV2" and cfg["ROI_HEAD"]["ROI_AWARE_POOL"] == dict(POOL_SIZE=6, NUM_FEATURES=128, MAX_POINTS_PER_VOXEL=128)
    full = C.parta2_model_cfg()["ROI_HEAD"]
    assert full["ROI_AWARE_POOL"]["POOL_SIZE"] == 12 and full["SHARED_FC"] == [256, 256, 256] and full["TARGET_CONFIG"]["REG_FG_THRESH"] == 0.65
    net = detectors.build_detector(cfg, num_class=3, dataset=C.SyntheticDatasetInfo(num_point_features=4))
    assert [type(m).__name__ for m in net.module_list] == ["MeanVFE", "UNetV2", "HeightCompression", "BaseBEVBackbone", "AnchorHeadSingle",
                                                           "PointIntraPartOffsetHead", "PartA2FCHead"]
    assert net.LOSS_HEADS == ("dense_head", "point_head", "roi_head")
    sd = net.state_dict()
    assert tuple(sd["point_head.cls_layers.0.weight"].shape) == (1, 16) and tuple(sd["point_head.part_reg_layers.0.weight"].shape) == (3, 16)
    assert tuple(sd["roi_head.conv_part.0.0.weight"].shape) == (64, 3, 3, 3, 4) and tuple(sd["roi_head.conv_rpn.0.0.weight"].shape) == (64, 3, 3, 3, 16)
    assert tuple(sd["roi_head.shared_fc_layer.0.weight"].shape) == (256, 128 * 6 ** 3, 1) and tuple(sd["roi_head.reg_layers.7.weight"].shape) == (7, 256, 1)


def test_point_part_labels_cpu_restatement():
    """ret_part_labels is additive: the class labels are what PointHeadSimple gets; a foreground point's part label is its position in the box
    frame over the box's extent + 0.5."""
    from seevcn_amd.pcdet.utils import common_utils
    box = torch.tensor([[1.0, 2.0, 0.0, 4.0, 2.0, 2.0, 0.5, 1.0]])
    local = torch.tensor([[1.0, 0.5, -0.5], [-1.9, -0.9, 0.9]])
    pts = common_utils.rotate_points_along_z(local.view(1, -1, 3), box[:, 6]).view(-1, 3) + box[:, 0:3]
    back = common_utils.rotate_points_along_z((pts - box[:, 0:3]).view(-1, 1, 3), -box[:, 6].expand(2)).view(-1, 3)
    assert torch.allclose(back / box[:, 3:6] + 0.5, torch.tensor([[0.75, 0.75, 0.25], [0.025, 0.05, 0.95]]), atol=1e-6)


def test_state_dict_names_match_the_reference(golden_dir):
    """Names and shapes recorded from the reference's own UNetV2, PointIntraPartOffsetHead and PartA2FCHead (make_parta2_golden.py)."""
    from seevcn_amd.pcdet.models import dense_heads, roi_heads
    g = np.load(os.path.join(golden_dir, "parta2_heads.npz"))
    point_cfg, roi_cfg = C.parta2_cfg(**SMALL)
    ours = {"names_unet": _unet()[0],
            "names_point_head": dense_heads.__all__["PointIntraPartOffsetHead"](num_class=1, input_channels=POINT_CHANNELS, model_cfg=point_cfg),
            "names_roi_head": roi_heads.__all__["PartA2FCHead"](input_channels=POINT_CHANNELS, model_cfg=roi_cfg, num_class=1)}
    for key, mod in ours.items():
        want = dict(zip(g[key].tolist(), g[key + "_shapes"].tolist()))
        got = {k: ",".join(str(s) for s in v.shape) for k, v in mod.state_dict().items()}
        assert got == want, (key, sorted(set(got) ^ set(want))[:10])
        assert list(got) == g[key].tolist()                                   # the same order, too


# ---------------------------------------------------------------------------------------------------------------- GPU
def _heads(cuda):
    from seevcn_amd.pcdet.models import dense_heads, roi_heads
    point_cfg, roi_cfg = C.parta2_cfg(**SMALL)
    ph = dense_heads.__all__["PointIntraPartOffsetHead"](num_class=1, input_channels=POINT_CHANNELS, model_cfg=point_cfg, predict_boxes_when_training=True)
    ph.load_state_dict(seeded_state_dict(ph, seed=11))
    rh = roi_heads.__all__["PartA2FCHead"](input_channels=POINT_CHANNELS, model_cfg=roi_cfg, num_class=1)
    rh.load_state_dict(seeded_state_dict(rh, seed=13))
    return ph.to(cuda), rh.to(cuda)


def _head_batch(cuda, inp, **replace):
    keys = ("gt_boxes", "point_coords", "point_features", "batch_cls_preds", "batch_box_preds")
    bd = {"batch_size": 2, "cls_preds_normalized": False, **{k: torch.from_numpy(inp[k]).to(cuda) for k in keys}}
    bd.update(replace)
    return bd


@pytest.mark.gpu
@pytest.mark.parametrize("stacked", [True, False])
def test_heads_match_reference_golden(golden_dir, cuda, hip_lib, stacked):
    """Point targets and losses, the sampled RoIs, labels, rcnn_cls / rcnn_reg and losses in train mode, box predictions in eval mode, against
    the reference's own classes.  stacked = False shuffles the points across scenes: the head then takes the per-scene loop."""
    g = np.load(os.path.join(golden_dir, "parta2_heads.npz"))
    inp = make_inputs()
    perm = torch.from_numpy(np.random.default_rng(1).permutation(len(inp["point_coords"]))).to(cuda)

    def for_roi_head(bd):
        """detached, and with stacked = False the point rows (the point head wants them stacked) shuffled across the scenes"""
        bd = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in bd.items()}
        if not stacked:
            for k in ("point_coords", "point_features", "point_cls_scores", "point_part_offset"):
                bd[k] = bd[k][perm].contiguous()
        return bd

    ph, rh = _heads(cuda)
    ph.train()
    rh.train()
    bd = ph(_head_batch(cuda, inp))
    fr = ph.forward_ret_dict
    assert np.array_equal(fr["point_cls_labels"].cpu().numpy(), g["point_cls_labels"])
    np.testing.assert_allclose(fr["point_part_labels"].cpu().numpy(), g["point_part_labels"], rtol=1e-4, atol=1e-5)
    assert_close_per_channel(bd["point_part_offset"].detach().cpu().numpy(), g["point_part_offset"], name="point_part_offset")
    np.testing.assert_allclose(bd["point_cls_scores"].detach().cpu().numpy(), g["point_cls_scores"], rtol=1e-3, atol=1e-5)
    loss, tb = ph.get_loss()
    for k in ("point_loss_cls", "point_loss_part", "point_pos_num"):
        assert abs(float(tb[k]) - float(g[k])) <= 1e-3 * abs(float(g[k])), (k, tb[k], float(g[k]))
    assert abs(float(loss) - float(g["point_loss"])) <= 1e-3 * float(g["point_loss"])
    np.random.seed(7)
    torch.manual_seed(7)
    rh(for_roi_head(bd))
    fr = rh.forward_ret_dict
    np.testing.assert_allclose(fr["rois"].cpu().numpy(), g["train_rois"], rtol=0, atol=0)            # same NMS survivors, same random sample
    assert np.array_equal(fr["roi_labels"].cpu().numpy(), g["train_roi_labels"])
    np.testing.assert_allclose(fr["gt_iou_of_rois"].cpu().numpy(), g["gt_iou_of_rois"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(fr["gt_of_rois"].cpu().numpy(), g["gt_of_rois"], rtol=1e-4, atol=1e-4)
    assert np.array_equal(fr["reg_valid_mask"].cpu().numpy(), g["reg_valid_mask"])
    np.testing.assert_allclose(fr["rcnn_cls_labels"].cpu().numpy(), g["rcnn_cls_labels"], rtol=1e-3, atol=1e-4)
    # behind train-mode BatchNorm over 32 RoIs and a 6912-term fp32 contraction: the bounds of test_hip_voxelrcnn_head_matches_reference_golden
    assert_close_per_channel(fr["rcnn_cls"].detach().cpu().numpy(), g["rcnn_cls"], atol_frac=1e-3, name="rcnn_cls")
    assert_close_per_channel(fr["rcnn_reg"].detach().cpu().numpy(), g["rcnn_reg"], atol_frac=1e-3, name="rcnn_reg")
    loss, tb = rh.get_loss()
    for k in ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss_corner", "rcnn_loss"):
        assert abs(tb[k] - float(g[k])) < 1e-3 * abs(float(g[k])), (k, tb[k], float(g[k]))
    loss.backward()
    assert torch.isfinite(rh.conv_part[0][0].weight.grad).all() and torch.isfinite(rh.conv_rpn[0][0].weight.grad).all()
    ph.eval()
    rh.eval()
    with torch.no_grad():
        bd = rh(for_roi_head(ph(_head_batch(cuda, inp))))
    np.testing.assert_allclose(bd["rois"].cpu().numpy(), g["eval_rois"], rtol=0, atol=0)
    assert np.array_equal(bd["roi_labels"].cpu().numpy(), g["eval_roi_labels"])
    assert_close_per_channel(bd["batch_cls_preds"].cpu().numpy(), g["eval_batch_cls_preds"], atol_frac=1e-3, name="eval batch_cls_preds")
    assert_close_per_channel(bd["batch_box_preds"].cpu().numpy(), g["eval_batch_box_preds"], name="eval batch_box_preds")


@pytest.mark.gpu
def test_every_roi_empty_takes_the_fake_index_path(cuda, hip_lib):
    """No point inside any RoI: fewer than 3 non-empty cells, the first cell of every RoI stands in and the targets are marked invalid."""
    inp = make_inputs()
    far = inp["point_coords"].copy()
    far[:, 3] += 50.0                                                          # 50 m above every box
    ph, rh = _heads(cuda)
    ph.train()
    rh.train()
    np.random.seed(7)
    torch.manual_seed(7)
    bd = ph(_head_batch(cuda, dict(inp, point_coords=far)))
    rh({k: (v.detach() if torch.is_tensor(v) else v) for k, v in bd.items()})
    fr = rh.forward_ret_dict
    assert bool((fr["rcnn_cls_labels"] == -1).all()) and bool((fr["reg_valid_mask"] == -1).all())
    assert fr["rcnn_cls"].shape == (32, 1) and fr["rcnn_reg"].shape == (32, 7) and torch.isfinite(fr["rcnn_cls"]).all()
    loss, tb = rh.get_loss()
    assert torch.isfinite(loss) and tb["rcnn_loss_cls"] == 0
@pytest.mark.gpu
def test_unet_eval_against_float64(cuda):
    coords, feats = _voxels()
    m, sd = _unet()
    m = m.to(cuda).eval()
    with torch.no_grad():
        bd = m({"batch_size": 2, "voxel_features": torch.from_numpy(feats).to(cuda), "voxel_coords": torch.from_numpy(coords).to(cuda)})
    ref = UR.UNetV2Reference(sd, coords, m.sparse_shape, training=False)
    with torch.no_grad():
        want = ref.forward(torch.from_numpy(feats))
    assert_close_per_channel(bd["point_features"].cpu().numpy(), want["point_features"].numpy(), name="point_features")
    xyz = (coords[:, [3, 2, 1]].astype(np.float64) + 0.5) * np.array(VOXEL) + np.array(RANGE[:3])
    pc = bd["point_coords"].cpu().numpy()
    assert np.array_equal(pc[:, 0], coords[:, 0].astype(np.float32))
    np.testing.assert_allclose(pc[:, 1:], xyz, rtol=0, atol=1e-5)
    enc = bd["encoded_spconv_tensor"]
    assert bd["encoded_spconv_tensor_stride"] == 8 and list(enc.spatial_shape) == [2, 3, 3] == list(want["encoded_shape"])
    assert np.array_equal(enc.indices.cpu().numpy(), want["encoded_coords"])
    assert_close_per_channel(enc.features.cpu().numpy(), want["encoded"].numpy(), name="encoded_spconv_tensor")


@pytest.mark.gpu
def test_unet_train_gradients_against_float64(cuda):
    """One train-mode forward and backward; loss = <point_features, G> + <encoded features, H>.  Bound of the gradients: rtol 2e-3, atol_frac
    5e-4, what smoke() and the sparse conv tests hold fp32 weight gradients to against float64."""
    coords, feats = _voxels()
    m, sd = _unet()
    m = m.to(cuda).train()
    bd = m({"batch_size": 2, "voxel_features": torch.from_numpy(feats).to(cuda), "voxel_coords": torch.from_numpy(coords).to(cuda)})
    g = torch.Generator().manual_seed(3)
    G = torch.randn(bd["point_features"].shape, generator=g)
    H = torch.randn(bd["encoded_spconv_tensor"].features.shape, generator=g)
    ((bd["point_features"] * G.to(cuda)).sum() + (bd["encoded_spconv_tensor"].features * H.to(cuda)).sum()).backward()
    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    ref = UR.UNetV2Reference(sd64, coords, m.sparse_shape, training=True)
    want = ref.forward(torch.from_numpy(feats))
    assert_close_per_channel(bd["point_features"].detach().cpu().numpy(), want["point_features"].detach().numpy(), name="train point_features")
    ((want["point_features"] * G.double()).sum() + (want["encoded"] * H.double()).sum()).backward()
    from oracle import spconv as osp
    for name in ("conv_input.0.weight", "inv_conv3.0.weight"):
        got = dict(m.named_parameters())[name].grad.cpu().numpy()
        assert_close_per_channel(osp.weight_to_kio(got), osp.weight_to_kio(sd64[name].grad.numpy()), rtol=2e-3, atol_frac=5e-4, name=f"gradient of {name}")


@pytest.mark.gpu
def test_parta2_detector_train_step_and_eval(cuda, hip_lib):
    """PartA2Net from the registries at reduced sizes: one train step with finite losses of every head and a gradient on every parameter, one eval
    pass with the pred_dicts contract."""
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.models import detectors
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=60)
    cfg = C.parta2_model_cfg(dynamic_vfe=True, pool_size=6, roi_per_image=32, nms_post_train=128, nms_pre_train=2048, shared_fc=(64, 64), num_features=32)
    net = detectors.build_detector(cfg, num_class=3, dataset=C.SyntheticDatasetInfo())
    net.load_state_dict(seeded_state_dict(net, seed=6))
    net = net.to(cuda).train()
    np.random.seed(0)
    torch.manual_seed(0)
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda)}
    ret, tb, _ = net(dict(batch))
    assert torch.isfinite(ret["loss"])
    assert {"rpn_loss", "point_loss_cls", "point_loss_part", "rcnn_loss"} <= set(tb) and all(np.isfinite(tb[k]) for k in tb), tb
    ret["loss"].backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    net.eval()
    with torch.no_grad():
        preds, recall = net(dict(batch))
    assert len(preds) == 2 and "gt" in recall
    for p in preds:
        n = p["pred_boxes"].shape[0]
        assert p["pred_boxes"].shape == (n, 7) and p["pred_scores"].shape == (n,) and p["pred_labels"].shape == (n,)
        assert torch.isfinite(p["pred_boxes"]).all() and bool(((p["pred_labels"] >= 1) & (p["pred_labels"] <= 3)).all())
