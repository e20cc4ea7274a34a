"""CaDDN's modules on the GPU: ImageVFE (with a two-convolution stub DDN) against the float64 CPU restatement of tests/caddn_reference.py with the
same weights, Conv2DCollapse on the fused kernel's storage order and on a plain copy, and the small caddn_model_cfg detector end to end."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import caddn_reference as R
from oracle.tolerances import assert_close_per_channel
from seevcn_amd.pcdet import model_cfgs as M
from seevcn_amd.pcdet.models import detectors
from seevcn_amd.pcdet.models.backbones_2d import map_to_bev
from seevcn_amd.pcdet.models.backbones_3d import vfe
from seevcn_amd.pcdet.models.backbones_3d.vfe.image_vfe_modules.ffn import ddn

pytestmark = pytest.mark.gpu


class StubDDN(nn.Module):
    """features = a stride-4 convolution of the image, logits = a 3x3 convolution of the features"""

    def __init__(self, num_classes, backbone_name=None, feat_channels=12):
        super().__init__()
        self.features = nn.Conv2d(3, feat_channels, 5, stride=4, padding=2)
        self.logits = nn.Conv2d(feat_channels, num_classes, 3, padding=1)

    def forward(self, images):
        f = torch.tanh(self.features(images))
        return {"features": f, "logits": 2.0 * self.logits(f)}


DISC = dict(mode="LID", num_bins=7, depth_min=2.0, depth_max=11.0)
GRID, RANGE = (11, 10, 3), (1., -6., -2., 12., 6., 1.)


def _vfe_cfg():
    return dict(NAME="ImageVFE",
                FFN=dict(NAME="DepthFFN", DDN=dict(NAME="StubDDN", BACKBONE_NAME=None, ARGS=dict(feat_channels=12)),
                         CHANNEL_REDUCE=dict(in_channels=12, out_channels=6, kernel_size=1, stride=1, bias=False), DISCRETIZE=DISC,
                         LOSS=dict(NAME="DDNLoss", ARGS=dict(weight=3.0, alpha=0.25, gamma=2.0, fg_weight=13, bg_weight=1))),
                F2V=dict(NAME="FrustumToVoxel", SAMPLER=dict(mode="bilinear", padding_mode="zeros")))


def _calibration():
    case = R.CASES["base_LID"]
    return case["lidar_to_cam"].float(), case["cam_to_img"].float(), torch.tensor(case["image_shape"], dtype=torch.int32)


def test_image_vfe_against_float64_restatement(cuda, monkeypatch):
    monkeypatch.setitem(ddn.__all__, "StubDDN", StubDDN)
    torch.manual_seed(0)
    m = vfe.__all__["ImageVFE"](model_cfg=_vfe_cfg(), grid_size=np.array(GRID), point_cloud_range=np.array(RANGE, np.float32), depth_downsample_factor=4,
                                num_point_features=4, voxel_size=None)
    assert m.get_output_feature_dim() == 6
    g = torch.Generator().manual_seed(1)
    images = torch.rand((2, 3, 36, 52), generator=g)
    gout = torch.randn((2, 6, 3, 10, 11), generator=g)
    l2c, c2i, ishape = _calibration()
    # float64 on the CPU: the same modules in double, then the restatement's statements
    ref = copy.deepcopy(m.ffn).double().train()
    res = ref.ddn(images.double())
    feats64 = ref.channel_reduce(res["features"])
    grid64 = R.frustum_grid(l2c, c2i, ishape, GRID, RANGE, DISC, torch.float64)
    want = R.sample(R.create_frustum_features(feats64, res["logits"]), grid64)
    (want * gout.double()).sum().backward()

    m = m.to(cuda).train()
    batch = dict(images=images.to(cuda), trans_lidar_to_cam=l2c.to(cuda), trans_cam_to_img=c2i.to(cuda), image_shape=ishape.to(cuda),
                 depth_maps=torch.zeros((2, 9, 13), device=cuda), gt_boxes2d=torch.zeros((2, 1, 4), device=cuda))
    out = m(batch)
    assert "frustum_features" not in out and out["depth_probs"].shape == (2, 8, 9, 13)
    got = out["voxel_features"]
    assert got.shape == (2, 6, 3, 10, 11)
    assert_close_per_channel(got.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-3, atol_frac=1e-4, name="voxel_features", channel_axis=1)
    (got * gout.to(cuda)).sum().backward()
    ref_params = dict(ref.named_parameters())
    for name, p in m.ffn.named_parameters():
        assert p.grad is not None, name
        a, b = p.grad.cpu().numpy(), ref_params[name].grad.numpy()
        assert_close_per_channel(a.reshape(1, -1), b.reshape(1, -1), rtol=1e-3, atol_frac=1e-4, name=name, channel_axis=0)


def test_conv2d_collapse_on_the_view_and_on_a_copy(cuda):
    torch.manual_seed(2)
    m = map_to_bev.__all__["Conv2DCollapse"](model_cfg=dict(NAME="Conv2DCollapse", NUM_BEV_FEATURES=6, ARGS=dict(kernel_size=1, stride=1, bias=False)),
                                             grid_size=np.array(GRID)).to(cuda).eval()
    assert m.num_bev_features == 6 and m.block.conv.in_channels == 18
    store = torch.randn((2, 10, 11, 6, 3), device=cuda)                    # (B, Y, X, C, Z), the fused kernel's storage order
    view = store.permute(0, 3, 4, 1, 2)                                    # (B, C, Z, Y, X)
    flat = view.flatten(1, 2)
    assert flat.data_ptr() == store.data_ptr() and flat.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        a = m({"voxel_features": view})["spatial_features"]
        b = m({"voxel_features": view.contiguous()})["spatial_features"]
        want = torch.relu(m.block.bn(torch.einsum("oc,bcyx->boyx", m.block.conv.weight[:, :, 0, 0].double(), view.reshape(2, 18, 10, 11).double()).float()))
    assert a.shape == (2, 6, 10, 11)
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a, want, rtol=1e-4, atol=1e-5)


def _detector(cuda):
    torch.manual_seed(3)
    ds = M.SyntheticDatasetInfo(point_cloud_range=[2, -6.4, -3, 14.8, 6.4, 1], voxel_size=(0.4, 0.4, 0.4))
    ds.depth_downsample_factor = 4
    assert ds.grid_size.tolist() == [32, 32, 10]
    cfg = M.caddn_model_cfg(backbone_name="ResNet50", pretrained_path=None, feat_channels=16, num_bins=12, depth_min=2.0, depth_max=14.8, layer_nums=(1, 1, 1))
    return detectors.build_detector(cfg, 3, ds).to(cuda), cfg


def _batch(cuda):
    g = torch.Generator().manual_seed(4)
    B, H, W = 2, 48, 160
    l2c = torch.stack([R._l2c(t=(0., -0.08, -0.27))] * B).float()
    c2i = torch.stack([R._c2i(fx=90.0, fy=90.0, cx=80.0, cy=24.0, t=(5.0, 0.1, 0.003))] * B).float()
    gt = torch.tensor([[[6.0, 1.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1.0], [10.0, -3.0, -0.8, 0.8, 0.6, 1.73, 1.2, 2.0]],
                       [[8.0, -1.5, -1.0, 1.76, 0.6, 1.73, -0.4, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]])
    boxes2d = torch.tensor([[[60.0, 10.0, 110.0, 40.0], [100.0, 12.0, 130.0, 36.0]], [[70.0, 8.0, 95.0, 44.0], [0.0, 0.0, 0.0, 0.0]]])
    return dict(batch_size=B, images=torch.rand((B, 3, H, W), generator=g).to(cuda), trans_lidar_to_cam=l2c.to(cuda), trans_cam_to_img=c2i.to(cuda),
                image_shape=torch.tensor([[H, W]] * B, dtype=torch.int32, device=cuda), gt_boxes=gt.to(cuda), gt_boxes2d=boxes2d.to(cuda),
                depth_maps=(torch.rand((B, H // 4, W // 4), generator=g) * 16).to(cuda))


def test_caddn_detector_train_step_and_eval(cuda):
    model, cfg = _detector(cuda)
    model.train()
    batch = _batch(cuda)
    ret, tb, disp = model(dict(batch))
    loss = ret["loss"]
    assert torch.isfinite(loss)
    assert {"loss_rpn", "loss_depth", "rpn_loss_cls", "rpn_loss_loc", "rpn_loss_dir", "rpn_loss", "balancer_loss", "fg_loss", "bg_loss", "ddn_loss"} <= set(tb)
    assert all(isinstance(tb[k], float) for k in ("loss_rpn", "loss_depth", "ddn_loss"))
    loss.backward()
    missing = [n for n, p in model.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    # the depth loss on the same logits, restated in float64 on the CPU
    ffn = model.vfe.ffn
    args = cfg["VFE"]["FFN"]["LOSS"]["ARGS"]
    want, _, _ = R.ddn_loss(ffn.forward_ret_dict["depth_logits"].detach().double().cpu(), batch["depth_maps"].double().cpu(), batch["gt_boxes2d"].double().cpu(),
                            cfg["VFE"]["FFN"]["DISCRETIZE"], downsample_factor=4, **args)
    assert abs(tb["loss_depth"] - float(want)) <= 1e-4 * abs(float(want))
    assert abs(tb["loss_rpn"] + tb["loss_depth"] - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))

    model.eval()
    with torch.no_grad():
        pred_dicts, recall = model(dict(batch))
    assert len(pred_dicts) == 2
    for p in pred_dicts:
        assert {"pred_boxes", "pred_scores", "pred_labels"} <= set(p)
        assert p["pred_boxes"].shape[-1] == 7 and p["pred_boxes"].shape[0] == p["pred_scores"].shape[0] == p["pred_labels"].shape[0]
