"""Voxel R-CNN on VoxelBackBone8xFocal with the image branch (model_cfgs.voxelrcnn_focal_model_cfg(use_img=True, img_pretrain=None): the MODEL
section of kitti_models/voxel_rcnn_car_focal_multimodal.yaml as the yaml sets it, the image network at random initialisation): one train step and
one eval pass on a synthetic scene batch with a random image and a synthetic calibration."""
import numpy as np
import pytest
import torch

import focal_image_reference as FI
import seevcn_amd.pcdet.model_cfgs as C
from seeding import seeded_state_dict

IMAGE = (96, 320)


def _net_and_batch(cuda):
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.models import detectors
    # 8 RoIs per scene: at seeded weights the RoIs pile up on one spot, and the order-fixed voxel-pool gradient sorts one key list per voxel -- its
    # longest list, and with it the time of this test (tens of seconds at 32 RoIs), grows with the RoIs that share a voxel
    cfg = C.voxelrcnn_focal_model_cfg(dynamic_vfe=True, roi_per_image=8, nms_post_train=128, nms_pre_train=2048, use_img=True, img_pretrain=None)
    net = detectors.build_detector(cfg, num_class=1, dataset=C.SyntheticDatasetInfo(class_names=C.VOXELRCNN_CLASS_NAMES))
    net.load_state_dict(seeded_state_dict(net, seed=6))
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=100)
    gt = gt.copy()
    gt[:, :, 7] = np.where(gt[:, :, 3] > 0, 1, 0)                                            # one class
    images = torch.from_numpy(np.random.RandomState(12).rand(2, 3, *IMAGE).astype(np.float32)).to(cuda)
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda), "images": images,
             "calib": [FI.make_calib(IMAGE, b) for b in range(2)], "noise_rot": torch.tensor([0.1, -0.2], device=cuda),
             "flip_x": torch.tensor([True, False], device=cuda)}
    return net.to(cuda), batch


def _train_step(net, batch):
    net.zero_grad(set_to_none=True)
    np.random.seed(0)
    torch.manual_seed(0)
    ret, tb, _ = net(dict(batch))
    ret["loss"].backward()
    return ret, tb, {n: p.grad.cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.gpu
def test_hip_voxelrcnn_focal_multimodal_train_step_and_eval(cuda, hip_lib):
    import seevcn_amd
    net, batch = _net_and_batch(cuda)
    net.train()
    bb = net.backbone_3d
    focal_layers = {"conv1": bb.conv1[1], "conv2": bb.conv2[3], "conv3": bb.conv3[3], "image": bb.conv_focal_multimodal}
    terms = {}
    hooks = [layer.register_forward_hook(lambda mod, args, out, key=key: terms.__setitem__(key, float(out[2]))) for key, layer in focal_layers.items()]
    # the order-fixed route covers this library's scatter gradients; torch's dense convolutions sum their weight gradients in a fixed order only
    # when asked to
    before = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        with seevcn_amd.set_ordered_gradients(True):
            ret, tb, grads = _train_step(net, batch)
            for h in hooks:
                h.remove()
            _, _, grads2 = _train_step(net, batch)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before
    assert torch.isfinite(ret["loss"]) and {"rpn_loss", "rcnn_loss", "loss_box_of_pts"} <= set(tb)
    assert all(np.isfinite(v) for v in tb.values() if isinstance(v, float)), tb
    # loss_box_of_pts holds the image layer's term beside the three stages'
    assert set(terms) == set(focal_layers) and terms["image"] > 0, terms
    assert abs(tb["loss_box_of_pts"] - sum(terms.values())) <= 1e-5 * sum(terms.values()), (tb["loss_box_of_pts"], terms)
    image_side = [n for n in grads if n.startswith("backbone_3d.semseg.reduce_blocks.0.") or n.startswith("backbone_3d.semseg.ifn.model.backbone.layer1.")]
    assert any("reduce_blocks.0.conv.weight" in n for n in image_side) and any("layer1.2.conv3.weight" in n for n in image_side)
    for n in image_side + [k for k in grads if k.startswith("backbone_3d.conv_focal_multimodal.")]:
        assert np.isfinite(grads[n]).all() and np.abs(grads[n]).sum() > 0, n
    assert not any(n.startswith("backbone_3d.semseg.ifn.model.backbone.layer2") for n in grads)               # the ResNet stops behind layer1
    differ = [n for n in image_side if grads[n].tobytes() != grads2[n].tobytes()]
    print(len(image_side), "image-side parameters with a gradient,", len(differ), "differ between the two steps; terms", terms)
    assert differ == [], differ[:10]
    net.eval()
    with torch.no_grad():
        preds, recall = net(dict(batch))
    assert len(preds) == 2 and "gt" in recall
    for p in preds:
        n = p["pred_boxes"].shape[0]
        assert p["pred_boxes"].shape == (n, 7) and p["pred_scores"].shape == (n,) and p["pred_labels"].shape == (n,)
        assert torch.isfinite(p["pred_boxes"]).all() and bool((p["pred_labels"] == 1).all())
