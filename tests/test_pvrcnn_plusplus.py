"""PV-RCNN++: the configuration restatement against the yaml's values (tests/golden/pv_rcnn_plusplus_model.json, the MODEL section of
waymo_models/pv_rcnn_plusplus.yaml as data) and the detector built from the registries at reduced sizes."""
import json
import os

import numpy as np
import pytest
import torch

from seeding import seeded_state_dict
from seevcn_amd.pcdet import model_cfgs as C

SMALL = dict(num_keypoints=256, roi_per_image=32, nms_post_train=64, nms_pre_train=512)


def _same(mine, theirs, path=""):
    """every key of the yaml with the yaml's value, and nothing besides"""
    if isinstance(theirs, dict):
        assert isinstance(mine, dict) and sorted(mine) == sorted(theirs), (path, sorted(mine) if isinstance(mine, dict) else mine, sorted(theirs))
        for k in theirs:
            _same(mine[k], theirs[k], f"{path}.{k}")
    elif isinstance(theirs, (list, tuple)):
        assert isinstance(mine, (list, tuple)) and len(mine) == len(theirs), (path, mine, theirs)
        for i, (a, b) in enumerate(zip(mine, theirs)):
            _same(a, b, f"{path}[{i}]")
    else:
        assert mine == theirs and isinstance(mine, bool) == isinstance(theirs, bool), (path, mine, theirs)


def test_config_restates_the_yaml_key_by_key(golden_dir):
    yaml_model = json.load(open(os.path.join(golden_dir, "pv_rcnn_plusplus_model.json")))
    _same(C.pvrcnnpp_model_cfg(), yaml_model, "MODEL")
    assert C.pvrcnnpp_model_cfg()["ROI_HEAD"]["ROI_GRID_POOL"] == C.PVRCNNPP_ROI_GRID_POOL
    small = C.pvrcnnpp_model_cfg(dynamic_vfe=True, **SMALL)
    assert small["VFE"]["NAME"] == "DynMeanVFE" and small["PFE"]["NUM_KEYPOINTS"] == 256 and small["PFE"]["SAMPLE_METHOD"] == "SPC"
    assert small["ROI_HEAD"]["TARGET_CONFIG"]["ROI_PER_IMAGE"] == 32 and small["ROI_HEAD"]["NMS_CONFIG"]["TRAIN"]["NMS_POST_MAXSIZE"] == 64
    assert C.pvrcnnpp_model_cfg()["PFE"]["SA_LAYER"] is not C.PVRCNNPP_SA_LAYER          # a copy: a test that shrinks it leaves the restatement alone


def test_detector_is_registered():
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.pcdet.models.detectors.pv_rcnn_plusplus import PVRCNNPlusPlus
    assert detectors.__all__["PVRCNNPlusPlus"] is PVRCNNPlusPlus and PVRCNNPlusPlus.LOSS_HEADS == ("dense_head", "point_head", "roi_head")


def _net_and_batch(cuda):
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.models import detectors
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=100)
    pts = np.concatenate([pts, np.random.default_rng(4).uniform(size=(len(pts), 1)).astype(np.float32)], 1)      # intensity
    gt = gt.copy()
    gt[:, :, 7] = np.where(gt[:, :, 3] > 0, 1, 0)                                            # every box a 'Vehicle'
    cfg = C.pvrcnnpp_model_cfg(dynamic_vfe=True, **SMALL)
    # four point features [x, y, z, intensity]: the dynamic voxeliser sums up to four in fixed point, so the step is reproducible to the bit; the
    # one feature channel of the raw points is its own reduced channel
    cfg["PFE"]["SA_LAYER"]["raw_points"]["NUM_REDUCED_CHANNELS"] = 1
    ds = C.SyntheticDatasetInfo(class_names=C.WAYMO_CLASS_NAMES, point_cloud_range=C.DA_RANGE, voxel_size=C.DA_VOXEL, num_point_features=4)
    net = detectors.build_detector(cfg, num_class=3, dataset=ds)
    assert type(net).__name__ == "PVRCNNPlusPlus"
    net.load_state_dict(seeded_state_dict(net, seed=6))
    counts = [int((pts[:, 0] == b).sum()) for b in range(2)]
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda), "points_per_scene": counts}
    return net.to(cuda), batch


def _train_step(net, batch):
    net.zero_grad(set_to_none=True)
    np.random.seed(0)
    torch.manual_seed(0)
    ret, tb, _ = net(dict(batch))
    ret["loss"].backward()
    return ret["loss"].detach().cpu().numpy().copy(), tb, {n: p.grad.cpu().numpy().copy() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.gpu
def test_hip_pvrcnn_plusplus_train_step_and_eval(cuda, hip_lib):
    import seevcn_amd
    net, batch = _net_and_batch(cuda)
    net.train()
    # the order-fixed route covers this library's scatter gradients; the dense convolutions of BaseBEVBackbone / CenterHead / the vector-pool MLPs are
    # torch's, whose weight gradients are summed in a fixed order only when asked to be
    before = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        with seevcn_amd.set_ordered_gradients(True):
            loss, tb, grads = _train_step(net, batch)
            loss2, _, grads2 = _train_step(net, batch)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before
    assert np.isfinite(loss) and {"rpn_loss", "point_loss_cls", "rcnn_loss"} <= set(tb), (loss, sorted(tb))
    # every parameter the reference's graph reaches: all of them but PointHeadSimple's box-less leftovers, which it does not have
    missing = [n for n, p in net.named_parameters() if p.requires_grad and n not in grads]
    assert missing == [], missing
    bad = [n for n, g in grads.items() if not np.isfinite(g).all()]
    assert bad == [], bad
    # two identical steps on the order-fixed route: the same bits
    assert loss.tobytes() == loss2.tobytes(), (loss, loss2)
    differ = [n for n in grads if grads[n].tobytes() != grads2[n].tobytes()]
    print(len(grads), "parameters with a gradient,", len(differ), "differ between the two steps")
    assert differ == [], (len(differ), differ[:10])
    net.eval()
    with torch.no_grad():
        preds, recall = net(dict(batch))
    assert len(preds) == 2 and "gt" in recall
    for p in preds:
        n = p["pred_boxes"].shape[0]
        assert p["pred_boxes"].shape == (n, 7) and p["pred_scores"].shape == (n,) and p["pred_labels"].shape == (n,)
        assert torch.isfinite(p["pred_boxes"]).all() and bool(((p["pred_labels"] >= 1) & (p["pred_labels"] <= 3)).all())
