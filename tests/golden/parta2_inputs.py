"""Deterministic inputs shared by make_parta2_golden.py (reference side) and tests/test_parta2.py (this repo's modules)."""
import numpy as np

SMALL = dict(pool_size=6, roi_per_image=16, nms_post_train=64, nms_pre_train=512, dp_ratio=0.0, shared_fc=(64, 64), num_features=32)
POINT_CHANNELS = 16
VOXEL = np.array([0.2, 0.2, 0.2])


def make_inputs():
    """Two scenes: the centres of the occupied 0.2 m voxels as points, stacked scene after scene (what UNetV2 hands the heads), seeded point
    features, ground truth, and first-stage proposals (jittered ground truth + random boxes), 32 RoIs in all after sampling."""
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet import model_cfgs as C
    rng = np.random.default_rng(29)
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=60)
    gt = gt[:, :10].copy()
    rg = np.array(C.KITTI_RANGE[:3])
    cells = np.unique(np.concatenate([pts[:, 0:1], np.floor((pts[:, 1:4] - rg) / VOXEL)], 1).astype(np.int64), axis=0)
    keep = np.zeros(len(cells), bool)
    for b in range(2):                                                     # every point near a box, and a sample of the rest
        g = gt[b][gt[b, :, 3] > 0]
        c = (cells[:, 1:4] + 0.5) * VOXEL + rg
        near = (np.abs(c[:, None, :2] - g[None, :, :2]).max(-1) < 4.0).any(1)
        keep |= (cells[:, 0] == b) & (near | (rng.uniform(size=len(cells)) < 0.1))
    cells = cells[keep]
    order = np.concatenate([rng.permutation(np.flatnonzero(cells[:, 0] == b)) for b in range(2)])
    cells = cells[order]
    coords = np.concatenate([cells[:, 0:1].astype(np.float32), ((cells[:, 1:4] + 0.5) * VOXEL + rg).astype(np.float32)], 1)
    out = {'gt_boxes': gt.astype(np.float32), 'point_coords': coords, 'point_features': rng.normal(size=(len(coords), POINT_CHANNELS)).astype(np.float32)}
    boxes, scores = [], []
    for b in range(2):
        g = gt[b][gt[b, :, 3] > 0][:, :7]
        rep = np.repeat(g, 12, axis=0) + rng.normal(0, 1, (len(g) * 12, 7)).astype(np.float32) * np.array([0.25, 0.25, 0.1, 0.1, 0.05, 0.05, 0.1], np.float32)
        rnd = np.concatenate([rng.uniform([0, -40, -2], [70, 40, 0], (100, 3)), rng.uniform([1.5, 0.6, 1.2], [4.5, 2, 2], (100, 3)),
                              rng.uniform(-3, 3, (100, 1))], 1).astype(np.float32)
        bx = np.concatenate([rep, rnd])[:200]
        boxes.append(np.concatenate([bx, np.zeros((200 - len(bx), 7), np.float32)]))
        scores.append(rng.normal(size=(200, 1)).astype(np.float32))
    out['batch_box_preds'] = np.stack(boxes).astype(np.float32)
    out['batch_cls_preds'] = np.stack(scores).astype(np.float32)
    return out
