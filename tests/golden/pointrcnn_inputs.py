"""Deterministic inputs shared by make_pointrcnn_golden.py (reference side) and tests/test_pointrcnn.py (this repo's modules)."""
import numpy as np

POINT_CHANNELS = 128                    # PointRCNNHead merges its 128 lifted xyz channels with as many backbone channels
POINTS_PER_SCENE = 256
SMALL = dict(npoints=(128, 32, 8, 4), num_sampled_points=32, roi_npoints=(8, 4, -1), roi_per_image=16, nms_pre_train=512, nms_post_train=64,
             nms_pre_test=512, nms_post_test=16)
CLEAR = 1e-3
GT_EXTRA_WIDTH = 0.2


def _local(boxes, pts):
    """float64 box-frame coordinates (M, N, 3) of pts (N, 3) for boxes (M, 7)."""
    b, p = np.asarray(boxes, np.float64), np.asarray(pts, np.float64)
    s = p[None, :, :] - b[:, None, :3]
    c, sn = np.cos(-b[:, 6])[:, None], np.sin(-b[:, 6])[:, None]
    return np.stack([s[..., 0] * c - s[..., 1] * sn, s[..., 0] * sn + s[..., 1] * c, s[..., 2]], -1)


def clear_of(boxes, pts, clear=CLEAR):
    """(N,) bool: every point at least `clear` away from the surface of every box, per axis, in float64."""
    b = np.asarray(boxes, np.float64)
    d = np.abs(_local(boxes, pts)) - b[:, None, 3:6] / 2
    return ((d < -clear).all(-1) | (d > clear).any(-1)).all(0)


def make_gt():
    """gt_boxes (2, 4, 8) fp32 [x, y, z, dx, dy, dz, heading, class]: one of each class in scene 0 and a zero row, four boxes in scene 1."""
    rng = np.random.default_rng(41)
    sizes = {1: [3.9, 1.6, 1.56], 2: [0.8, 0.6, 1.73], 3: [1.76, 0.6, 1.73]}
    gt = np.zeros((2, 4, 8), np.float32)
    for b, classes in enumerate(([1, 2, 3], [1, 1, 3, 2])):
        for k, c in enumerate(classes):
            gt[b, k] = [10.0 + 12.0 * k + rng.uniform(-1, 1), rng.uniform(-15, 15), rng.uniform(-1.2, -0.6),
                        *(np.array(sizes[c]) * rng.uniform(0.85, 1.15, 3)), rng.uniform(-3.1, 3.1), c]
    return gt


def make_head_inputs():
    """point_coords (2 * 256, 4) stacked scene after scene: 60 % of the points in and around the ground-truth boxes (inside, in the 0.2 m shell
    of the enlarged box, just outside it), the rest anywhere; every point CLEAR away from the surfaces of the boxes and of the enlarged boxes.
    point_features (512, POINT_CHANNELS) seeded."""
    rng = np.random.default_rng(43)
    gt = make_gt()
    coords = np.zeros((2, POINTS_PER_SCENE, 4), np.float32)
    for b in range(2):
        boxes = gt[b][gt[b, :, 3] > 0][:, :7]
        large = boxes.copy()
        large[:, 3:6] = large[:, 3:6] + np.float32(GT_EXTRA_WIDTH)
        for i in range(POINTS_PER_SCENE):
            for _ in range(1000):
                if rng.uniform() < 0.6:
                    bx = boxes[rng.integers(len(boxes))].astype(np.float64)
                    loc = rng.uniform(-0.7, 0.7, 3) * bx[3:6]
                    c, s = np.cos(bx[6]), np.sin(bx[6])
                    p = np.array([bx[0] + loc[0] * c - loc[1] * s, bx[1] + loc[0] * s + loc[1] * c, bx[2] + loc[2]])
                else:
                    p = rng.uniform([0, -30, -2.5], [60, 30, 0.5])
                p = p.astype(np.float32)[None]
                if clear_of(boxes, p).all() and clear_of(large, p).all():
                    coords[b, i] = [b, *p[0]]
                    break
            else:
                raise AssertionError("no clear point found")
    return {'gt_boxes': gt, 'point_coords': coords.reshape(-1, 4),
            'point_features': rng.normal(size=(2 * POINTS_PER_SCENE, POINT_CHANNELS)).astype(np.float32)}


def make_coder_inputs():
    """boxes (40, 7), points (40, 3), classes (40) in 1..3, encodings (40, 8) for PointResidualCoder."""
    rng = np.random.default_rng(47)
    boxes = np.concatenate([rng.uniform(-20, 20, (40, 3)), rng.uniform(0.4, 5.0, (40, 3)), rng.uniform(-3.1, 3.1, (40, 1))], 1).astype(np.float32)
    boxes[0, 3:6] = 0.0                                                     # a degenerate box: its sizes are clamped to 1e-5 inside encode
    points = (boxes[:, :3] + rng.normal(0, 1, (40, 3))).astype(np.float32)
    classes = rng.integers(1, 4, 40).astype(np.int64)
    enc = (rng.normal(0, 0.5, (40, 8))).astype(np.float32)
    return boxes, points, classes, enc


MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]


def make_rois(points):
    """rois (2, 8, 7) for the head tests: the ground-truth boxes grown and turned a little, and far-away boxes that hold no point; every point of
    `points` (2 * 256, 4) is CLEAR away from every RoI's surface (a candidate that is not is drawn again)."""
    rng = np.random.default_rng(53)
    gt = make_gt()
    rois = np.zeros((2, 8, 7), np.float32)
    for b in range(2):
        pts = points[points[:, 0] == b][:, 1:4]
        boxes = gt[b][gt[b, :, 3] > 0][:, :7]
        for k in range(8):
            for _ in range(1000):
                if k < 6:
                    r = boxes[k % len(boxes)].copy()
                    r[0:3] += rng.normal(0, 0.15, 3)
                    r[3:6] *= rng.uniform(1.0, 1.4, 3)
                    r[6] += rng.normal(0, 0.2)
                else:
                    r = np.array([65.0 + 3 * k, -35.0, 5.0, 2.0, 2.0, 2.0, rng.uniform(-3, 3)])
                r = r.astype(np.float32)
                if clear_of(r[None], pts).all():
                    rois[b, k] = r
                    break
            else:
                raise AssertionError("no clear RoI found")
    return rois
