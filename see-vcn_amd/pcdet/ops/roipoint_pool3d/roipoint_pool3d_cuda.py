"""`roipoint_pool3d_cuda` with the reference's entry name and argument order (detector3d/pcdet/ops/roipoint_pool3d/src/roipoint_pool3d.cpp:
forward(xyz, boxes3d, pts_feature, pooled_features, pooled_empty_flag)) over sv_roipoint_pool3d: ONE launch, caller-allocated outputs, return
value 1.  Every element of both outputs is written, so they may come from torch.empty.  `canonical` (keyword only, seevcn extension): the xyz
columns of pooled_features hold the point in its box's frame."""
import torch

from .... import _lib


def forward(xyz, boxes3d, pts_feature, pooled_features, pooled_empty_flag, *, canonical=False):
    """xyz (B, N, 3), boxes3d (B, M, 7), pts_feature (B, N, C), pooled_features (B, M, S, 3 + C), pooled_empty_flag (B, M) int32"""
    assert xyz.dtype == boxes3d.dtype == pts_feature.dtype == pooled_features.dtype == torch.float32 and pooled_empty_flag.dtype == torch.int32
    batch, n_pts, n_boxes, c = xyz.shape[0], xyz.shape[1], boxes3d.shape[1], pts_feature.shape[2]
    n_sampled = pooled_features.shape[2]
    assert tuple(xyz.shape) == (batch, n_pts, 3) and tuple(boxes3d.shape) == (batch, n_boxes, 7) and tuple(pts_feature.shape) == (batch, n_pts, c)
    assert tuple(pooled_features.shape) == (batch, n_boxes, n_sampled, 3 + c) and tuple(pooled_empty_flag.shape) == (batch, n_boxes)
    p = lambda t: _lib.ptr(t) if t.numel() else None
    _lib.launch("sv_roipoint_pool3d", p(xyz), p(pts_feature), p(boxes3d), batch, n_pts, n_boxes, c, n_sampled, int(bool(canonical)), p(pooled_features),
                p(pooled_empty_flag))
    return 1
