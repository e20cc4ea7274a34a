"""The roiaware_pool3d helpers the hot path uses, with the reference's names and signatures (detector3d/pcdet/ops/roiaware_pool3d/
roiaware_pool3d_utils.py:9-41), over the pybind-level module roiaware_pool3d_cuda.  `points_in_boxes_cpu` keeps its name and
numpy / torch-CPU interface; the box test itself runs on the GPU (there is no CPU path in this build).  RoIAwarePool3d
(:44-107) runs on sv_roiaware_assign / sv_roiaware_pool directly."""
import numpy as np
import torch

from .... import _lib, ordered
from . import roiaware_pool3d_cuda


def points_in_boxes_cpu(points, boxes):
    """points (num_points,3), boxes (N,7) -> point_indices (N,num_points) int32 0/1 (box test with margin 1e-2, :9-25)."""
    assert boxes.shape[1] == 7
    assert points.shape[1] == 3
    is_numpy = isinstance(points, np.ndarray)
    p = (torch.from_numpy(points) if is_numpy else points).float().contiguous()
    b = (torch.from_numpy(boxes) if isinstance(boxes, np.ndarray) else boxes).float().contiguous()
    point_indices = p.new_zeros((b.shape[0], p.shape[0]), dtype=torch.int)
    roiaware_pool3d_cuda.points_in_boxes_cpu(b, p, point_indices)
    return point_indices.numpy() if is_numpy else point_indices


def points_in_boxes_gpu(points, boxes):
    """points (B,M,3), boxes (B,T,7) -> (B,M) int32 box index of each point, background = -1 (:28-41)"""
    assert boxes.shape[0] == points.shape[0]
    assert boxes.shape[2] == 7 and points.shape[2] == 3
    _lib.require_cuda(points, boxes)
    batch_size, num_points, _ = points.shape
    box_idxs_of_pts = torch.full((batch_size, num_points), -1, dtype=torch.int32, device=points.device)
    roiaware_pool3d_cuda.points_in_boxes_gpu(boxes.contiguous().float(), points.contiguous().float(), box_idxs_of_pts)
    return box_idxs_of_pts


POOL_METHODS = {"max": 0, "avg": 1}


def _out_xyz(out_size):
    if isinstance(out_size, int):
        return out_size, out_size, out_size
    assert len(out_size) == 3
    for k in range(3):
        assert isinstance(out_size[k], int)
    return tuple(out_size)


def assign_points_to_cells(rois, pts, out_size, max_pts_each_voxel, box_pt_range=None):
    """pts_idx_of_voxels (N, out_x, out_y, out_z, max_pts_each_voxel) int32 of sv_roiaware_assign: slot 0 of a cell its count, then the rows of
    pts inside the box that fall into the cell, ascending.  box_pt_range (N, 2) int32: box b looks at rows [lo, hi) only.  The tensor is not
    zero-filled: slots behind a count hold whatever the allocation held."""
    assert rois.shape[1] == 7 and pts.shape[1] == 3
    out_x, out_y, out_z = _out_xyz(out_size)
    rois, pts = rois.contiguous().float(), pts.contiguous().float()
    if box_pt_range is not None:
        assert box_pt_range.dtype == torch.int32 and tuple(box_pt_range.shape) == (rois.shape[0], 2)
        box_pt_range = box_pt_range.contiguous()
    lists = torch.empty((rois.shape[0], out_x, out_y, out_z, max_pts_each_voxel), dtype=torch.int32, device=rois.device)
    _lib.launch("sv_roiaware_assign", _lib.ptr(rois) if rois.numel() else None, rois.shape[0], _lib.ptr(pts) if pts.numel() else None, pts.shape[0],
                _lib.ptr(box_pt_range) if box_pt_range is not None and box_pt_range.numel() else None, out_x, out_y, out_z, max_pts_each_voxel,
                _lib.ptr(lists) if lists.numel() else None)
    return lists


class RoIAwarePoolFromListsFunction(torch.autograd.Function):
    """Pooling of one feature set over lists that assign_points_to_cells left; saves the lists and argmax.  Only pts_feature gets a gradient."""

    @staticmethod
    def forward(ctx, pts_feature, pts_idx_of_voxels, pool_method):
        assert pts_feature.dim() == 2 and pts_idx_of_voxels.dtype == torch.int32 and pts_idx_of_voxels.dim() == 5
        method = POOL_METHODS[pool_method]
        feat = pts_feature.contiguous().float()
        lists = pts_idx_of_voxels.contiguous()
        n, ox, oy, oz, cap = lists.shape
        c = feat.shape[1]
        pooled = torch.empty((n, ox, oy, oz, c), dtype=torch.float32, device=feat.device)
        argmax = torch.empty((n, ox, oy, oz, c), dtype=torch.int32, device=feat.device) if method == 0 else None
        _lib.launch("sv_roiaware_pool", _lib.ptr(feat) if feat.numel() else None, c, _lib.ptr(lists) if lists.numel() else None, n, ox * oy * oz, cap, method,
                    _lib.ptr(pooled) if pooled.numel() else None, _lib.ptr(argmax) if argmax is not None and argmax.numel() else None)
        ctx.roiaware_pool3d_for_backward = (lists, argmax, method, feat.shape[0], c)
        return pooled

    @staticmethod
    def backward(ctx, grad_out):
        lists, argmax, method, num_pts, c = ctx.roiaware_pool3d_for_backward
        n, ox, oy, oz, cap = lists.shape
        cells = ox * oy * oz
        grad_out = grad_out.contiguous().float()
        grad_in = torch.empty((num_pts, c), dtype=torch.float32, device=grad_out.device)
        lib = _lib.load()
        args = (_lib.ptr(lists) if lists.numel() else None, _lib.ptr(argmax) if argmax is not None and argmax.numel() else None,
                _lib.ptr(grad_out) if grad_out.numel() else None, n, cells, c, cap, method, num_pts)
        gi = _lib.ptr(grad_in) if grad_in.numel() else None
        if ordered.ordered_gradients():                               # read when the backward runs
            nbytes = lib.sv_roiaware_pool_backward_ordered_scratch_bytes(n, cells, c, cap, method, num_pts)
            if nbytes == 0:
                raise _lib.SeevcnHipError("roiaware pooling: the order-fixed gradient needs fewer than 2^31 keys")
            scratch = _lib.workspace.scratch("roiaware_pool_ordered", nbytes, grad_out.device)
            _lib.launch("sv_roiaware_pool_backward_ordered", *args, _lib.ptr(scratch), gi)
            ordered.count_call("roiaware_pool")
        else:
            _lib.launch("sv_roiaware_pool_backward", *args, gi)
        return grad_in, None, None


class RoIAwarePool3dFunction(torch.autograd.Function):
    """The reference's Function (roiaware_pool3d_utils.py:55-107), same arguments: assignment and pooling of one feature set."""

    @staticmethod
    def forward(ctx, rois, pts, pts_feature, out_size, max_pts_each_voxel, pool_method):
        assert rois.shape[1] == 7 and pts.shape[1] == 3
        assert pts_feature.shape[0] == pts.shape[0]
        lists = assign_points_to_cells(rois, pts, out_size, max_pts_each_voxel)
        return RoIAwarePoolFromListsFunction.forward(ctx, pts_feature, lists, pool_method)

    @staticmethod
    def backward(ctx, grad_out):
        grad_in = RoIAwarePoolFromListsFunction.backward(ctx, grad_out)[0]
        return None, None, grad_in, None, None, None


class RoIAwarePool3d(torch.nn.Module):
    """roiaware_pool3d_utils.py:44-53 over sv_roiaware_assign / sv_roiaware_pool (the pybind-level pair roiaware_pool3d_cuda.forward / backward
    is not built and still raises: this module calls the library's entries itself)."""

    def __init__(self, out_size, max_pts_each_voxel=128):
        super().__init__()
        self.out_size = out_size
        self.max_pts_each_voxel = max_pts_each_voxel

    def forward(self, rois, pts, pts_feature, pool_method='max'):
        assert pool_method in ['max', 'avg']
        return RoIAwarePool3dFunction.apply(rois, pts, pts_feature, self.out_size, self.max_pts_each_voxel, pool_method)

    def forward_multi(self, rois, pts, pts_features, pool_methods, box_pt_range=None):
        """Beyond the reference: ONE assignment, then one pooling per feature set.  pts_features: tensors (npoints, C_i); pool_methods: 'max' /
        'avg' for each.  box_pt_range (N, 2) int32, rows [lo, hi) of pts that box b looks at: with the rows of a batch stacked scene after
        scene, the boxes of every scene are served by one launch.  Returns the (N, out_x, out_y, out_z, C_i) results."""
        assert len(pts_features) == len(pool_methods)
        for f, m in zip(pts_features, pool_methods):
            assert m in ['max', 'avg']
            assert f.shape[0] == pts.shape[0]
        lists = assign_points_to_cells(rois, pts, self.out_size, self.max_pts_each_voxel, box_pt_range)
        return [RoIAwarePoolFromListsFunction.apply(f, lists, m) for f, m in zip(pts_features, pool_methods)]
