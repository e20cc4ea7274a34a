"""Focal sparse convolution's expansion of the active set (csrc/focal_conv.hip): host wrappers over the sv_focal_* entries and the autograd
Function the FocalSparseConv module calls.  Replaces split_voxels / check_repeat / combine_out of the reference
(detector3d/pcdet/models/backbones_3d/focal_sparse_conv/focal_sparse_utils.py:39-147, focal_sparse_conv.py:171-197).  Below them the image branch
(csrc/focal_image.hip): the pixels of the projected voxels and the fused [image | voxel] rows of construct_multimodal_features (focal_sparse_conv.py:50-113)."""
import ctypes

import torch

from .. import _lib
from .core import SparseConvTensor

N_IMPORTANCE = 27          # columns of the importance map: 26 kernel offsets (centre removed) + the voxel importance


def _shape3(shape):
    return _lib.host_array(ctypes.c_int32, [int(v) for v in shape])


def _check_inputs(indices, s):
    assert indices.dtype == torch.int32 and indices.dim() == 2 and indices.shape[1] == 4, "indices: (n, 4) int32 [b, z, y, x]"
    assert s.dtype == torch.float32 and s.shape == (indices.shape[0], N_IMPORTANCE), "s: (n, 27) fp32 = sigmoid(imps)"


def index_workspace(batch_size, spatial_shape, device):
    """The coordinate-index workspace of a (batch, grid): the one the rank-dictionary rulebook builders keep zeroed under the same name."""
    lib = _lib.load()
    ncells = int(batch_size) * int(spatial_shape[0]) * int(spatial_shape[1]) * int(spatial_shape[2])
    return _lib.workspace.persistent(f"rb_index_{tuple(int(v) for v in spatial_shape)}_{int(batch_size)}", lib.sv_index_persistent_bytes(ncells), device), ncells


def focal_select(s, indices, batch_size, topk, threshold):
    """fore (n) uint8: the foreground rows (sv_focal_select).  No host read."""
    lib = _lib.load()
    _check_inputs(indices, s)
    s, indices = s.contiguous(), indices.contiguous()
    n = indices.shape[0]
    fore = torch.empty((n,), dtype=torch.uint8, device=s.device)
    scratch = _lib.workspace.scratch("focal_select", lib.sv_focal_select_scratch_bytes(int(batch_size)), s.device) if topk else None
    _lib.launch("sv_focal_select", _lib.ptr(s), _lib.ptr(indices), n, int(batch_size), int(bool(topk)), float(threshold), _lib.ptr(scratch), _lib.ptr(fore))
    return fore


def focal_cells(indices, s, fore, batch_size, spatial_shape, threshold, capacity=None, out_coords=None):
    """-> (out_coords (num_out, 4) int32 in canonical order, row_of_in (n) int32, num_out): the union of the input cells and the kept candidates
    (sv_focal_expand), with ONE device -> host read (num_out).  capacity: rows the output may take (default: 27 n, at most the number of cells);
    a larger set raises and nothing is written past capacity.  out_coords: a caller's buffer of at least capacity rows."""
    lib = _lib.load()
    _check_inputs(indices, s)
    assert fore.dtype == torch.uint8 and fore.shape == (indices.shape[0],)
    s, indices, fore = s.contiguous(), indices.contiguous(), fore.contiguous()
    n, dev = indices.shape[0], indices.device
    ws, ncells = index_workspace(batch_size, spatial_shape, dev)
    if capacity is None:
        capacity = max(min(N_IMPORTANCE * n, ncells), 1)
    capacity = int(capacity)
    if out_coords is None:
        out_coords = torch.empty((capacity, 4), dtype=torch.int32, device=dev)
    assert out_coords.dtype == torch.int32 and out_coords.dim() == 2 and out_coords.shape[1] == 4 and out_coords.shape[0] >= capacity
    scratch = _lib.workspace.scratch("focal_expand", lib.sv_focal_expand_scratch_bytes(ncells), dev)
    row_of_in = torch.empty((n,), dtype=torch.int32, device=dev)
    num_out = torch.empty((1,), dtype=torch.int32, device=dev)
    _lib.launch("sv_focal_expand", _lib.ptr(indices), _lib.ptr(s), _lib.ptr(fore), n, int(batch_size), _shape3(spatial_shape), float(threshold), _lib.ptr(ws),
                _lib.ptr(scratch), _lib.ptr(out_coords), _lib.ptr(row_of_in), capacity, _lib.ptr(num_out))
    n_out = _lib.host_int(num_out)          # the host allocates the output rows: the one read of a focal layer
    if n_out > capacity:
        raise _lib.SeevcnHipError(f"sv_focal_expand: the expanded set has {n_out} cells, the capacity is {capacity}")
    return out_coords[:n_out], row_of_in, n_out


class FocalExpandFunction(torch.autograd.Function):
    """(features (n, C), s (n, 27) = sigmoid(imps)) -> features of the expanded set (num_out, C); also returns, without gradient, the expanded
    indices, fore and row_of_in.  nbr: the (27, n) k = 3 submanifold table of the input set.  The selection is constant in the backward, which is a
    gather through the same table: no float atomics, bit-identical run to run."""

    @staticmethod
    def forward(ctx, features, s, indices, nbr, batch_size, spatial_shape, topk, threshold, mask_multi, skip_mask_kernel, capacity):
        features, s, indices = features.contiguous().float(), s.contiguous(), indices.contiguous()
        n, C = features.shape
        assert nbr.dtype == torch.int32 and nbr.shape == (N_IMPORTANCE, n) and nbr.is_contiguous(), "nbr: the (27, n) submanifold table of the input set"
        fore = focal_select(s, indices, batch_size, topk, threshold)
        out_indices, row_of_in, n_out = focal_cells(indices, s, fore, batch_size, spatial_shape, threshold, capacity)
        dev = features.device
        out = torch.empty((n_out, C), dtype=torch.float32, device=dev)
        w = torch.empty((n,), dtype=torch.float32, device=dev)
        cnt = torch.empty((n,), dtype=torch.int32, device=dev)
        _lib.launch("sv_focal_place", _lib.ptr(features), _lib.ptr(s), _lib.ptr(indices), _lib.ptr(fore), _lib.ptr(nbr), _lib.ptr(row_of_in), n, C,
                    int(bool(mask_multi)), int(bool(skip_mask_kernel)), float(threshold), n_out, _lib.ptr(w), _lib.ptr(cnt), _lib.ptr(out))
        ctx.save_for_backward(features, s, indices, fore, nbr, row_of_in, w, cnt)
        ctx.flags = (int(bool(mask_multi)), int(bool(skip_mask_kernel)), float(threshold))
        ctx.mark_non_differentiable(out_indices, fore, row_of_in)
        return out, out_indices, fore, row_of_in

    @staticmethod
    def backward(ctx, grad_out, _gi, _gf, _gr):
        features, s, indices, fore, nbr, row_of_in, w, cnt = ctx.saved_tensors
        mask_multi, skip_mask_kernel, threshold = ctx.flags
        n, C = features.shape
        grad_out = grad_out.contiguous().float()
        grad_f = torch.empty_like(features)
        grad_s = torch.empty_like(s)
        dots = torch.empty((n,), dtype=torch.float32, device=features.device)
        _lib.launch("sv_focal_backward", _lib.ptr(grad_out), _lib.ptr(features), _lib.ptr(s), _lib.ptr(indices), _lib.ptr(fore), _lib.ptr(nbr),
                    _lib.ptr(row_of_in), _lib.ptr(w), _lib.ptr(cnt), n, C, mask_multi, skip_mask_kernel, threshold, _lib.ptr(dots), _lib.ptr(grad_f),
                    _lib.ptr(grad_s))
        return grad_f, grad_s, None, None, None, None, None, None, None, None, None


def focal_expand(x, s, nbr, topk=False, threshold=0.5, mask_multi=False, skip_mask_kernel=False, capacity=None):
    """The expanded SparseConvTensor of `x` under the importance map s (n, 27): int32 indices in canonical order, the input's grid and indice_dict
    carried along as SparseConvolution.forward does.  -> (tensor, fore, row_of_in)"""
    assert isinstance(x, SparseConvTensor)
    out, out_indices, fore, row_of_in = FocalExpandFunction.apply(x.features, s, x.indices, nbr, x.batch_size, x.spatial_shape, topk, threshold,
                                                                  mask_multi, skip_mask_kernel, capacity)
    return SparseConvTensor(out, out_indices, x.spatial_shape, x.batch_size, x.grid, x.indice_dict), fore, row_of_in


# ---- the image branch (csrc/focal_image.hip): FocalSparseConv.construct_multimodal_features, focal_sparse_conv.py:50-113 ----
def image_aug_table(batch_dict, batch_size, device):
    """(B, 4) fp32 [noise_scale, noise_rot, flip_x, flip_y] from the keys the batch carries (focal_sparse_conv.py:83-90); identity values stand in
    for absent keys.  Device tensors stay on the device: no read."""
    identity = (1.0, 0.0, 0.0, 0.0)
    cols = []
    for key, fill in zip(('noise_scale', 'noise_rot', 'flip_x', 'flip_y'), identity):
        if key in batch_dict:
            cols.append(torch.as_tensor(batch_dict[key]).to(device=device, dtype=torch.float32).reshape(batch_size))
        else:
            cols.append(torch.full((batch_size,), fill, dtype=torch.float32, device=device))
    return torch.stack(cols, dim=1).contiguous()


def focal_image_pixels(indices, batch_size, voxel_stride, voxel_size, origin, calib_table, aug_table, image_hw):
    """pix (n) int32 = v * W + u of every row's projection into its scene's image, -1 outside (sv_focal_image_pixels).  voxel_size / origin: the
    layer's z-first host values; calib_table (B, 24), aug_table (B, 4) fp32 on the device.  No host read."""
    assert indices.dtype == torch.int32 and indices.dim() == 2 and indices.shape[1] == 4, "indices: (n, 4) int32 [b, z, y, x]"
    assert calib_table.dtype == torch.float32 and calib_table.shape == (batch_size, 24), "calib_table: (B, 24) fp32 = [V2C^T R0^T (4 x 3) | P2 (3 x 4)]"
    assert aug_table.dtype == torch.float32 and aug_table.shape == (batch_size, 4), "aug_table: (B, 4) fp32"
    indices = indices.contiguous()
    n = indices.shape[0]
    pix = torch.empty((n,), dtype=torch.int32, device=indices.device)
    vs = _lib.host_array(ctypes.c_float, [float(v) for v in voxel_size])
    org = _lib.host_array(ctypes.c_float, [float(v) for v in origin])
    _lib.launch("sv_focal_image_pixels", _lib.ptr(indices), n, int(batch_size), int(voxel_stride), vs, org, _lib.ptr(calib_table.contiguous()),
                _lib.ptr(aug_table.contiguous()), int(image_hw[0]), int(image_hw[1]), _lib.ptr(pix))
    return pix


class FocalImageSampleFunction(torch.autograd.Function):
    """(f (n, Cv), image features (B, h, w, C) channel-last) -> [img | f] (n, C + Cv), or f + img (n, Cv) under fuse_sum, where img is the row of
    the features bilinearly up-sampled to image_hw at the row's pixel (sv_focal_image_sample).  indices and pix are constant.  The gradient into
    the features is sv_focal_image_sample_grad: per-pixel lists in ascending key order, no float atomics, equal bits run to run."""

    @staticmethod
    def forward(ctx, f, features, indices, pix, image_hw, fuse_sum):
        f, features, indices, pix = f.contiguous().float(), features.contiguous().float(), indices.contiguous(), pix.contiguous()
        (n, Cv), (B, h, w, C) = f.shape, features.shape
        assert indices.dtype == torch.int32 and indices.shape == (n, 4) and pix.dtype == torch.int32 and pix.shape == (n,)
        mode = int(bool(fuse_sum))
        H, W = int(image_hw[0]), int(image_hw[1])
        out = torch.empty((n, Cv if mode else C + Cv), dtype=torch.float32, device=f.device)
        _lib.launch("sv_focal_image_sample", _lib.ptr(features), B, h, w, C, H, W, _lib.ptr(f), Cv, _lib.ptr(indices), _lib.ptr(pix), n, mode, _lib.ptr(out))
        ctx.save_for_backward(indices, pix)
        ctx.geom = (B, h, w, C, H, W, Cv, mode)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        indices, pix = ctx.saved_tensors
        B, h, w, C, H, W, Cv, mode = ctx.geom
        n = indices.shape[0]
        g = grad_out.contiguous().float()
        grad_f = (g if mode else g[:, C:]) if ctx.needs_input_grad[0] else None
        grad_features = None
        if ctx.needs_input_grad[1]:
            nbytes = lib.sv_focal_image_sample_grad_scratch_bytes(n, B, h, w, H, W)
            if nbytes == 0:
                raise _lib.SeevcnHipError("sv_focal_image_sample_grad: pixel index or tap key exceeds int32")
            scratch = _lib.workspace.scratch("focal_image_grad", nbytes, g.device)
            grad_features = torch.empty((B, h, w, C), dtype=torch.float32, device=g.device)
            _lib.launch("sv_focal_image_sample_grad", _lib.ptr(g), g.shape[1], _lib.ptr(indices), _lib.ptr(pix), n, B, h, w, C, H, W, _lib.ptr(scratch),
                        _lib.ptr(grad_features))
        return grad_f, grad_features, None, None, None, None


def focal_image_fuse(f, features_nhwc, indices, pix, image_hw, fuse_sum=False):
    """The fused rows of construct_multimodal_features for rows `indices` whose pixels are `pix` (focal_image_pixels)."""
    return FocalImageSampleFunction.apply(f, features_nhwc, indices, pix, image_hw, fuse_sum)
