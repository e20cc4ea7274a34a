"""Autograd functions / modules with the reference's names and call signatures
(detector3d/pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py:8-188, 264-453)."""
import numbers

import torch
import torch.nn as nn
from torch.autograd import Function

from . import pointnet2_stack_cuda as pointnet2


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
        assert new_xyz.is_contiguous() and new_xyz_batch_cnt.is_contiguous()
        assert xyz.is_contiguous() and xyz_batch_cnt.is_contiguous()
        B = xyz_batch_cnt.shape[0]
        M = new_xyz.shape[0]
        idx = torch.zeros((M, nsample), dtype=torch.int32, device=new_xyz.device)
        pointnet2.ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx)
        empty_ball_mask = (idx[:, 0] == -1)
        idx[empty_ball_mask] = 0
        ctx.mark_non_differentiable(idx)
        ctx.mark_non_differentiable(empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None


ball_query = BallQuery.apply


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features, features_batch_cnt, idx, idx_batch_cnt):
        assert features.is_contiguous() and features_batch_cnt.is_contiguous()
        assert idx.is_contiguous() and idx_batch_cnt.is_contiguous()
        assert features.shape[0] == features_batch_cnt.sum(), \
            'features: %s, features_batch_cnt: %s' % (str(features.shape), str(features_batch_cnt))
        assert idx.shape[0] == idx_batch_cnt.sum(), 'idx: %s, idx_batch_cnt: %s' % (str(idx.shape), str(idx_batch_cnt))
        M, nsample = idx.size()
        N, C = features.size()
        B = idx_batch_cnt.shape[0]
        output = torch.empty((M, C, nsample), dtype=torch.float32, device=features.device)
        pointnet2.group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, output)
        ctx.for_backwards = (B, N, idx, features_batch_cnt, idx_batch_cnt)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        B, N, idx, features_batch_cnt, idx_batch_cnt = ctx.for_backwards
        M, C, nsample = grad_out.size()
        grad_features = torch.empty((N, C), dtype=torch.float32, device=grad_out.device)
        pointnet2.group_points_grad_wrapper(B, M, C, N, nsample, grad_out.contiguous(), idx, idx_batch_cnt, features_batch_cnt,
                                            grad_features)
        return grad_features, None, None, None


grouping_operation = GroupingOperation.apply


class SAScaleTrain(Function):
    """One radius scale of StackSAModuleMSG in TRAINING mode as one autograd node over the hand-written MFMA kernels
    (sv_sa_train_forward / sv_sa_train_backward, csrc/set_abstraction_train.hip): gather -> Conv2d 1x1 -> BatchNorm2d(batch statistics) ->
    ReLU, twice -> max over nsample (pointnet2_modules.py:96-110), without the (M, C+3, nsample) tensor; running statistics and
    num_batches_tracked of the two norms are updated like nn.BatchNorm2d does.  idx / row_start as ball_query_wrapper leaves them."""

    @staticmethod
    def forward(ctx, xyz, features, new_xyz, idx, row_start, w1, g1, b1, w2, g2, b2, rm1, rv1, nbt1, rm2, rv2, nbt2, momentum, eps):
        from ..... import _lib
        lib = _lib.load()
        dev = xyz.device
        M, ns = idx.shape
        C = 0 if features is None else features.shape[1]
        C1, C2 = w1.shape[0], w2.shape[0]
        w1c, w2c = w1.detach().reshape(C1, C + 3).contiguous(), w2.detach().reshape(C2, C1).contiguous()
        R = M * ns
        f32 = dict(dtype=torch.float32, device=dev)
        N = xyz.shape[0]
        proj = torch.empty((N, C1), **f32) if C else None                     # layer 1's feature part, once per support point (work buffer)
        z1, z2 = torch.empty((R, C1), **f32), torch.empty((R, C2), **f32)
        stats = torch.empty((2 * C1 + 2 * C2,), **f32)
        sm1, si1, sm2, si2 = stats[:C1], stats[C1:2 * C1], stats[2 * C1:2 * C1 + C2], stats[2 * C1 + C2:]
        sel, aux, out = torch.empty((M, C2), **f32), torch.empty((M, C2), **f32), torch.empty((M, C2), **f32)
        arg, aux_arg = torch.empty((M, C2), dtype=torch.uint8, device=dev), torch.empty((M, C2), dtype=torch.uint8, device=dev)
        scratch = _lib.workspace.scratch("sa_train", lib.sv_sa_train_scratch_bytes(C, C1, C2), dev)
        _lib.launch("sv_sa_train_forward", _lib.ptr(xyz), _lib.ptr(features) if C else None, _lib.ptr(new_xyz), _lib.ptr(idx), _lib.ptr(row_start), M, N, C, ns,
                    _lib.ptr(w1c), _lib.ptr(g1.detach()), _lib.ptr(b1.detach()), _lib.ptr(rm1), _lib.ptr(rv1), _lib.ptr(nbt1), C1, _lib.ptr(w2c),
                    _lib.ptr(g2.detach()), _lib.ptr(b2.detach()), _lib.ptr(rm2), _lib.ptr(rv2), _lib.ptr(nbt2), C2, float(momentum), float(eps),
                    _lib.ptr(scratch), _lib.ptr(proj), _lib.ptr(z1), _lib.ptr(z2), _lib.ptr(sm1), _lib.ptr(si1), _lib.ptr(sm2), _lib.ptr(si2), _lib.ptr(sel),
                    _lib.ptr(aux), _lib.ptr(arg), _lib.ptr(aux_arg), _lib.ptr(out))
        ctx.save_for_backward(xyz, features, new_xyz, idx, row_start, w1c, g1, b1, w2c, g2, b2, z1, z2, stats, sel, arg, out)
        ctx.w_shapes = (w1.shape, w2.shape)
        ctx.mark_non_differentiable(idx)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from ..... import _lib, ordered
        lib = _lib.load()
        xyz, features, new_xyz, idx, row_start, w1c, g1, b1, w2c, g2, b2, z1, z2, stats, sel, arg, out = ctx.saved_tensors
        dev = xyz.device
        M, ns = idx.shape
        C = 0 if features is None else features.shape[1]
        N = xyz.shape[0]
        C1, C2 = w1c.shape[0], w2c.shape[0]
        sm1, si1, sm2, si2 = stats[:C1], stats[C1:2 * C1], stats[2 * C1:2 * C1 + C2], stats[2 * C1 + C2:]
        f32 = dict(dtype=torch.float32, device=dev)
        dy1, aux = torch.empty((M * ns, C1), **f32), torch.empty((M, C2), **f32)
        scatter = torch.empty((N, C1), **f32) if C else None
        gf = torch.empty((N, C), **f32) if C and ctx.needs_input_grad[1] else None
        gw1, gw2 = torch.empty((C1, C + 3), **f32), torch.empty((C2, C1), **f32)
        gbn = torch.empty((2 * C1 + 2 * C2,), **f32)
        dg1, db1, dg2, db2 = gbn[:C1], gbn[C1:2 * C1], gbn[2 * C1:2 * C1 + C2], gbn[2 * C1 + C2:]
        if ordered.ordered_gradients():                   # the scatter summed in ascending (query, slot) order instead of float atomics
            name = "sv_sa_train_backward_ordered"
            scratch = _lib.workspace.scratch("sa_train_ordered", lib.sv_sa_train_backward_ordered_scratch_bytes(M, N, C, ns, C1, C2), dev)
            ordered.count_call("sa_train")
        else:
            name = "sv_sa_train_backward"
            scratch = _lib.workspace.scratch("sa_train", lib.sv_sa_train_scratch_bytes(C, C1, C2), dev)
        _lib.launch(name, _lib.ptr(xyz), _lib.ptr(features) if C else None, _lib.ptr(new_xyz), _lib.ptr(idx), _lib.ptr(row_start), M, N, C,
                    ns, _lib.ptr(w1c), _lib.ptr(g1.detach()), _lib.ptr(b1.detach()), C1, _lib.ptr(w2c), _lib.ptr(g2.detach()),
                    _lib.ptr(b2.detach()), C2, _lib.ptr(z1), _lib.ptr(z2), _lib.ptr(sm1), _lib.ptr(si1), _lib.ptr(sm2), _lib.ptr(si2),
                    _lib.ptr(sel), _lib.ptr(arg), _lib.ptr(out), _lib.ptr(grad_out.contiguous()), _lib.ptr(scratch), _lib.ptr(dy1),
                    _lib.ptr(aux), _lib.ptr(scatter), _lib.ptr(gf), _lib.ptr(gw1), _lib.ptr(gw2), _lib.ptr(dg1), _lib.ptr(db1), _lib.ptr(dg2),
                    _lib.ptr(db2))
        s1, s2 = ctx.w_shapes
        return (None, gf, None, None, None, gw1.view(s1), dg1, db1, gw2.view(s2), dg2, db2, None, None, None, None, None, None, None, None)


sa_scale_train = SAScaleTrain.apply


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None):
        """xyz (N1+N2..,3), new_xyz (M1+M2..,3), features (N1+N2..,C) -> new_features (M1+M2.., C(+3), nsample), idx"""
        assert xyz.shape[0] == xyz_batch_cnt.sum(), 'xyz: %s, xyz_batch_cnt: %s' % (str(xyz.shape), str(new_xyz_batch_cnt))
        assert new_xyz.shape[0] == new_xyz_batch_cnt.sum(), \
            'new_xyz: %s, new_xyz_batch_cnt: %s' % (str(new_xyz.shape), str(new_xyz_batch_cnt))
        idx, empty_ball_mask = ball_query(self.radius, self.nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        grouped_xyz = grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)  # (M, 3, nsample)
        grouped_xyz = grouped_xyz - new_xyz.unsqueeze(-1)
        grouped_xyz[empty_ball_mask] = 0
        if features is not None:
            grouped_features = grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)  # (M, C, nsample)
            grouped_features[empty_ball_mask] = 0
            new_features = torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features
        else:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            new_features = grouped_xyz
        return new_features, idx


class FarthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        """xyz (B,N,3) -> (B,npoint) int32 (reference pointnet2_utils.py:162-188)"""
        assert xyz.is_contiguous()
        B, N, _ = xyz.size()
        output = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
        temp = torch.empty((B, N), dtype=torch.float32, device=xyz.device) if N > 24576 else None
        pointnet2.farthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output)
        return output

    @staticmethod
    def backward(xyz, a=None):
        return None, None


farthest_point_sample = furthest_point_sample = FarthestPointSampling.apply


class StackFarthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, xyz_batch_cnt, npoint):
        """xyz (N1 + N2 + ..., 3), xyz_batch_cnt [N1, N2, ...], npoint int | list | tensor [M1, M2, ...] -> (M1 + M2 + ...) int32 GLOBAL rows
        (reference pointnet2_utils.py:191-227).  One launch over the device counts; the output is sized from a host npoint, or -- a device tensor
        being what the reference's sector_fps hands over -- from one read of its sum."""
        assert xyz.is_contiguous() and xyz.shape[1] == 3
        batch_size = xyz_batch_cnt.shape[0]
        dev = xyz.device
        if not torch.is_tensor(npoint):
            if isinstance(npoint, numbers.Integral):
                npoint = [int(npoint)] * batch_size
            total = int(sum(npoint))
            npoint = torch.tensor(npoint, dtype=torch.int32).to(dev, non_blocking=True)
        else:
            npoint = npoint.to(device=dev, dtype=torch.int32).contiguous()
            total = int(npoint.sum().item())
        assert npoint.shape[0] == batch_size
        cnt = xyz_batch_cnt.to(device=dev, dtype=torch.int32).contiguous()
        start = (torch.cumsum(cnt, 0, dtype=torch.int32) - cnt).contiguous()
        out_start = (torch.cumsum(npoint, 0, dtype=torch.int32) - npoint).contiguous()
        output = torch.empty((total,), dtype=torch.int32, device=dev)
        pointnet2.stack_farthest_point_sampling_ragged(xyz, None, start, cnt, npoint, out_start, output)
        return output

    @staticmethod
    def backward(xyz, a=None):
        return None, None, None


def stack_farthest_point_sample(points, xyz_batch_cnt, npoint, max_n=None, bucketed=True):
    """An int npoint: the (batch, npoint) table of the seevcn extension (pointnet2_stack_cuda.stack_farthest_point_sampling, what VoxelSetAbstraction's
    FPS route uses).  A list or tensor npoint: the reference's StackFarthestPointSampling, flat (sum npoint)."""
    if isinstance(npoint, numbers.Integral):                       # Python and numpy integers alike
        return pointnet2.stack_farthest_point_sampling(points, xyz_batch_cnt, npoint, max_n, bucketed)
    return StackFarthestPointSampling.apply(points, xyz_batch_cnt, npoint)


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features (M1 + M2 ..., C), idx / weight (N1 + N2 ..., 3) -> (N1 + N2 ..., C)   (reference pointnet2_utils.py:264-303)"""
        assert idx.shape[0] == weight.shape[0] and idx.shape[1] == weight.shape[1] == 3
        idx, weight = idx.contiguous(), weight.contiguous()
        ctx.three_interpolate_for_backward = (idx, weight, features.shape[0])
        output = torch.empty((idx.shape[0], features.shape[1]), dtype=torch.float32, device=features.device)
        pointnet2.three_interpolate_wrapper(features.contiguous(), idx, weight, output)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight, M = ctx.three_interpolate_for_backward
        grad_features = torch.empty((M, grad_out.shape[1]), dtype=torch.float32, device=grad_out.device)
        pointnet2.three_interpolate_grad_wrapper(grad_out.contiguous(), idx, weight, grad_features)
        return grad_features, None, None


three_interpolate = ThreeInterpolate.apply


class ThreeNNForVectorPoolByTwoStep(Function):
    @staticmethod
    def forward(ctx, support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt,
                max_neighbour_distance, nsample, neighbor_type, avg_length_of_neighbor_idxs, num_total_grids,
                neighbor_distance_multiplier):
        """Same arguments as the reference (pointnet2_utils.py:306-358) -> (dist (M, G, 3), idx (M, G, 3) int32, avg_length_of_neighbor_idxs).
        One launch keeps each query's neighbour list on the chip, so nothing is counted, read back or retried: avg_length_of_neighbor_idxs
        is returned as it came."""
        assert new_xyz_grid_centers.shape[1] == num_total_grids
        idx, dist2 = pointnet2.vector_pool_three_nn(
            support_xyz.contiguous(), xyz_batch_cnt, new_xyz.contiguous(), new_xyz_grid_centers.contiguous(), new_xyz_batch_cnt,
            max_neighbour_distance * neighbor_distance_multiplier, nsample, neighbor_type)
        ctx.mark_non_differentiable(idx)
        return torch.sqrt(dist2), idx, avg_length_of_neighbor_idxs

    @staticmethod
    def backward(ctx, *grads):
        return (None,) * 11


three_nn_for_vector_pool_by_two_step = ThreeNNForVectorPoolByTwoStep.apply


class VectorPoolWithVoxelQuery(Function):
    @staticmethod
    def forward(ctx, support_xyz, xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, num_grid_x, num_grid_y, num_grid_z,
                max_neighbour_distance, num_c_out_each_grid, use_xyz, num_mean_points_per_grid=100, nsample=-1, neighbor_type=0,
                pooling_type=0):
        """Same arguments and the same four returns as the reference (pointnet2_utils.py:361-453): new_features (M, G * c_each),
        new_local_xyz (M, 3 G), num_mean_points_per_grid (returned as it came: nothing is counted), point_cnt_of_grid (M, G).
        Only pooling_type 1 (`voxel_random_choice`) is built; with one row per cell the reference's division by the count is a no-op."""
        assert support_xyz.is_contiguous() and support_features.is_contiguous() and xyz_batch_cnt.is_contiguous()
        assert new_xyz.is_contiguous() and new_xyz_batch_cnt.is_contiguous()
        if pooling_type != 1:
            raise NotImplementedError("vector_pool_with_voxel_query_op: only pooling_type 1 (voxel_random_choice) is built; no configuration "
                                      "selects voxel_avg_pool")
        N, num_c_in = support_features.shape
        assert num_c_in % num_c_out_each_grid == 0, \
            f'the input channels ({num_c_in}) should be an integral multiple of num_c_out_each_grid({num_c_out_each_grid})'
        choice, point_cnt_of_grid, new_local_xyz, new_features = pointnet2.vector_pool_choice(
            support_xyz, xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, num_grid_x, num_grid_y, num_grid_z,
            max_neighbour_distance, num_c_out_each_grid, nsample, neighbor_type)
        num_mean_points_per_grid = torch.Tensor([num_mean_points_per_grid]).int()
        ctx.vector_pool_for_backward = (point_cnt_of_grid, choice, N, num_c_in)
        ctx.mark_non_differentiable(new_local_xyz, num_mean_points_per_grid, point_cnt_of_grid)
        return new_features, new_local_xyz, num_mean_points_per_grid, point_cnt_of_grid

    @staticmethod
    def backward(ctx, grad_new_features, grad_local_xyz, grad_num_cum_sum, grad_point_cnt_of_grid):
        point_cnt_of_grid, choice, N, num_c_in = ctx.vector_pool_for_backward
        grad_support_features = pointnet2.vector_pool_choice_grad(grad_new_features.contiguous(), choice, point_cnt_of_grid, N, num_c_in)
        return (None, None, grad_support_features) + (None,) * 12


vector_pool_with_voxel_query_op = VectorPoolWithVoxelQuery.apply
