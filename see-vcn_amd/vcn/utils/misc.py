import torch

from ... import _lib


def fps(data, number):
    """data (B,N,3) -> (B,number,3): farthest point sampling from point 0 + gather (reference utils/misc.py:29-36, which calls the
    third-party pointnet2_ops; same algorithm as the in-tree pointnet2_batch sampling kernel) on sv_farthest_point_sampling."""
    _lib.require_cuda(data)
    x = data.detach().float().contiguous()
    B, N, _ = x.shape
    idx = torch.empty((B, number), dtype=torch.int32, device=x.device)
    from ...pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda import farthest_point_sampling_wrapper
    farthest_point_sampling_wrapper(B, N, int(number), x, None, idx)
    return torch.gather(data, 1, idx.long().unsqueeze(-1).expand(-1, -1, data.shape[2])).contiguous()
