"""Set-abstraction and feature-propagation modules of the dense-batch PointNet++ (reference pointnet2_batch/pointnet2_modules.py:10-170): the
same class names, constructor keywords and state_dict keys (`mlps.<scale>.<layer>`, `mlp.<layer>`), over this package's pointnet2_utils (HIP
sampling, ball query, grouping, 3-NN, interpolation).  The 1x1 Conv2d + BatchNorm2d + ReLU stacks are torch modules on packed NCHW tensors.
Unlike the reference, a constructor never edits the `mlps` lists it is given (the reference adds 3 to the caller's first entry in place)."""
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import pointnet2_utils


def _shared_mlp(spec, bn=True):
    """Conv2d(1x1, no bias) + BatchNorm2d + ReLU per layer.  `bn` is accepted and, as in the reference (:90-97, :132-139), not looked at: its
    stacks always carry BatchNorm2d, and checkpoints of PointRCNN's USE_BN: False head hold those keys."""
    layers = []
    for c_in, c_out in zip(spec[:-1], spec[1:]):
        layers.append(nn.Conv2d(c_in, c_out, kernel_size=1, bias=False))
        layers.append(nn.BatchNorm2d(c_out))
        layers.append(nn.ReLU())
    return nn.Sequential(*layers)


class _PointnetSAModuleBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.npoint = None
        self.groupers = None
        self.mlps = None
        self.pool_method = 'max_pool'

    def forward(self, xyz: torch.Tensor, features: torch.Tensor = None, new_xyz=None) -> (torch.Tensor, torch.Tensor):
        """xyz (B, N, 3), features (B, C, N) or None -> new_xyz (B, npoint, 3) (None with npoint=None), new_features (B, sum_k mlps[k][-1], npoint)"""
        if new_xyz is None and self.npoint is not None:
            idx = pointnet2_utils.farthest_point_sample(xyz, self.npoint)
            new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        out = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            x = mlp(grouper(xyz, new_xyz, features))                        # (B, mlp[-1], npoint, nsample)
            if self.pool_method == 'max_pool':
                x = F.max_pool2d(x, kernel_size=[1, x.size(3)])
            elif self.pool_method == 'avg_pool':
                x = F.avg_pool2d(x, kernel_size=[1, x.size(3)])
            else:
                raise NotImplementedError
            out.append(x.squeeze(-1))
        return new_xyz, torch.cat(out, dim=1)


class PointnetSAModuleMSG(_PointnetSAModuleBase):
    """Set abstraction with multi-scale grouping: one ball query + shared MLP + pool per (radius, nsample, mlp) scale."""

    def __init__(self, *, npoint: int, radii: List[float], nsamples: List[int], mlps: List[List[int]], bn: bool = True, use_xyz: bool = True,
                 pool_method='max_pool'):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, mlp in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz) if npoint is not None
                                 else pointnet2_utils.GroupAll(use_xyz))
            spec = list(mlp)                                                # a copy: the caller's list stays as it was
            if use_xyz:
                spec[0] += 3
            self.mlps.append(_shared_mlp(spec, bn))
        self.pool_method = pool_method


class PointnetSAModule(PointnetSAModuleMSG):
    """Single-scale set abstraction; npoint=None groups all points around the origin (GroupAll)."""

    def __init__(self, *, mlp: List[int], npoint: int = None, radius: float = None, nsample: int = None, bn: bool = True, use_xyz: bool = True,
                 pool_method='max_pool'):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz, pool_method=pool_method)


class PointnetFPModule(nn.Module):
    """Feature propagation: inverse-distance interpolation from the three nearest known points, concatenation with the skip features, shared MLP."""

    def __init__(self, *, mlp: List[int], bn: bool = True):
        super().__init__()
        self.mlp = _shared_mlp(list(mlp), bn)

    def forward(self, unknown: torch.Tensor, known: torch.Tensor, unknow_feats: torch.Tensor, known_feats: torch.Tensor) -> torch.Tensor:
        """unknown (B, n, 3), known (B, m, 3) or None, unknow_feats (B, C1, n) or None, known_feats (B, C2, m) -> (B, mlp[-1], n)"""
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            dist_recip = 1.0 / (dist + 1e-8)
            weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
            interpolated = pointnet2_utils.three_interpolate(known_feats.contiguous(), idx, weight.contiguous())
        else:
            interpolated = known_feats.expand(*known_feats.size()[0:2], unknown.size(1))
        x = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
        return self.mlp(x.unsqueeze(-1)).squeeze(-1)
