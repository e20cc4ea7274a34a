"""TEST INFRASTRUCTURE: a float64 torch-CPU restatement of the dense-batch PointNet++ modules (set abstraction with multi-scale grouping, group-all,
feature propagation), written from the statements of the operations.  The index ops (farthest point sampling, ball query, 3-NN) come from
oracle/pointnet2.py, which tests/test_pointnet2.py pins to the HIP ops; everything that carries values or gradients is float64 autograd here.

  SA scale    idx = ball query (first nsample hits, padded with the first hit, all 0 for an empty ball); grouped = [xyz[idx] - new_xyz |
              features[idx]] (xyz first, only with use_xyz); per layer Conv 1x1 (no bias) -> BatchNorm (training: batch statistics over
              B * npoint * nsample, biased variance; eval: running statistics) -> ReLU; max or mean over nsample; scales concatenated on channels
  group-all   npoint None: ONE group of all N points around the origin, new_xyz None
  FP          3-NN inverse-distance weights w_k = (1 / (d_k + 1e-8)) / sum (constants for autograd), interpolated = sum_k w_k known_feats[idx_k];
              known None: known_feats (B, C, 1) repeated; concatenated IN FRONT of the skip features; the same layer stack
"""
import numpy as np
import torch

from oracle import pointnet2 as opn

D = torch.float64


def params64(module):
    """name -> float64 leaf copies of a module's parameters (requires_grad) and buffers."""
    out = {k: v.detach().cpu().to(D).requires_grad_(True) for k, v in module.named_parameters()}
    out.update({k: v.detach().cpu().to(D) for k, v in module.named_buffers() if v.is_floating_point()})
    return out


def shared_mlp(x, p, prefix, training, eps=1e-5):
    """x (B, C, H, W) through the Conv2d / BatchNorm2d / ReLU triples stored under prefix + '0', '1', '3', '4', ..."""
    k = 0
    while f"{prefix}{3 * k}.weight" in p:
        x = torch.einsum("oi,bihw->bohw", p[f"{prefix}{3 * k}.weight"][:, :, 0, 0], x)
        bn = f"{prefix}{3 * k + 1}."
        if training:
            mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        else:
            mean, var = p[bn + "running_mean"], p[bn + "running_var"]
        x = (x - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * p[bn + "weight"].view(1, -1, 1, 1) + p[bn + "bias"].view(1, -1, 1, 1)
        x = torch.relu(x)
        k += 1
    assert k > 0, prefix
    return x


def _pool(x, pool_method):
    return x.max(dim=3)[0] if pool_method == "max_pool" else x.mean(dim=3)


def sa_forward(p, xyz, features, npoint, radii, nsamples, use_xyz=True, pool_method="max_pool", training=False):
    """xyz (B, N, 3) float64 (fp32 values), features (B, C, N) float64 or None -> (new_xyz (B, npoint, 3) or None, new_features (B, sum C_k, npoint))"""
    B, N, _ = xyz.shape
    xyz32 = xyz.detach().numpy().astype(np.float32)
    outs = []
    if npoint is None:
        g = xyz.transpose(1, 2).unsqueeze(2)                                                   # (B, 3, 1, N)
        g = g if features is None else (torch.cat([g, features.unsqueeze(2)], dim=1) if use_xyz else features.unsqueeze(2))
        return None, _pool(shared_mlp(g, p, "mlps.0.", training), pool_method)
    fps = torch.from_numpy(np.stack([opn.farthest_point_sampling(xyz32[b], npoint) for b in range(B)]).astype(np.int64))
    bidx = torch.arange(B).view(B, 1)
    new_xyz = xyz[bidx, fps]                                                                   # (B, npoint, 3)
    new32 = new_xyz.detach().numpy().astype(np.float32)
    for k, (radius, nsample) in enumerate(zip(radii, nsamples)):
        idx = torch.from_numpy(opn.ball_query_batch(radius, nsample, xyz32, new32).astype(np.int64))     # (B, npoint, nsample)
        b3 = torch.arange(B).view(B, 1, 1)
        g = (xyz[b3, idx] - new_xyz.unsqueeze(2)).permute(0, 3, 1, 2)                          # (B, 3, npoint, nsample)
        if features is not None:
            gf = features.transpose(1, 2)[b3, idx].permute(0, 3, 1, 2)                         # (B, C, npoint, nsample)
            g = torch.cat([g, gf], dim=1) if use_xyz else gf
        outs.append(_pool(shared_mlp(g, p, f"mlps.{k}.", training), pool_method))
    return new_xyz, torch.cat(outs, dim=1)


def fp_forward(p, unknown, known, unknow_feats, known_feats, training=False):
    """unknown (B, n, 3), known (B, m, 3) or None, unknow_feats (B, C1, n) or None, known_feats (B, C2, m) -> (B, C_out, n)"""
    B, n, _ = unknown.shape
    if known is not None:
        with torch.no_grad():
            u32, k32 = unknown.numpy().astype(np.float32), known.numpy().astype(np.float32)
            idx = torch.from_numpy(np.stack([opn.three_nn(u32[b], k32[b])[1] for b in range(B)]).astype(np.int64))       # (B, n, 3)
            b3 = torch.arange(B).view(B, 1, 1)
            dist = (unknown.unsqueeze(2) - known[b3, idx]).norm(dim=-1)
            recip = 1.0 / (dist + 1e-8)
            weight = recip / recip.sum(dim=2, keepdim=True)
        interp = (known_feats.transpose(1, 2)[b3, idx] * weight.unsqueeze(-1)).sum(dim=2).transpose(1, 2)               # (B, C2, n)
    else:
        interp = known_feats.expand(B, known_feats.shape[1], n)
    x = interp if unknow_feats is None else torch.cat([interp, unknow_feats], dim=1)
    return shared_mlp(x.unsqueeze(-1), p, "mlp.", training).squeeze(-1)
