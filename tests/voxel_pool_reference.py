"""CPU restatement of Voxel R-CNN's voxel RoI pooling, written from the behaviour of the reference (pointnet2_stack/src/voxel_query_gpu.cu:10-89,
voxel_query_utils.py, voxel_pool_modules.py, utils/common_utils.py:235-252): numpy, one loop per query, fp32 rounding at every step of the
distance, everything behind the query in float64."""
import numpy as np


def voxel2pinds(indices, batch_size, spatial_shape):
    """(batch_size, Z, Y, X) int32: -1 everywhere, r at [b, z, y, x] of row r of indices (N, 4)."""
    vol = np.full([int(batch_size)] + [int(s) for s in spatial_shape], -1, np.int32)
    ind = np.asarray(indices).astype(np.int64)
    vol[ind[:, 0], ind[:, 1], ind[:, 2], ind[:, 3]] = np.arange(len(ind), dtype=np.int32)
    return vol


def voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices, idx=None, return_counts=False):
    """idx (M, nsample) int32 as the kernel leaves it in a buffer the caller zero-filled (or in `idx`): the first nsample neighbours in visit
    order (dz outermost, dx innermost), later slots = the first one, idx[m][0] = -1 and the rest untouched for a query without one.
    return_counts: also the number of neighbours inside the radius per query, uncapped."""
    xyz, new_xyz = np.asarray(xyz, np.float32), np.asarray(new_xyz, np.float32)
    new_coords, vol = np.asarray(new_coords), np.asarray(point_indices)
    M = len(new_coords)
    _, R1, R2, R3 = vol.shape
    zr, yr, xr = (int(v) for v in max_range)
    out = np.zeros((M, nsample), np.int32) if idx is None else idx
    counts = np.zeros(M, np.int64)
    radius2 = np.float32(radius) * np.float32(radius)
    for m in range(M):
        b, cz, cy, cx = (int(v) for v in new_coords[m])
        q = new_xyz[m]
        cnt = 0
        for z in range(max(cz - zr, 0), min(cz + zr, R1 - 1) + 1):
            for y in range(max(cy - yr, 0), min(cy + yr, R2 - 1) + 1):
                row = vol[b, z, y, max(cx - xr, 0):max(min(cx + xr, R3 - 1) + 1, 0)]
                for j in row[row >= 0]:
                    p = xyz[j]
                    dx, dy, dz = np.float32(p[0] - q[0]), np.float32(p[1] - q[1]), np.float32(p[2] - q[2])
                    dist2 = np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))
                    if dist2 > radius2:
                        continue
                    counts[m] += 1
                    if cnt < nsample:
                        if cnt == 0:
                            out[m, :] = j
                        out[m, cnt] = j
                        cnt += 1
        if cnt == 0:
            out[m, 0] = -1
    return (out, counts) if return_counts else out


def post_process(idx):
    """VoxelQuery.forward behind the kernel: (idx with the rows of empty queries set to 0, empty mask)."""
    empty = idx[:, 0] == -1
    out = idx.copy()
    out[empty] = 0
    return out, empty


def voxel_pool_max(f_in, xyz, new_xyz, idx, wp, bp):
    """out[m][c] = max_s ReLU(f_in[idx[m][s]][c] + wp[c] . (xyz[idx[m][s]] - new_xyz[m]) + bp[c]) in float64; idx as the kernel wrote it,
    an empty query (idx[m][0] = -1) gives ReLU(bp)."""
    f_in, xyz, new_xyz, wp, bp = (np.asarray(a, np.float64) for a in (f_in, xyz, new_xyz, wp, bp))
    empty = idx[:, 0] < 0
    j = np.where(empty[:, None], 0, idx)
    pos = np.einsum('msk,ck->msc', xyz[j] - new_xyz[:, None, :], wp) + bp
    val = np.maximum(f_in[j] + pos, 0.0).max(axis=1)
    val[empty] = np.maximum(bp, 0.0)
    return val


def _bn(x, sd, prefix, train, eps=1e-5):
    """BatchNorm over the rows of x (rows, C): running statistics, or the rows' own (biased variance) in training"""
    w, b = sd[prefix + '.weight'], sd[prefix + '.bias']
    if train:
        mean, var = x.mean(axis=0), x.var(axis=0)
    else:
        mean, var = sd[prefix + '.running_mean'], sd[prefix + '.running_var']
    return (x - mean) / np.sqrt(var + eps) * w + b


def neighbor_voxel_sa(state_dict, idx_list, xyz, new_xyz, features, pool_method='max_pool', train=False):
    """NeighborVoxelSAModuleMSG.forward in float64 from its state_dict; idx_list[k] = the raw voxel_query result of scale k (GLOBAL rows).
    train: batch statistics in every norm (mlps_pos over all M * nsample grouped offsets, the zeroed ones of empty queries included)."""
    sd = {k: np.asarray(v, np.float64) for k, v in state_dict.items() if not k.endswith('num_batches_tracked')}
    xyz, new_xyz, features = (np.asarray(a, np.float64) for a in (xyz, new_xyz, features))
    outs = []
    for k, idx in enumerate(idx_list):
        f_in = _bn(features @ sd[f'mlps_in.{k}.0.weight'][:, :, 0].T, sd, f'mlps_in.{k}.1', train)                # (N, C1)
        empty = idx[:, 0] < 0
        j = np.where(empty[:, None], 0, idx)
        keep = (~empty)[:, None, None]
        g_feat = np.where(keep, f_in[j], 0.0)                                                                     # (M, ns, C1)
        g_xyz = np.where(keep, xyz[j] - new_xyz[:, None, :], 0.0)                                                 # (M, ns, 3)
        M, ns, _ = g_xyz.shape
        pos = _bn(g_xyz.reshape(M * ns, 3) @ sd[f'mlps_pos.{k}.0.weight'][:, :, 0, 0].T, sd, f'mlps_pos.{k}.1', train).reshape(M, ns, -1)
        x = np.maximum(g_feat + pos, 0.0)
        if pool_method == 'max_pool':
            x = x.max(axis=1)
        elif pool_method == 'avg_pool':
            x = x.mean(axis=1)
        else:
            raise NotImplementedError
        outs.append(np.maximum(_bn(x @ sd[f'mlps_out.{k}.0.weight'][:, :, 0].T, sd, f'mlps_out.{k}.1', train), 0.0))
    return np.concatenate(outs, axis=1)
