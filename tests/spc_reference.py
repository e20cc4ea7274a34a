"""numpy restatement of PV-RCNN++'s sectorized proposal-centric keypoint sampling, every fp32 operation rounded to fp32.

Written from the reference's statements (backbones_3d/pfe/voxel_set_abstraction.py:45-121, 206-225 and the stacked FPS kernel,
pointnet2_stack/src/sampling_gpu.cu:188-319), not from the HIP kernels:

  select     dist_j = sqrt(dx*dx + dy*dy + dz*dz) summed left to right, nearest RoI = lowest index among equal dist,
             selected iff dist < sqrt((l/2)^2 + (w/2)^2 + (h/2)^2) + radius of that RoI (strict)
  sector     floor((atan2(y, x) + fp32(pi)) / fp32(2 pi / S)) clamped to [0, S]; the axis cases take their IEEE 754 values
  partition  stable rows per (scene, sector), quota min(cnt, ceil(cnt / n_sel * K)) in float64, the two fallbacks
  fps        the kernel's own loop over 1024 slots and its lower-slot-wins tree, slot by slot (no closed-form tie key)
"""
import math

import numpy as np

F = np.float32
PI_F = F(np.pi)
T = 1024                     # the stacked kernel always runs 1024 threads (sampling_gpu.cu:340)


def roi_threshold(rois, radius):
    """fp32 (M,) sqrt((l/2)^2 + (w/2)^2 + (h/2)^2) + radius"""
    h = (rois[:, 3:6].astype(F) / F(2)).astype(F)
    s = (h[:, 0] * h[:, 0]).astype(F)
    s = (s + (h[:, 1] * h[:, 1]).astype(F)).astype(F)
    s = (s + (h[:, 2] * h[:, 2]).astype(F)).astype(F)
    return (np.sqrt(s).astype(F) + F(radius)).astype(F)


def select_mask(points, rois, radius, return_parts=False):
    """points (N, 3), rois (M, 7 + C) of ONE scene -> bool (N,)"""
    p, c = points[:, None, 0:3].astype(F), rois[None, :, 0:3].astype(F)
    d = (p - c).astype(F)
    s = (d[..., 0] * d[..., 0]).astype(F)
    s = (s + (d[..., 1] * d[..., 1]).astype(F)).astype(F)
    s = (s + (d[..., 2] * d[..., 2]).astype(F)).astype(F)
    dist = np.sqrt(s).astype(F)                               # numpy's fp32 sqrt is correctly rounded
    j = np.argmin(dist, axis=1)                               # first of the equal minima
    dmin = dist[np.arange(len(points)), j]
    thr = roi_threshold(rois, radius)[j]
    mask = dmin < thr
    return (mask, dmin, thr) if return_parts else mask


def angle(x, y):
    """fp32 atan2(y, x): the axis cases by IEEE 754, everything else the float64 value rounded once"""
    x, y = np.asarray(x, F), np.asarray(y, F)
    a = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F)
    xneg = (x < 0) | ((x == 0) & np.signbit(x))
    a = np.where(y == 0, np.copysign(np.where(xneg, PI_F, F(0)), y), a)
    a = np.where((x == 0) & (y != 0), np.copysign(F(np.pi / 2), y), a)
    return a.astype(F)


def sector_quotient(points, S):
    """float64 (N,) value of (atan2(y, x) + pi) / (2 pi / S): how far a row is from a sector edge"""
    a = np.arctan2(points[:, 1].astype(np.float64), points[:, 0].astype(np.float64))
    return (a + np.pi) / (np.pi * 2 / S)


def sector_of(points, S):
    """int32 (N,) in [0, S]"""
    size = F(np.pi * 2 / S)
    q = ((angle(points[:, 0], points[:, 1]) + PI_F).astype(F) / size).astype(F)
    return np.clip(np.floor(q), 0, S).astype(np.int32)


def select(xyz, start, cnt, rois, radius, S):
    """stacked xyz (N, 3), rois (B, M, 7 + C) -> sector (N,) int32: -1 | 0..S (S == 0: 0 | -1)"""
    out = np.full(len(xyz), -1, np.int32)
    for b, (s, n) in enumerate(zip(start, cnt)):
        pts = xyz[s:s + n]
        mask = select_mask(pts, rois[b], radius)
        sec = sector_of(pts, S) if S > 0 else np.zeros(n, np.int32)
        out[s:s + n] = np.where(mask, sec, -1)
    return out


def partition(sector, xyz, start, cnt, K, S):
    """-> dict(order (N,) with -1 where nothing is defined, seg_start / seg_cnt / seg_m / seg_out_start (B * max(S, 1),), kp_cnt (B,))"""
    B, nseg = len(cnt), max(S, 1)
    order = np.full(len(sector), -1, np.int32)
    tab = {k: np.zeros(B * nseg, np.int32) for k in ("seg_start", "seg_cnt", "seg_m", "seg_out_start")}
    kp = np.zeros(B, np.int32)
    for b, (st, n) in enumerate(zip(start, cnt)):
        sec = sector[st:st + n]
        rows = [st + np.nonzero(sec == s)[0] for s in range(S + 1)]           # ascending original rows
        pos = st
        bucket_start = []
        for r in rows:
            order[pos:pos + len(r)] = r
            bucket_start.append(pos)
            pos += len(r)
        n_sel = int((sec >= 0).sum())
        if S == 0:
            tab["seg_start"][b], tab["seg_cnt"][b], kp[b] = st, n_sel, n_sel
            continue
        segs = [(st, 0, 0)] * S
        if n == 0:
            pass
        elif n_sel == 0:                                                     # points[:1]
            s0 = int(sector_of(xyz[st:st + 1], S)[0])
            order[st] = st
            segs[s0 if s0 < S else 0] = (st, 1, min(1, math.ceil(1 / 1 * K)) if s0 < S else K)
        elif all(len(r) == 0 for r in rows[:S]):                             # 'empty sector points': all of them, quota K
            segs[0] = (bucket_start[S], n_sel, K)
        else:
            segs = [(bucket_start[s], len(rows[s]), min(len(rows[s]), math.ceil(len(rows[s]) / n_sel * K))) for s in range(S)]
        out = b * (K + S)
        for s, (a, c, m) in enumerate(segs):
            g = b * S + s
            tab["seg_start"][g], tab["seg_cnt"][g], tab["seg_m"][g], tab["seg_out_start"][g] = a, c, m, out
            out += m
        kp[b] = out - b * (K + S)
    return dict(order=order, kp_cnt=kp, **tab)


def fps_segment(pts, m):
    """The stacked kernel's loop for one segment: pts (n, 3) fp32 in segment order -> m positions (int64).  1024 slots; slot t scans k = t, t + 1024,
    ... with a strict '>' from best = -1 / besti = 0; the tree keeps the LOWER slot on equal values (__update: v2 > v1 ? i2 : i1)."""
    n = len(pts)
    if n == 0 or m <= 0:
        return np.zeros(0, np.int64)
    pts = pts.astype(F)
    temp = np.full(n, 1e10, F)
    rounds = (n + T - 1) // T
    pad = rounds * T - n
    out = np.zeros(m, np.int64)
    old = 0
    for j in range(1, m):
        d = (pts - pts[old]).astype(F)
        s = (d[:, 0] * d[:, 0]).astype(F)
        s = (s + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
        s = (s + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        temp = np.minimum(s, temp)
        grid = np.concatenate([temp, np.full(pad, -1, F)]).reshape(rounds, T)      # [i, t] = temp[t + i * 1024]; absent rows can never pass '>'
        first = np.argmax(grid, axis=0)                                            # strict '>' keeps the first maximum of a slot's scan
        best = grid[first, np.arange(T)]
        besti = np.where(best > -1, np.arange(T) + first * T, 0)
        width = T // 2
        while width >= 1:
            v1, v2 = best[:width], best[width:2 * width]
            take = v2 > v1
            besti = np.where(take, besti[width:2 * width], besti[:width])
            best = np.maximum(v1, v2)
            width //= 2
        old = int(besti[0])
        out[j] = old
    return out


def fps_ragged(xyz, order, seg_start, seg_cnt, seg_m, seg_out_start, idx):
    """writes GLOBAL rows into idx (in place) like the kernel; order None = identity"""
    for a, c, m, o in zip(seg_start, seg_cnt, seg_m, seg_out_start):
        if c <= 0 or m <= 0:
            continue
        rows = order[a:a + c] if order is not None else np.arange(a, a + c)
        idx[o:o + m] = rows[fps_segment(xyz[rows], int(m))]
    return idx


def sample_batch(xyz, start, cnt, rois, radius, K, S):
    """The whole of get_sampled_points with SPC: -> (keypoint rows of every scene concatenated, kp_cnt (B,), sector, tables)"""
    sector = select(xyz, start, cnt, rois, radius, S)
    t = partition(sector, xyz, start, cnt, K, S)
    idx = np.full(len(cnt) * (K + S), -1, np.int64)
    fps_ragged(xyz, t["order"], t["seg_start"], t["seg_cnt"], t["seg_m"], t["seg_out_start"], idx)
    rows = np.concatenate([idx[b * (K + S):b * (K + S) + t["kp_cnt"][b]] for b in range(len(cnt))]) if len(cnt) else np.zeros(0, np.int64)
    return rows, t["kp_cnt"], sector, t


def stack_fps(xyz, xyz_batch_cnt, npoint):
    """StackFarthestPointSampling: (sum npoint,) global rows"""
    cnt = np.asarray(xyz_batch_cnt, np.int64)
    m = np.full(len(cnt), npoint, np.int64) if np.isscalar(npoint) else np.asarray(npoint, np.int64)
    start, ostart = np.cumsum(cnt) - cnt, np.cumsum(m) - m
    idx = np.zeros(int(m.sum()), np.int64)
    return fps_ragged(xyz, None, start, cnt, m, ostart, idx)
