"""TEST INFRASTRUCTURE: a numpy restatement of PointRCNN's RoI point pooling, written from the statements of the operation and not from the kernel
under test.

  in-box test   |z - cz| (fp32) > dz / 2 (double) -> outside; local x/y = the shift rotated by cos/sin(-rz) in fp32, every product and sum
                rounded; inside iff |lx| < dx / 2 + 1e-5 and |ly| < dy / 2 + 1e-5 (double compare, 1e-5 the fp32 constant); no margin on z
  list          of box (b, m): the rows of scene b that pass the test, ascending, cut after S
  flag          1 when the list is empty, and the box's S rows are zeros
  padding       with 0 < cnt < S, slot k >= cnt repeats slot k % cnt
  row s         [xyz[b, list[s]] | pts_feature[b, list[s]]], fp32 values copied
  canonical     the xyz columns hold the point in the box's frame: x, y = (p - centre) rotated by -heading in FLOAT64 (of the fp32 inputs), with
                the bound 8 * 2^-24 * (|sx| + |sy|), s = p - centre, that an fp32 evaluation keeps (one rounding for the subtraction, one per
                product, one for the sum, up to two ulp each for cosf / sinf: six, rounded up to eight); z = fp32(z) - fp32(cz), exact
"""
import numpy as np

F = np.float32


def inside_fp32(boxes, pts):
    """(M, N) bool: the fp32 statements of the in-box test for boxes (M, 7) and pts (N, 3)."""
    boxes, pts = np.asarray(boxes, F).reshape(-1, 7), np.asarray(pts, F).reshape(-1, 3)
    out = np.zeros((len(boxes), len(pts)), bool)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    margin = np.float64(F(1e-5))
    for m, box in enumerate(boxes):
        cx, cy, cz, dx, dy, dz, rz = [F(v) for v in box]
        z_ok = ~(np.abs((z - cz).astype(F)).astype(np.float64) > np.float64(dz) / 2.0)
        cosa, sina = np.cos(F(-rz), dtype=F), np.sin(F(-rz), dtype=F)
        sx, sy = (x - cx).astype(F), (y - cy).astype(F)
        lx = ((sx * cosa).astype(F) + (sy * F(-sina)).astype(F)).astype(F)
        ly = ((sx * sina).astype(F) + (sy * cosa).astype(F)).astype(F)
        out[m] = z_ok & (np.abs(lx).astype(np.float64) < np.float64(dx) / 2.0 + margin) & (np.abs(ly).astype(np.float64) < np.float64(dy) / 2.0 + margin)
    return out


def local64(boxes, pts):
    """float64 box-frame coordinates (M, N, 3) of pts (N, 3) for boxes (M, 7), from the values as given."""
    b, p = np.asarray(boxes, np.float64).reshape(-1, 7), np.asarray(pts, np.float64).reshape(-1, 3)
    s = p[None, :, :] - b[:, None, :3]
    c, sn = np.cos(-b[:, 6])[:, None], np.sin(-b[:, 6])[:, None]
    return np.stack([s[..., 0] * c - s[..., 1] * sn, s[..., 0] * sn + s[..., 1] * c, s[..., 2]], -1)


def inside_f64(boxes, pts):
    """(M, N) bool: the same test in float64 throughout."""
    b = np.asarray(boxes, np.float64).reshape(-1, 7)
    loc = np.abs(local64(boxes, pts))
    return (loc[..., 2] <= b[:, None, 5] / 2) & (loc[..., 0] < b[:, None, 3] / 2 + 1e-5) & (loc[..., 1] < b[:, None, 4] / 2 + 1e-5)


def lists(xyz, boxes, n_sampled):
    """(idx (B, M, S) int64 with padding applied (-1 in an empty box), cnt (B, M) the list lengths after the cut)."""
    xyz, boxes = np.asarray(xyz, F), np.asarray(boxes, F)
    B, M = boxes.shape[0], boxes.shape[1]
    idx = np.full((B, M, n_sampled), -1, np.int64)
    cnt = np.zeros((B, M), np.int64)
    for b in range(B):
        ins = inside_fp32(boxes[b], xyz[b]) if xyz.shape[1] else np.zeros((M, 0), bool)
        for m in range(M):
            rows = np.flatnonzero(ins[m])[:n_sampled]
            cnt[b, m] = len(rows)
            if len(rows):
                idx[b, m] = rows[np.arange(n_sampled) % len(rows)]
    return idx, cnt


def pool(xyz, feat, boxes, n_sampled, canonical=False):
    """canonical False: (pooled (B, M, S, 3 + C) fp32, flag (B, M) int32).
    canonical True: (pooled float64 -- x, y the float64 box-frame values, z and the features the exact fp32 values --, flag, bound (B, M, S))."""
    xyz, feat, boxes = np.asarray(xyz, F), np.asarray(feat, F), np.asarray(boxes, F)
    B, M, C = boxes.shape[0], boxes.shape[1], feat.shape[2]
    idx, cnt = lists(xyz, boxes, n_sampled)
    flag = (cnt == 0).astype(np.int32)
    pooled = np.zeros((B, M, n_sampled, 3 + C), np.float64 if canonical else F)
    bound = np.zeros((B, M, n_sampled), np.float64)
    for b in range(B):
        for m in range(M):
            if cnt[b, m] == 0:
                continue
            rows = idx[b, m]
            pooled[b, m, :, 3:] = feat[b, rows]
            if not canonical:
                pooled[b, m, :, :3] = xyz[b, rows]
                continue
            loc = local64(boxes[b, m], xyz[b, rows])[0]
            pooled[b, m, :, 0:2] = loc[:, 0:2]
            pooled[b, m, :, 2] = (xyz[b, rows, 2] - boxes[b, m, 2]).astype(F)
            s = xyz[b, rows, 0:2].astype(np.float64) - boxes[b, m, 0:2].astype(np.float64)
            bound[b, m] = 8.0 * 2.0 ** -24 * np.abs(s).sum(-1)
    return (pooled, flag, bound) if canonical else (pooled, flag)
