"""TEST INFRASTRUCTURE: a numpy restatement of RoI-aware point feature pooling (Part-A2), written from the statements of the operation and not
from the kernels under test.

  in-box test   |z - cz| (fp32) > dz / 2 (double) -> outside; local x/y = the shift rotated by cos/sin(-rz) in fp32, every product and sum
                rounded; inside iff |lx| < dx / 2 + 1e-5 and |ly| < dy / 2 + 1e-5 (double compare, 1e-5 the fp32 constant); no margin on z
  cell          x_res = dx / out_x (fp32); x_idx = int((lx + dx / 2) / x_res) clamped to [0, out_x - 1]; the same for y and z (lz = z - cz)
  lists         (N, out_x, out_y, out_z, cap) int32: slot 0 the count, slots 1..count the point rows ascending, at most cap - 1 kept, the
                later ones dropped; slots behind the count are unspecified (here: -7)
  max           strict > in list order from -inf: the first row of the largest value wins; argmax -1 and value 0 for an empty cell
  avg           the sum in list order over the count; 0 for an empty cell
  backward      max: grad_in[argmax] += grad_out; avg: grad_in[p] += grad_out / max(count, 1) for each listed p        (float64)
"""
import numpy as np

F = np.float32
UNSET = -7


def cells_of_points(box, pts, out_size):
    """(inside (M,) bool, cell (M, 3) int64 [x_idx, y_idx, z_idx]) of pts (M, 3) fp32 for one box (7,) fp32."""
    box, pts = np.asarray(box, F), np.asarray(pts, F).reshape(-1, 3)
    cx, cy, cz, dx, dy, dz, rz = [F(v) for v in box]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    z_ok = ~(np.abs(z - cz).astype(np.float64) > np.float64(dz) / 2.0)
    cosa, sina = np.cos(F(-rz), dtype=F), np.sin(F(-rz), dtype=F)
    sx, sy = (x - cx).astype(F), (y - cy).astype(F)
    lx = ((sx * cosa).astype(F) + (sy * F(-sina)).astype(F)).astype(F)
    ly = ((sx * sina).astype(F) + (sy * cosa).astype(F)).astype(F)
    margin = np.float64(F(1e-5))
    inside = z_ok & (np.abs(lx).astype(np.float64) < np.float64(dx) / 2.0 + margin) & (np.abs(ly).astype(np.float64) < np.float64(dy) / 2.0 + margin)
    lz = (z - cz).astype(F)
    idx = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for local, d, n in ((lx, dx, out_size[0]), (ly, dy, out_size[1]), (lz, dz, out_size[2])):
            res = F(d / F(n))
            q = ((local + F(d / F(2))).astype(F) / res).astype(F)
            q = np.where(np.isfinite(q), q, 0)
            idx.append(np.clip(np.trunc(q).astype(np.int64), 0, n - 1))
    return inside, np.stack(idx, 1)


def assign(rois, pts, out_size, cap, box_pt_range=None):
    """pts_idx_of_voxels (N, ox, oy, oz, cap) int32; box_pt_range (N, 2): box b looks at rows [lo, hi) only, the stored rows are absolute."""
    rois, pts = np.asarray(rois, F).reshape(-1, 7), np.asarray(pts, F).reshape(-1, 3)
    ox, oy, oz = out_size
    lists = np.full((len(rois), ox, oy, oz, cap), UNSET, np.int32)
    lists[..., 0] = 0
    for b, box in enumerate(rois):
        lo, hi = (0, len(pts)) if box_pt_range is None else (max(int(box_pt_range[b][0]), 0), min(int(box_pt_range[b][1]), len(pts)))
        if hi <= lo:
            continue
        inside, cell = cells_of_points(box, pts[lo:hi], out_size)
        for k in np.flatnonzero(inside):                            # ascending point index
            c = lists[b, cell[k, 0], cell[k, 1], cell[k, 2]]
            if c[0] < cap - 1:
                c[c[0] + 1] = lo + k
                c[0] += 1
    return lists


def pool(lists, feat, method):
    """(pooled (N, ox, oy, oz, C) float64 -- max: the winning fp32 value itself; avg: the float64 mean --, argmax int32 or None)."""
    feat = np.asarray(feat, F)
    C = feat.shape[1]
    flat = lists.reshape(-1, lists.shape[-1])
    pooled = np.zeros((len(flat), C), np.float64)
    argmax = np.full((len(flat), C), -1, np.int32) if method == "max" else None
    for i, c in enumerate(flat):
        rows = c[1:1 + c[0]]
        if len(rows) == 0:
            continue
        if method == "max":
            best = np.full(C, -np.inf)
            for p in rows:
                gt = feat[p] > best
                best[gt] = feat[p][gt]
                argmax[i][gt] = p
            pooled[i] = np.where(argmax[i] >= 0, best, 0.0)
        else:
            pooled[i] = feat[rows].astype(np.float64).sum(0) / len(rows)
    shape = lists.shape[:-1] + (C,)
    return pooled.reshape(shape), (argmax.reshape(shape) if argmax is not None else None)


def pool_backward(lists, argmax, grad_out, n_pts, method):
    """grad_in (n_pts, C) float64."""
    g = np.asarray(grad_out, np.float64)
    C = g.shape[-1]
    g = g.reshape(-1, C)
    grad_in = np.zeros((n_pts, C), np.float64)
    if method == "max":
        a = argmax.reshape(-1, C)
        for c in range(C):
            ok = a[:, c] >= 0
            np.add.at(grad_in[:, c], a[ok, c], g[ok, c])
    else:
        flat = lists.reshape(-1, lists.shape[-1])
        for i, c in enumerate(flat):
            rows = c[1:1 + c[0]]
            if len(rows):
                np.add.at(grad_in, rows, g[i] / max(int(c[0]), 1))
    return grad_in


def lists_equal(got, want):
    """Counts, and slots 1..count; slots behind the count are not compared."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(got[..., 0], want[..., 0]):
        return False
    cap = want.shape[-1]
    live = np.arange(cap) <= want[..., :1]
    return bool(np.array_equal(np.where(live, got, 0), np.where(live, want, 0)))
