"""TEST INFRASTRUCTURE: a numpy restatement of PV-RCNN++'s vector-pool operations, written from the statements of the operations and not from the
kernels under test.  Every fp32 operation is rounded where the statement rounds it.

  in range      local = fp32(p - q) per axis; a row is REJECTED when any |local| > R (cube) or, neighbor_type == 1,
                fp32(fp32(fp32(lx * lx) + fp32(ly * ly)) + fp32(lz * lz)) > fp32(R * R) (ball); otherwise it is in range
  cell          per axis i = floor(fp32(fp32(local + R) / gs)), gs = fp32(fp32(R * 2) / n); combined ix * ny * nz + iy * nz + iz, THEN clamped to
                [0, G - 1] (so local == +R aliases into a neighbouring cell or the last one)
  choice        walk the query's scene in ascending row order; an in-range row whose cell is still empty is taken; stop once nsample (> 0) rows or
                G rows are taken.  choice = global row or -1, cnt in {0, 1}, local xyz of the taken row, features[row][c_in - c_each + j]
  choice grad   for every c < c_in: grad_support[choice[m][g]][c] += fp32(grad_new[m][g * c_each + c % c_each] * fp32(1 / max(cnt, 1)))
  list          the first min(1000, nsample if nsample > 0) in-range rows of the query's scene, ascending (distance R given as fp32)
  three_nn      per grid centre the three list entries smallest under (d, position in list), d = fp32 (cx-x)^2 + (cy-y)^2 + (cz-z)^2 summed left
                to right; 1 found: slots 2, 3 repeat slot 1; 2 found: slot 3 repeats slot 1; none: idx -1, dist2 +inf
  interpolate   out = fp32(fp32(fp32(w0 * f0) + fp32(w1 * f1)) + fp32(w2 * f2)); an index outside [0, n) gives the term +0.0f
  ordered sums  start at +0.0f, keys ascending, every addition rounded to fp32
"""
import numpy as np

F = np.float32
LIST_CAP = 1000


def scene_ranges(counts):
    counts = np.asarray(counts, np.int64)
    starts = np.cumsum(counts) - counts
    return [(int(s), int(c)) for s, c in zip(starts, counts)]


def local_xyz(p, q):
    return (np.asarray(p, F) - np.asarray(q, F)).astype(F)


def in_range(local, R, neighbor_type):
    """(n,) bool for local (n, 3) fp32."""
    R = F(R)
    lx, ly, lz = local[:, 0], local[:, 1], local[:, 2]
    if neighbor_type == 1:
        d = (((lx * lx).astype(F) + (ly * ly).astype(F)).astype(F) + (lz * lz).astype(F)).astype(F)
        return ~(d > F(R * R))
    return ~((np.abs(lx) > R) | (np.abs(ly) > R) | (np.abs(lz) > R))


def cell_index(local, R, grid):
    """(n,) int64 combined-then-clamped cell of in-range local (n, 3)."""
    R = F(R)
    nx, ny, nz = (int(v) for v in grid)
    G = nx * ny * nz
    i = []
    for a, n in enumerate((nx, ny, nz)):
        gs = F(F(R * F(2)) / F(n))
        i.append(np.floor(((local[:, a] + R).astype(F) / gs).astype(F)).astype(np.int64))
    return np.clip(i[0] * ny * nz + i[1] * nz + i[2], 0, G - 1)


def choice(xyz, xyz_cnt, feats, new_xyz, new_cnt, grid, R, nsample, neighbor_type, c_each):
    """-> choice (M, G) int32, cnt (M, G) int32, new_local_xyz (M, 3 G) fp32, new_features (M, G * c_each) fp32"""
    xyz, feats, new_xyz = np.asarray(xyz, F).reshape(-1, 3), np.asarray(feats, F), np.asarray(new_xyz, F).reshape(-1, 3)
    G = int(grid[0]) * int(grid[1]) * int(grid[2])
    M, c_in = len(new_xyz), feats.shape[1]
    assert c_in % c_each == 0
    ch = np.full((M, G), -1, np.int32)
    loc = np.zeros((M, G, 3), F)
    nf = np.zeros((M, G, c_each), F)
    for (qs, qn), (ps, pn) in zip(scene_ranges(new_cnt), scene_ranges(xyz_cnt)):
        for m in range(qs, qs + qn):
            l = local_xyz(xyz[ps:ps + pn], new_xyz[m])
            ok = in_range(l, R, neighbor_type)
            cells = cell_index(l, R, grid)
            taken = 0
            for k in range(pn):
                if not ok[k] or ch[m, cells[k]] >= 0:
                    continue
                ch[m, cells[k]] = ps + k
                loc[m, cells[k]] = l[k]
                nf[m, cells[k]] = feats[ps + k, c_in - c_each:]
                taken += 1
                if (nsample > 0 and taken >= nsample) or taken >= G:
                    break
    return ch, (ch >= 0).astype(np.int32), loc.reshape(M, 3 * G), nf.reshape(M, G * c_each)


def choice_grad_terms(grad_new, ch, cnt, N, c_in, c_each, exact=False):
    """Per support row the fp32 terms in ascending key m * G + g: list of (n_terms, c_in) arrays.  exact: the unrounded float64 products."""
    grad_new = np.asarray(grad_new, F)
    T = np.float64 if exact else F
    M, G = ch.shape
    cols = np.arange(c_in) % c_each
    terms = [[] for _ in range(N)]
    for key in range(M * G):
        m, g = divmod(key, G)
        row = int(ch[m, g])
        if row < 0 or row >= N:
            continue
        scale = F(F(1) / np.maximum(F(cnt[m, g]), F(1)))
        terms[row].append((grad_new[m, g * c_each + cols].astype(T) * T(scale)).astype(T))
    return [np.stack(t) if t else np.zeros((0, c_in), T) for t in terms]


def ordered_sum(terms, width):
    """(N, width) fp32: per row +0.0f + its terms in the given order, every addition rounded."""
    out = np.zeros((len(terms), width), F)
    for n, t in enumerate(terms):
        a = np.zeros(width, F)
        for row in t:
            a = (a + row).astype(F)
        out[n] = a
    return out


def sum_f64_and_bound(terms, width):
    """terms: the EXACT float64 products per row.  -> (N, width) float64 sums and the bound that an fp32 sum of the rounded products keeps in ANY
    order: K additions, each within 2^-24 (relative) of a partial sum that never exceeds sum|term| (1 + 2^-24)^K -> K * 2^-24 * sum|term|; one
    rounding per product -> 2^-24 * sum|term|; the factor 1.001 covers the second-order terms (K < 2^13)."""
    ref, bound = np.zeros((len(terms), width)), np.zeros((len(terms), width))
    for n, t in enumerate(terms):
        if len(t):
            t64 = np.asarray(t, np.float64)
            mag = np.abs(t64).sum(0)
            ref[n], bound[n] = t64.sum(0), 1.001 * (len(t) + 1) * 2.0 ** -24 * mag
    return ref, bound


def neighbour_list(xyz_scene, q, R, nsample, neighbor_type):
    """scene-local rows of the query's list."""
    ok = in_range(local_xyz(xyz_scene, q), R, neighbor_type)
    cap = min(LIST_CAP, nsample) if nsample > 0 else LIST_CAP
    return np.flatnonzero(ok)[:cap]


def three_nn_of_list(xyz, rows, centers_m):
    """xyz (N, 3) fp32, rows: the list as GLOBAL rows in list order, centers_m (G, 3) -> idx (G, 3) int32, dist2 (G, 3) fp32"""
    G = len(centers_m)
    idx, d2 = np.full((G, 3), -1, np.int32), np.full((G, 3), np.inf, F)
    rows = np.asarray(rows, np.int64)
    if not len(rows):
        return idx, d2
    p = xyz[rows]
    for g in range(G):
        c = centers_m[g]
        dx, dy, dz = (c[0] - p[:, 0]).astype(F), (c[1] - p[:, 1]).astype(F), (c[2] - p[:, 2]).astype(F)
        d = (((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)
        order = np.lexsort((np.arange(len(rows)), d))[:3]              # key (d, position in list)
        sel = [order[0], order[1] if len(order) > 1 else order[0], order[2] if len(order) > 2 else order[0]]
        idx[g], d2[g] = rows[sel], d[sel]
    return idx, d2


def three_nn(xyz, xyz_cnt, new_xyz, centers, new_cnt, R, nsample, neighbor_type):
    """R: the query distance as the fp32 value the caller passes.  -> idx (M, G, 3) int32 global rows, dist2 (M, G, 3) fp32"""
    xyz, new_xyz, centers = np.asarray(xyz, F).reshape(-1, 3), np.asarray(new_xyz, F).reshape(-1, 3), np.asarray(centers, F)
    M, G = centers.shape[0], centers.shape[1]
    idx = np.full((M, G, 3), -1, np.int32)
    d2 = np.full((M, G, 3), np.inf, F)
    for (qs, qn), (ps, pn) in zip(scene_ranges(new_cnt), scene_ranges(xyz_cnt)):
        for m in range(qs, qs + qn):
            rows = neighbour_list(xyz[ps:ps + pn], new_xyz[m], R, nsample, neighbor_type)
            idx[m], d2[m] = three_nn_of_list(xyz, ps + rows, centers[m])
    return idx, d2


def _valid(idx, n):
    return (idx >= 0) & (idx < n)


def interpolate(feats, idx, weight):
    feats, weight = np.asarray(feats, F), np.asarray(weight, F)
    n = len(feats)
    t = []
    for s in range(3):
        ok = _valid(idx[:, s], n)
        f = feats[np.where(ok, idx[:, s], 0)] if n else np.zeros((len(idx), feats.shape[1]), F)
        t.append(np.where(ok[:, None], (weight[:, s:s + 1] * f).astype(F), F(0)).astype(F))
    return ((t[0] + t[1]).astype(F) + t[2]).astype(F)


def interpolate_grad_terms(grad_out, idx, weight, n, exact=False):
    """Per feature row the fp32 terms fp32(grad_out[r] * w[r][t]) in ascending key 3 r + t.  exact: the unrounded float64 products."""
    T = np.float64 if exact else F
    grad_out, weight = np.asarray(grad_out, F).astype(T), np.asarray(weight, F).astype(T)
    terms = [[] for _ in range(n)]
    for r in range(len(idx)):
        for s in range(3):
            i = int(idx[r, s])
            if 0 <= i < n:
                terms[i].append((grad_out[r] * weight[r, s]).astype(T))
    C = grad_out.shape[1]
    return [np.stack(t) if t else np.zeros((0, C), T) for t in terms]
