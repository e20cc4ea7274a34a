"""The stated order of the dense-batch order-fixed gradients (include/seevcn_hip.h: sv_group_points_grad_batch_ordered,
sv_gather_points_grad_batch_ordered, sv_three_interpolate_grad_batch_ordered) as plain numpy loops over ascending keys, np.float32 adds and -- for
the interpolation -- np.float32 products, and the cases the tests run them on.  Every reference returns, per element, the fp32 result of the
stated order, the float64 sum of the float64 terms, the float64 sum of |terms| and the term count T; an index outside its range names nothing."""
import functools

import numpy as np

F = np.float32


def group_grad(grad_out, idx, n):
    """grad_out (B, c, per), idx (B, per) -> fp32 (B, c, n), float64 sum (B, c, n), float64 sum |t| (B, c, n), T (B, n)"""
    B, c, per = grad_out.shape
    out, exact, mag, cnt = np.zeros((B, c, n), F), np.zeros((B, c, n)), np.zeros((B, c, n)), np.zeros((B, n))
    g64 = grad_out.astype(np.float64)
    for b in range(B):
        for j in range(per):                                                     # ascending key
            i = int(idx[b, j])
            if i < 0 or i >= n:
                continue
            out[b, :, i] = out[b, :, i] + grad_out[b, :, j]                      # fp32 + fp32, rounded to fp32
            exact[b, :, i] += g64[b, :, j]
            mag[b, :, i] += np.abs(g64[b, :, j])
            cnt[b, i] += 1
    assert out.dtype == F
    return out, exact, mag, cnt


def interpolate_grad(grad_out, idx, weight, m):
    """grad_out (B, c, n), idx / weight (B, n, 3) -> fp32 (B, c, m), float64 sum, float64 sum |t|, T (B, m); key 3 p + t"""
    B, c, n = grad_out.shape
    out, exact, mag, cnt = np.zeros((B, c, m), F), np.zeros((B, c, m)), np.zeros((B, c, m)), np.zeros((B, m))
    g64, w64 = grad_out.astype(np.float64), weight.astype(np.float64)
    for b in range(B):
        for p in range(n):
            for t in range(3):
                i = int(idx[b, p, t])
                if i < 0 or i >= m:
                    continue
                term = grad_out[b, :, p] * weight[b, p, t]                       # the product is rounded to fp32 before it is added
                assert term.dtype == F
                out[b, :, i] = out[b, :, i] + term
                t64 = g64[b, :, p] * w64[b, p, t]
                exact[b, :, i] += t64
                mag[b, :, i] += np.abs(t64)
                cnt[b, i] += 1
    return out, exact, mag, cnt


# ------------------------------------------------------------------------------------------------ cases
def _balls(rng, allowed, n_queries, nsample):
    """(n_queries, nsample) indices as ball_query writes them: the hits ascending, the rest repeats of the first hit"""
    idx = np.empty((n_queries, nsample), np.int32)
    for q in range(n_queries):
        hits = np.sort(rng.choice(allowed, size=int(rng.integers(1, min(nsample, len(allowed)) + 1)), replace=False))
        idx[q] = hits[0]
        idx[q, :len(hits)] = hits
    return idx


BALLS = dict(B=3, N=70, npoint=9, nsample=16)
BALLS_HOT, BALLS_UNUSED = 11, (3, 64)               # the row five single-hit queries of every scene point at; rows no query may name
BALLS_CHANNELS = [1, 5, 35]
TILE = dict(B=2, N=257, npoint=33, nsample=32, C=3)
GATHER = dict(B=2, N=64, npoint=40, C=6)
INTERP_B, INTERP_N = 2, 300
INTERP_CHANNELS, INTERP_M = [1, 7, 65], [2, 5, 257]


@functools.lru_cache(maxsize=None)
def balls_case(C):
    """-> grad_out (B, C, npoint * nsample), idx (B, npoint * nsample)"""
    B, N, npoint, nsample = (BALLS[k] for k in ("B", "N", "npoint", "nsample"))
    rng = np.random.default_rng(300 + C)
    allowed = np.array([r for r in range(N) if r not in BALLS_UNUSED])
    idx = np.stack([_balls(rng, allowed, npoint, nsample) for _ in range(B)])
    idx[:, 1:6] = BALLS_HOT                                                       # five single-hit queries: 5 * 16 = 80 slots on one row
    idx = idx.reshape(B, npoint * nsample)
    counts = np.stack([np.bincount(idx[b], minlength=N) for b in range(B)])
    assert (counts[:, BALLS_HOT] >= 80).all(), "a row with more keys than a wave has lanes"
    assert (counts[:, list(BALLS_UNUSED)] == 0).all() and (counts == 0).sum() >= 2 * B, "rows that nothing names"
    return rng.normal(0, 1, (B, C, npoint * nsample)).astype(F), idx


@functools.lru_cache(maxsize=None)
def tile_case():
    B, N, npoint, nsample, C = (TILE[k] for k in ("B", "N", "npoint", "nsample", "C"))
    rng = np.random.default_rng(310)
    idx = np.stack([_balls(rng, np.arange(N), npoint, nsample) for _ in range(B)])
    idx[:, 0] = N - 1                                                             # the row behind the first 256-thread tile
    idx = idx.reshape(B, npoint * nsample)
    assert N > 256 and (npoint * nsample) % 256 != 0 and (idx == N - 1).any(axis=1).all()
    return rng.normal(0, 1, (B, C, npoint * nsample)).astype(F), idx


@functools.lru_cache(maxsize=None)
def gather_case():
    B, N, npoint, C = (GATHER[k] for k in ("B", "N", "npoint", "C"))
    rng = np.random.default_rng(320)
    idx = rng.integers(0, N, (B, npoint)).astype(np.int32)
    idx[:, 7] = idx[:, 2]
    idx[:, 31] = idx[:, 2]
    assert all(len(np.unique(idx[b])) < npoint for b in range(B)), "repeated indices"
    return rng.normal(0, 1, (B, C, npoint)).astype(F), idx


@functools.lru_cache(maxsize=None)
def interp_case(c, m):
    """-> grad_out (B, c, n), idx (B, n, 3): the three nearest of m known points (fewer than three: slot 0's default, row 0), weight (B, n, 3),
    and the (b, row) whose sum is +0.0 + -0.0"""
    B, n = INTERP_B, INTERP_N
    rng = np.random.default_rng(400 + 10 * c + m)
    unknown, known = rng.uniform(-0.5, 0.5, (B, n, 3)), rng.uniform(-1, 1, (B, m, 3))      # the outer known points are nobody's neighbours
    d2 = ((unknown[:, :, None] - known[:, None]) ** 2).sum(-1)
    order = np.argsort(d2, axis=-1, kind="stable")[..., :3]
    idx = np.zeros((B, n, 3), np.int32)
    idx[..., :order.shape[-1]] = order
    weight = rng.uniform(0.05, 1, (B, n, 3))
    weight = (weight / weight.sum(-1, keepdims=True)).astype(F)                   # full-mantissa fp32
    grad_out = rng.normal(0, 1, (B, c, n)).astype(F)
    counts = np.bincount(idx[0].ravel(), minlength=m)
    if m == 2:
        assert (idx[..., 2] == 0).all() and (idx[..., :2] == 0).any(-1).all(), "two slots of one p name row 0"
    if m == 5:
        assert counts.max() >= 150
    if m == 257:
        assert (counts == 0).sum() >= 20
    # -1.5 * +0.0 = -0.0 enters a row whose other terms are zero; +0.0 + -0.0 = +0.0: the expected sign is plus
    named = np.nonzero(counts)[0]
    row = int(named[np.argmin(counts[named])])
    hit = idx[0] == row
    weight[0][hit] = 0.0
    grad_out[0, :, np.nonzero(hit.any(-1))[0][0]] = -1.5
    return grad_out, idx, weight, (0, row)


@functools.lru_cache(maxsize=None)
def balls_ref(C):
    return group_grad(*balls_case(C), BALLS["N"])


@functools.lru_cache(maxsize=None)
def tile_ref():
    return group_grad(*tile_case(), TILE["N"])


@functools.lru_cache(maxsize=None)
def gather_ref():
    return group_grad(*gather_case(), GATHER["N"])


@functools.lru_cache(maxsize=None)
def interp_ref(c, m):
    grad_out, idx, weight, _ = interp_case(c, m)
    return interpolate_grad(grad_out, idx, weight, m)


def with_strays(idx, rows):
    """A copy of idx (B, ...) with a -1 and an index equal to `rows` placed once in batch element 0 and once in the last one.  Unguarded,
    b * rows + idx would make them the neighbouring batch element's last and first row.  ORDERED ENTRIES ONLY: a plain entry writes there."""
    idx = idx.copy()
    flat = idx.reshape(idx.shape[0], -1)
    flat[0, 5], flat[0, 17] = -1, rows
    flat[-1, 3], flat[-1, 29] = rows, -1
    return idx
