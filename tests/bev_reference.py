"""numpy references for the channel-last BEV interpolation gradient (sv_bev_interpolate_grad_nhwc) and the keypoint sets its tests use.

The entry defines its result: for each pixel start from +0.0f and add grad_out[m, c] * w_t in ascending key 4 * m + t (t = 0..3: the taps wa, wb, wc,
wd of bev_taps in csrc/head.hip), every product and every sum rounded to fp32.  `grad_sequential_f32` is that definition in numpy float32;
`grad_f64` is the exact sum of the same fp32-weighted terms in float64 with the per-pixel term count and sum of magnitudes that bound fp32 error.

With x_min = y_min = 0, voxel 0.5 and stride 8 (DYADIC) every division in bev_taps is by a power of two, hence exact; the subtractions and products
are single correctly rounded fp32 operations on both sides, so `taps` gives the kernel's weights bit for bit."""
from collections import namedtuple

import numpy as np

Geom = namedtuple("Geom", "x_min y_min voxel_x voxel_y stride")
DYADIC = Geom(0.0, 0.0, 0.5, 0.5, 8.0)
KITTI = Geom(0.0, -40.0, 0.05, 0.05, 8.0)
F32 = np.float32


def taps(kps, geom, B, H, W):
    """bev_taps for every row of kps (M, 4) [b, x, y, z] in float32.  Returns valid (M,) bool, pix (M, 4) int64 pixel index (b * H + y) * W + x of
    the taps in key order (y0x0, y1x0, y0x1, y1x1), w (M, 4) float32."""
    kps = np.asarray(kps, F32).reshape(-1, 4)
    b = np.trunc(kps[:, 0]).astype(np.int64)
    x = ((kps[:, 1] - F32(geom.x_min)) / F32(geom.voxel_x)) / F32(geom.stride)
    y = ((kps[:, 2] - F32(geom.y_min)) / F32(geom.voxel_y)) / F32(geom.stride)
    assert x.dtype == F32 and y.dtype == F32
    fx0, fy0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x0, x1 = np.clip(fx0, 0, W - 1), np.clip(fx0 + 1, 0, W - 1)
    y0, y1 = np.clip(fy0, 0, H - 1), np.clip(fy0 + 1, 0, H - 1)
    fx0_, fx1_, fy0_, fy1_ = x0.astype(F32), x1.astype(F32), y0.astype(F32), y1.astype(F32)
    w = np.stack([(fx1_ - x) * (fy1_ - y), (fx1_ - x) * (y - fy0_), (x - fx0_) * (fy1_ - y), (x - fx0_) * (y - fy0_)], axis=1)
    assert w.dtype == F32
    valid = (b >= 0) & (b < B)
    base = np.where(valid, b, 0) * H * W
    pix = np.stack([base + y0 * W + x0, base + y1 * W + x0, base + y0 * W + x1, base + y1 * W + x1], axis=1)
    return valid, pix, w


def tap_terms(kps, geom, B, H, W, drop_key=None):
    """The terms of the gradient sum in ascending key order: keys (T,), pixel (T,), weight (T,) float32.  drop_key leaves one term out (for the
    checker's self-test)."""
    valid, pix, w = taps(kps, geom, B, H, W)
    M = valid.shape[0]
    keys = (4 * np.arange(M, dtype=np.int64)[:, None] + np.arange(4)[None, :])
    keep = np.repeat(valid[:, None], 4, axis=1)
    if drop_key is not None:
        keep = keep & (keys != drop_key)
    keys, pix, w = keys[keep], pix[keep], w[keep]                     # row-major boolean selection keeps ascending key order
    assert np.all(np.diff(keys) > 0), "keys must be unique and ascending"
    assert np.all(np.isfinite(w)), "tap weights must be finite"
    return keys, pix, w


def grad_sequential_f32(kps, grad_out, geom, B, C, H, W, reverse=False, drop_key=None):
    """The defined result, (B, H, W, C) float32.  reverse=True sums in DESCENDING key order (a wrong order, for the checker's self-test)."""
    grad_out = np.asarray(grad_out, F32).reshape(-1, C)
    keys, pix, w = tap_terms(kps, geom, B, H, W, drop_key)
    out = np.zeros((B * H * W, C), F32)
    order = range(len(keys) - 1, -1, -1) if reverse else range(len(keys))
    for i in order:
        prod = grad_out[keys[i] >> 2] * w[i]                          # float32 * float32 -> one rounding
        out[pix[i]] = out[pix[i]] + prod                              # one rounding
    assert out.dtype == F32
    return out.reshape(B, H, W, C)


def grad_f64(kps, grad_out, geom, B, C, H, W):
    """(exact, bound): the float64 sum of the fp32-weighted terms, (B, H, W, C), and the element-wise bound (n + 1) * 2^-24 * sum |grad_out * w| for
    an fp32 evaluation in ANY order: one rounding per product, n - 1 per sum (n = the pixel's number of terms; no terms -> bound 0)."""
    grad_out = np.asarray(grad_out, F32).reshape(-1, C)
    keys, pix, w = tap_terms(kps, geom, B, H, W)
    terms = grad_out[keys >> 2].astype(np.float64) * w.astype(np.float64)[:, None]
    exact = np.zeros((B * H * W, C), np.float64)
    mag = np.zeros((B * H * W, C), np.float64)
    np.add.at(exact, pix, terms)
    np.add.at(mag, pix, np.abs(terms))
    n = np.bincount(pix, minlength=B * H * W).astype(np.float64)
    bound = (n[:, None] + 1.0) * 2.0 ** -24 * mag
    return exact.reshape(B, H, W, C), bound.reshape(B, H, W, C)


def assert_bit_equal(got, want, name="gradient"):
    """Bitwise equality of two float32 arrays, the sign of zero included."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    if diff.any():
        i = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.size} elements differ in their bits, first at {i}: {got[i]!r} ({got.view(np.uint32)[i]:#010x}) "
                             f"!= {want[i]!r} ({want.view(np.uint32)[i]:#010x})")


def assert_within_bound(got, exact, bound, name="gradient"):
    """|got - exact| <= bound for EVERY element (a pixel without terms has bound 0: it must be exactly zero)."""
    err = np.abs(np.asarray(got, np.float64) - exact)
    bad = ~(err <= bound)                                             # also catches nan
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {i}: got {got[i]!r}, exact {exact[i]!r}, "
                             f"error {err[i]:.3e} > bound {bound[i]:.3e}; worst error / bound {np.nanmax(err / np.maximum(bound, 1e-300)):.3f}")


# ---------------------------------------------------------------------------------------------------------------- inputs
def order_sensitive_case():
    """Three keypoints on the same integer cell coordinate (weight exactly 1 on one pixel) with gradients 1, 2^-24, 2^-24: ascending order gives 1.0
    (each small term is half an ulp of 1 and rounds to even), descending order gives 1 + 2^-23."""
    kps = np.array([[0, 8.0, 4.0, 0.0]] * 3, F32)                     # DYADIC: cell (x 2, y 1)
    grad_out = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], F32)
    return kps, grad_out


def _xy(u, v, geom):
    """cell coordinates -> metres (float32)"""
    cx, cy = geom.voxel_x * geom.stride, geom.voxel_y * geom.stride
    return (geom.x_min + np.asarray(u, np.float64) * cx).astype(F32), (geom.y_min + np.asarray(v, np.float64) * cy).astype(F32)


def make_keypoints(kind, B, H, W, geom, seed=0):
    """(M, 4) float32 [b, x, y, z].
    'empty': M = 0.  'one': M = 1, inside.  'mixed': M = 1000 -- 500 inside, 200 outside the map on every side and corner (clamped corners), 200 exactly
    on integer cell coordinates (the last row / column and one past it included), 50 rows with batch index -1 and 50 with B, shuffled.
    'cluster': 300 keypoints inside ONE cell (key lists of 300) plus 20 spread ones."""
    rng = np.random.RandomState(seed)
    if kind == "empty":
        return np.zeros((0, 4), F32)
    if kind == "one":
        u, v, b = rng.uniform(0, W - 1, 1), rng.uniform(0, H - 1, 1), rng.randint(0, B, 1)
    elif kind == "mixed":
        ui, vi = rng.uniform(-0.5, W - 0.5, 500), rng.uniform(-0.5, H - 0.5, 500)
        side = rng.randint(0, 8, 200)                                 # 0..3 the sides, 4..7 the corners
        far = rng.uniform(0.1, 2.5, (200, 2))
        uo, vo = rng.uniform(0, W - 1, 200), rng.uniform(0, H - 1, 200)
        left, right = np.isin(side, (0, 4, 5)), np.isin(side, (1, 6, 7))
        low, high = np.isin(side, (2, 4, 6)), np.isin(side, (3, 5, 7))
        uo = np.where(left, -far[:, 0], np.where(right, W - 1 + far[:, 0], uo))
        vo = np.where(low, -far[:, 1], np.where(high, H - 1 + far[:, 1], vo))
        ug, vg = rng.randint(0, W + 1, 200).astype(np.float64), rng.randint(0, H + 1, 200).astype(np.float64)
        ug[:4], vg[:4] = (0, W - 1, W, W - 1), (0, H - 1, H - 1, H)
        ub, vb = rng.uniform(0, W - 1, 100), rng.uniform(0, H - 1, 100)
        u, v = np.concatenate([ui, uo, ug, ub]), np.concatenate([vi, vo, vg, vb])
        b = np.concatenate([rng.randint(0, B, 900), np.full(50, -1), np.full(50, B)])
        perm = rng.permutation(1000)
        u, v, b = u[perm], v[perm], b[perm]
    elif kind == "cluster":
        cu, cv = W // 2, H // 2
        u = np.concatenate([cu + rng.uniform(0.01, 0.99, 300), rng.uniform(0, W - 1, 20)])
        v = np.concatenate([cv + rng.uniform(0.01, 0.99, 300), rng.uniform(0, H - 1, 20)])
        b = np.concatenate([np.full(300, B - 1), rng.randint(0, B, 20)])
        perm = rng.permutation(320)
        u, v, b = u[perm], v[perm], b[perm]
    else:
        raise ValueError(kind)
    x, y = _xy(u, v, geom)
    return np.stack([b.astype(F32), x, y, rng.uniform(-1, 1, len(x)).astype(F32)], axis=1)
