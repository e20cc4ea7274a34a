"""Host references for the focal image branch (csrc/focal_image.hip, spconv/focal.py; tests/test_focal_image_reference.py on the CPU,
tests/test_focal_image.py on the GPU): a numpy / torch-CPU restatement of FocalSparseConv.construct_multimodal_features
(focal_sparse_conv.py:50-113 with Calibration.lidar_to_img, calibration_kitti.py:65-93), the seeded cases, the pixel mask and the bounds.

Projection.  `project32` is the reference's arithmetic in float32 (numpy's np.dot for the two matrix products, as the reference).  `project64`
carries the same statements out in float64 on the same fp32 inputs and, beside every value, a bound of what ANY fp32 evaluation of that statement
may be off by.  Error model (u = 2^-24, as tests/voxel_edge_reference.py): +, -, *, / are off by at most half an ulp of the result, evaluated at
an upper bound of its magnitude; an inner product of n terms, in any order, with or without FMA, by at most gamma_n * sum|a_i b_i|,
gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5)); cosf / sinf by at most 4 ulp (the OpenCL
full-profile bound the device library is built to); operand errors pass through by the usual first-order rules with the second-order term
kept.  The matrix M = V2C^T R0^T is itself an fp32 inner product of 3 terms: its entries carry gamma_3 * sum|V2C_ki R0_jk|, so the bound
holds whichever BLAS formed it.

Pixel mask.  A voxel is masked when an integer lies within that bound of u or v (every decision the pixel depends on -- truncation, 0 <= u < W,
the (-1, 0) -> 0 rule -- flips at an integer), or when |rect_z| < RECT_Z_FLOOR: near the camera plane u = p0 / rect_z is arbitrarily steep.
Masked voxels are left out of PIXEL comparisons only, and every case keeps its masked share under MASK_CAP (asserted on the CPU).

Sampling.  `taps` states the four taps of F.interpolate(mode='bilinear', align_corners=False) at an integer pixel with the weights as the
kernel forms them (the source coordinate is the rational (in (2 d + 1) - out) / (2 out); the upper weight is the remainder over 2 out rounded
to fp32 once); `forward64` blends in float64 with the exact weights, `forward_interp64` goes through F.interpolate and indexing as the
reference does, `forward_bound` bounds an fp32 evaluation of the four products and three sums (plus the add of the sum mode), and
`grad_loop32` is the gradient as an fp32 loop in ascending key order."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as TF

F = np.float32
U = 2.0 ** -24
RANGE_ZYX = [-3.0, -40.0, 0.0]             # the layer's defaults (focal_sparse_conv.py:15-16), z-first
VOXEL_ZYX = [0.1, 0.05, 0.05]
GRID_ZYX = (41, 1600, 1408)
RECT_Z_FLOOR = 0.5                          # metres
MASK_CAP = 0.05
TRIG_ULPS = 4.0

# a KITTI training calibration (object benchmark, calib/000000.txt: P2, R0_rect, Tr_velo_to_cam), values as data
KITTI_P2 = [[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01], [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01], [0.0, 0.0, 1.0, 2.745884e-03]]
KITTI_R0 = [[9.999239e-01, 9.837760e-03, -7.445048e-03], [-9.869795e-03, 9.999421e-01, -4.278459e-03], [7.402527e-03, 4.351614e-03, 9.999631e-01]]
KITTI_V2C = [[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03], [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
             [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]]
KITTI_IMAGE = (375, 1242)


def make_calib(image_hw, scene):
    """The KITTI calibration with P2's first two rows scaled to an (H, W) image; scene > 0 shifts the principal point and the mount a little, so
    that two scenes of a batch do not share a table."""
    P2 = np.array(KITTI_P2, np.float64)
    P2[0] *= image_hw[1] / KITTI_IMAGE[1]
    P2[1] *= image_hw[0] / KITTI_IMAGE[0]
    V2C = np.array(KITTI_V2C, np.float64)
    P2[0, 2] += 0.37 * scene
    V2C[:, 3] += 0.011 * scene
    return SimpleNamespace(P2=P2.astype(F), R0=np.array(KITTI_R0, F), V2C=V2C.astype(F))


# name, image (H, W), features (h, w), C, rows per scene, the augmentation keys the batch carries
CASES = [
    dict(name="ratio", image=(47, 159), feat=(12, 40), C=16, rows=[1100, 900], cluster=True,
         aug=dict(noise_scale=[0.97, 1.04], noise_rot=[0.31, -0.52], flip_x=[True, False], flip_y=[False, True])),
    dict(name="tiny", image=(11, 13), feat=(3, 4), C=16, rows=[300, 0], cluster=False, aug={}),
    dict(name="equal3", image=(12, 40), feat=(12, 40), C=3, rows=[260, 240], cluster=False, aug=dict(noise_rot=[-0.2, 0.45], flip_x=[False, True])),
    dict(name="equal16", image=(12, 40), feat=(12, 40), C=16, rows=[250, 250], cluster=False, aug=dict(noise_scale=[1.05, 0.95], flip_y=[True, False])),
]
CASE_NAMES = [c["name"] for c in CASES]
POOL = 30000


# ------------------------------------------------------------------------------------------------------------ values with bounds
def half_ulp(mag):
    return 0.5 * np.spacing(np.abs(np.asarray(mag, np.float64)).astype(F)).astype(np.float64)


class V:
    """value (float64) and a bound of the error an fp32 evaluation may carry"""

    def __init__(self, val, err=0.0):
        self.val = np.asarray(val, np.float64)
        self.err = np.broadcast_to(np.asarray(err, np.float64), self.val.shape).copy()

    def _round(self, val, err):
        return V(val, err + half_ulp(np.abs(val) + err))

    def __add__(self, o):
        return self._round(self.val + o.val, self.err + o.err)

    def __mul__(self, o):
        return self._round(self.val * o.val, np.abs(self.val) * o.err + np.abs(o.val) * self.err + self.err * o.err)

    def __truediv__(self, o):
        lo = np.abs(o.val) - o.err
        lo = np.where(lo > 0, lo, np.nan)                       # a divisor that may be zero: no bound (such voxels are under the rect_z floor)
        q = self.val / o.val
        return self._round(q, (self.err + np.abs(q) * o.err) / lo)

    def __neg__(self):
        return V(-self.val, self.err)


def dot(terms):
    """inner product of n (V, V) pairs evaluated in fp32 in any order"""
    n = len(terms)
    gamma = n * U / (1 - n * U)
    val = sum(a.val * b.val for a, b in terms)
    mag = sum(np.abs(a.val) * np.abs(b.val) for a, b in terms)
    err = sum(np.abs(a.val) * b.err + np.abs(b.val) * a.err + a.err * b.err for a, b in terms)
    return V(val, err + gamma * (mag + err))


def calib_matrix(calib):
    """M = np.dot(V2C.T, R0.T) (4 x 3) in fp32, as lidar_to_rect and the packer form it, and the bound of its entries"""
    V2C, R0 = np.asarray(calib.V2C, F), np.asarray(calib.R0, F)
    M = np.dot(V2C.T, R0.T)
    mag = np.abs(V2C.T.astype(np.float64)) @ np.abs(R0.T.astype(np.float64))
    return M, (3 * U / (1 - 3 * U)) * mag


# ------------------------------------------------------------------------------------------------------------ projection
def _aug_values(case, b):
    aug = case["aug"]
    return (F(aug["noise_scale"][b]) if "noise_scale" in aug else None, F(aug["noise_rot"][b]) if "noise_rot" in aug else None,
            bool(aug["flip_x"][b]) if "flip_x" in aug else False, bool(aug["flip_y"][b]) if "flip_y" in aug else False)


def centres32(case, coords, stride=1):
    """(n, 3) fp32 [x, y, z]: the voxel positions with the world transforms taken back (:62-64, :82-90), every statement in fp32 -- the points
    lidar_to_img receives.  The rotation's sums run in ascending term order."""
    coords = np.asarray(coords)
    zyx = (coords[:, 1:].astype(np.int64) * stride).astype(F) * np.array(VOXEL_ZYX, F) + np.array(RANGE_ZYX, F)
    x, y, z = zyx[:, 2].copy(), zyx[:, 1].copy(), zyx[:, 0].copy()
    for b in range(len(case["rows"])):
        m = coords[:, 0] == b
        scale, rot, flip_x, flip_y = _aug_values(case, b)
        if scale is not None:
            x[m], y[m], z[m] = x[m] / scale, y[m] / scale, z[m] / scale
        if rot is not None:
            ang = -rot
            c, s = np.cos(ang, dtype=F), np.sin(ang, dtype=F)
            xr = (x[m] * c + y[m] * (-s)) + z[m] * F(0)
            yr = (x[m] * s + y[m] * c) + z[m] * F(0)
            x[m], y[m] = xr, yr
        if flip_x:
            y[m] = -y[m]
        if flip_y:
            x[m] = -x[m]
    return np.stack([x, y, z], axis=1).astype(F)


def project32(calibs, coords, centres):
    """(u, v, rect_z) in fp32 by the reference's statements: np.dot with M = np.dot(V2C.T, R0.T), np.dot with P2.T, division by rect z"""
    n = len(centres)
    u, v, rz = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    for b, calib in enumerate(calibs):
        m = coords[:, 0] == b
        hom = np.hstack((centres[m], np.ones((int(m.sum()), 1), F)))
        rect = np.dot(hom, np.dot(np.asarray(calib.V2C, F).T, np.asarray(calib.R0, F).T))
        rect_hom = np.hstack((rect, np.ones((len(rect), 1), F)))
        hom2d = np.dot(rect_hom, np.asarray(calib.P2, F).T)
        with np.errstate(divide="ignore", invalid="ignore"):
            img = (hom2d[:, 0:2].T / rect_hom[:, 2]).T
        u[m], v[m], rz[m] = img[:, 0], img[:, 1], rect[:, 2]
    return u, v, rz


def project64(case, calibs, coords, stride=1):
    """(u, v, rect_z, bound_u, bound_v): float64 values of the statements of centres32 + project32 and the bound an fp32 evaluation stays within"""
    coords = np.asarray(coords)
    n = len(coords)
    out = [np.full(n, np.nan) for _ in range(5)]
    vs, org = np.array(VOXEL_ZYX, F).astype(np.float64), np.array(RANGE_ZYX, F).astype(np.float64)
    for b, calib in enumerate(calibs):
        m = coords[:, 0] == b
        if not m.any():
            continue
        idx = (coords[m, 1:].astype(np.int64) * stride).astype(np.float64)                  # exact in fp32 too (below 2^24)
        z, y, x = (V(idx[:, k]) * V(vs[k]) + V(org[k]) for k in range(3))
        scale, rot, flip_x, flip_y = _aug_values(case, b)
        if scale is not None:
            x, y, z = x / V(float(scale)), y / V(float(scale)), z / V(float(scale))
        if rot is not None:
            ang = -float(rot)
            trig = TRIG_ULPS * 2 * half_ulp(1.0)
            c, s = V(np.cos(ang), trig), V(np.sin(ang), trig)
            zero = V(0.0)
            x, y = dot([(x, c), (y, -s), (z, zero)]), dot([(x, s), (y, c), (z, zero)])
        if flip_x:
            y = -y
        if flip_y:
            x = -x
        M, Merr = calib_matrix(calib)
        one = V(1.0)
        rect = [dot([(x, V(M[0, j], Merr[0, j])), (y, V(M[1, j], Merr[1, j])), (z, V(M[2, j], Merr[2, j])), (one, V(M[3, j], Merr[3, j]))])
                for j in range(3)]
        P = np.asarray(calib.P2, F).astype(np.float64)
        p = [dot([(rect[0], V(P[k, 0])), (rect[1], V(P[k, 1])), (rect[2], V(P[k, 2])), (one, V(P[k, 3]))]) for k in range(2)]
        u, v = p[0] / rect[2], p[1] / rect[2]
        for dst, src in zip(out, (u.val, v.val, rect[2].val, u.err, v.err)):
            dst[m] = src
    return tuple(out)


def pixel_mask(u, v, rz, bu, bv):
    """True: the voxel's pixel is not compared (an integer within the bound of u or v, no bound, or |rect_z| under the floor)"""
    with np.errstate(invalid="ignore"):
        near = (np.abs(u - np.rint(u)) <= bu) | (np.abs(v - np.rint(v)) <= bv)
        return near | ~np.isfinite(bu) | ~np.isfinite(bv) | ~(np.abs(rz) >= RECT_Z_FLOOR)


def pixels(u, v, image_hw):
    """v * W + u with u, v truncated toward zero as .long() does, -1 where the reference's filter (:96) drops the voxel or a coordinate is not finite"""
    H, W = image_hw
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    ok = np.isfinite(u) & np.isfinite(v)
    ut, vt = np.trunc(np.where(ok, u, -5.0)), np.trunc(np.where(ok, v, -5.0))
    ok &= (0 <= ut) & (ut < W) & (0 <= vt) & (vt < H)
    return np.where(ok, vt * W + ut, -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ cases
def make_case(name):
    """The seeded inputs of a case: coords (n, 4) int32 with interleaved scenes, calibs, the aug keys, features (B, h, w, C), f (n, C) and the
    upstream gradients of both modes.  Rows are drawn from a pool of random cells so that about 70 % project into the image; one or two rows per
    scene have u in (-1, 0) with v inside; `cluster` adds a 12 x 4 block of far voxels that share a pixel or two."""
    case = dict(next(c for c in CASES if c["name"] == name))
    rng = np.random.RandomState(1000 + CASE_NAMES.index(name))
    B, (H, W), (h, w), C = len(case["rows"]), case["image"], case["feat"], case["C"]
    calibs = [make_calib((H, W), b) for b in range(B)]
    chosen = []
    for b, rows in enumerate(case["rows"]):
        if rows == 0:
            continue
        pool = np.stack([np.full(POOL, b), rng.randint(0, GRID_ZYX[0], POOL), rng.randint(0, GRID_ZYX[1], POOL), rng.randint(0, GRID_ZYX[2], POOL)],
                        axis=1).astype(np.int32)
        pool = np.unique(pool, axis=0)
        u, v, rz, bu, bv = project64(case, calibs, pool)
        clear = ~pixel_mask(u, v, rz, bu, bv)
        inside = pixels(u, v, (H, W)) >= 0
        edge = np.flatnonzero(clear & (u > -0.9) & (u < -0.1) & (v > 0.1) & (v < H - 0.1))[:2]
        assert len(edge) > 0, f"{name}: no voxel with u in (-1, 0) in scene {b}'s pool"
        n_in = int(0.7 * rows)
        take_in = rng.choice(np.flatnonzero(inside), n_in, replace=False)
        take_out = rng.choice(np.flatnonzero(~inside), rows - n_in - len(edge), replace=False)
        chosen.append(pool[np.concatenate([take_in, take_out, edge])])
    if case["cluster"]:
        block = np.array([[1, 20, iy, ix] for iy in range(798, 802) for ix in range(1380, 1392)], np.int32)
        chosen.append(block)
    coords = np.unique(np.concatenate(chosen), axis=0)
    coords = coords[rng.permutation(len(coords))]                       # the scenes interleave
    n = len(coords)
    case.update(B=B, calibs=calibs, coords=np.ascontiguousarray(coords), n=n,
                features=rng.randn(B, h, w, C).astype(F), f=rng.randn(n, C).astype(F),
                g_concat=rng.randn(n, 2 * C).astype(F), g_sum=rng.randn(n, C).astype(F))
    return case


def batch_dict_aug(case, device=None):
    """the augmentation keys of a case as batch_dict carries them (only the keys the case has)"""
    out = {}
    for key, values in case["aug"].items():
        out[key] = torch.tensor(values, dtype=torch.bool if key.startswith("flip") else torch.float32, device=device)
    return out


# ------------------------------------------------------------------------------------------------------------ sampling
def _axis(d, n_in, n_out):
    num = n_in * (2 * d.astype(np.int64) + 1) - n_out
    den = 2 * n_out
    pos = num > 0
    i0 = np.where(pos, num // den, 0)
    rem = np.where(pos, num - i0 * den, 0)
    i1 = i0 + (i0 < n_in - 1)
    l1_32 = rem.astype(F) / F(den)
    return i0, i1, (F(1) - l1_32, l1_32), (1.0 - rem / den, rem / den)


def taps(image_hw, feat_hw, pix):
    """For pixels pix >= 0: low-resolution pixel (n, 4) within the scene, weights (n, 4) fp32 as the kernel forms them, weights (n, 4) float64
    exact; taps t = 0..3 = (y0,x0), (y0,x1), (y1,x0), (y1,x1)."""
    (H, W), (h, w) = image_hw, feat_hw
    pix = np.asarray(pix, np.int64)
    v, u = pix // W, pix % W
    y0, y1, ly32, ly64 = _axis(v, h, H)
    x0, x1, lx32, lx64 = _axis(u, w, W)
    px = np.stack([y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1], axis=1)
    w32 = np.stack([ly32[0] * lx32[0], ly32[0] * lx32[1], ly32[1] * lx32[0], ly32[1] * lx32[1]], axis=1).astype(F)
    w64 = np.stack([ly64[0] * lx64[0], ly64[0] * lx64[1], ly64[1] * lx64[0], ly64[1] * lx64[1]], axis=1)
    return px, w32, w64


def image_rows64(features, coords, pix, image_hw):
    """img (n, C) float64 by the 4-tap statement (or the pixel itself at equal sizes), zero where pix < 0; and sum over taps of |f_t| w_t"""
    B, h, w, C = features.shape
    flat = features.reshape(B, h * w, C).astype(np.float64)
    img, mag = np.zeros((len(pix), C)), np.zeros((len(pix), C))
    ok = np.flatnonzero(pix >= 0)
    b = coords[ok, 0]
    if (h, w) == tuple(image_hw):
        img[ok] = flat[b, pix[ok]]
        mag[ok] = np.abs(img[ok])
        return img, mag
    px, _, w64 = taps(image_hw, (h, w), pix[ok])
    for t in range(4):
        img[ok] += flat[b, px[:, t]] * w64[:, t:t + 1]
        mag[ok] += np.abs(flat[b, px[:, t]]) * w64[:, t:t + 1]
    return img, mag


def image_rows_interp64(features, coords, pix, image_hw):
    """the same through F.interpolate(bilinear, align_corners=False) in float64 and indexing, as the reference goes (:69-70, :102-103)"""
    B, h, w, C = features.shape
    H, W = image_hw
    x = torch.from_numpy(features.astype(np.float64)).permute(0, 3, 1, 2)
    if (h, w) != (H, W):
        x = TF.interpolate(x, (H, W), mode="bilinear")
    x = x.permute(0, 2, 3, 1).reshape(B, H * W, C).numpy()
    img = np.zeros((len(pix), C))
    ok = np.flatnonzero(pix >= 0)
    img[ok] = x[coords[ok, 0], pix[ok]]
    return img


def forward64(case, pix, fuse_sum):
    img, _ = image_rows64(case["features"], case["coords"], pix, case["image"])
    f = case["f"].astype(np.float64)
    return f + img if fuse_sum else np.concatenate([img, f], axis=1)


def forward_bound(case, pix, fuse_sum):
    """Per element: what an fp32 evaluation of img = ((f0 w0 + f1 w1) + f2 w2) + f3 w3 (and of f + img) may differ from forward64 by.  Each weight
    is a product of two factors, the upper one a correctly rounded quotient (relative u), the lower 1 - upper (that error plus half an ulp of a
    number <= 1): each factor is within 2 u absolutely, the product within (4 u + 4 u^2) + u <= 6 u of the exact weight (factors <= 1).  The four
    products and three sums add gamma_4 * sum|f_t| w_t.  Equal sizes read the value itself: no error.  The copy of f in a concat is exact."""
    img, mag = image_rows64(case["features"], case["coords"], pix, case["image"])
    C = case["C"]
    if tuple(case["feat"]) == tuple(case["image"]):
        e_img = np.zeros_like(img)
    else:
        B, h, w, _ = case["features"].shape
        flat = np.abs(case["features"].reshape(B, h * w, C).astype(np.float64))
        tapsum = np.zeros_like(img)
        ok = np.flatnonzero(pix >= 0)
        px, _, _ = taps(case["image"], case["feat"], pix[ok])
        for t in range(4):
            tapsum[ok] += flat[case["coords"][ok, 0], px[:, t]]
        e_img = 6 * U * tapsum + (4 * U / (1 - 4 * U)) * (mag + 6 * U * tapsum)
    if fuse_sum:
        total = case["f"].astype(np.float64) + img
        return e_img + half_ulp(np.abs(total) + e_img)
    return np.concatenate([e_img, np.zeros((len(pix), C))], axis=1)


def grad_loop32(case, pix, g):
    """grad_features (B, h, w, C) fp32: +0 + sum of g[i, :C] * w_t over the keys of each low-resolution pixel in ASCENDING key (4 i + t, or i at
    equal sizes), every product and sum rounded to fp32; also the longest list."""
    B, h, w, C = case["features"].shape
    coords = case["coords"]
    out = np.zeros((B * h * w, C), F)
    count = np.zeros(B * h * w, np.int64)
    equal = (h, w) == tuple(case["image"])
    g = np.asarray(g, F)
    ok = np.flatnonzero(pix >= 0)
    px, w32, _ = taps(case["image"], (h, w), pix[ok])
    for k, i in enumerate(ok):                                           # ascending i, then t: ascending key
        base = int(coords[i, 0]) * h * w
        if equal:
            row = base + int(pix[i])
            out[row] = out[row] + g[i, :C] * F(1)
            count[row] += 1
            continue
        for t in range(4):
            row = base + int(px[k, t])
            out[row] = out[row] + g[i, :C] * w32[k, t]
            count[row] += 1
    return out.reshape(B, h, w, C), int(count.max())
