"""Case generators and float64 references for the edge tests of csrc/voxelize.hip (tests/test_voxel_edges.py).

Generators build inputs that sit ON an edge of the kernels (cell faces, the 1024-block seam of the hard voxeliser's scan, a voxel cap inside
a 256-point block, the 2^16-point / 2^15-magnitude limits of the fixed-point sums); test_voxel_edges.py proves on the CPU that each really
does.  The references restate MeanVFE and the PillarVFE decoration from their definitions in float64, and the tolerance functions bound what
fp32 arithmetic may lose against them.

Error model (u = 2^-24, the unit round-off of fp32, round to nearest):
  * a sum of n fp32 terms accumulated one after another IN ANY ORDER differs from the exact sum by at most (n - 1) * u * sum|x_i|
    (Jeannerod & Rump 2013, "Improved error bounds for inner products in floating-point arithmetic": the bound holds without higher-order terms);
  * every other operation (+, -, *, /, sqrt; the build rounds divide and sqrt correctly and never contracts a*b+c) is off by at most half an
    ulp of its result; `half_ulp(m)` is evaluated at an upper bound m of the result's magnitude, ulp being monotone in the magnitude;
  * an error e in the operand of the next operation passes through: unchanged by + and -, divided by n by the divide, and through sqrt by
    |sqrt(S + e) - sqrt(S)| = e / (sqrt(S + e) + sqrt(S)) <= e / (sqrt(S) + sqrt(max(S - e, 0))).
"""
import numpy as np

F = np.float32
U = 2.0 ** -24

KITTI = dict(lo=[0.0, -40.0, -3.0], vs=[0.05, 0.05, 0.1], grid=[1408, 1600, 40], pc_range=[0, -40, -3, 70.4, 40, 1])
PILLAR = dict(lo=[0.0, -39.68, -3.0], vs=[0.16, 0.16, 4.0], grid=[432, 496, 1], pc_range=[0, -39.68, -3, 69.12, 39.68, 1])
NUSC = dict(lo=[-51.2, -51.2, -5.0], vs=[0.2, 0.2, 8.0], grid=[512, 512, 1], pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0])
UNIT = dict(lo=[0.0, 0.0, 0.0], vs=[1.0, 1.0, 1.0], grid=[8, 6, 4], pc_range=[0, 0, 0, 8, 6, 4])
GEOMS = {"kitti": KITTI, "pillar": PILLAR, "nusc": NUSC, "unit": UNIT}

HV_BLOCK = 256                       # points per workgroup of the hard voxeliser
HV_SEAM = 1024 * HV_BLOCK            # first point of the second pass of its offset scan


def half_ulp(mag):
    """Half an ulp of an fp32 result whose magnitude is at most `mag` (float64 array)."""
    return 0.5 * np.spacing(np.abs(np.asarray(mag, np.float64)).astype(F)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- cell arithmetic
def cells_fp32(xyz, lo, vs):
    """The reference's floor((p - lo) / vs) in fp32: IEEE subtract, IEEE divide, floor; returned as float (NaN stays NaN)."""
    return np.floor((np.asarray(xyz, F) - np.asarray(lo, F)) / np.asarray(vs, F))


def cells_reciprocal(xyz, lo, vs):
    """The same with a multiply by the fp32 reciprocal in place of the divide."""
    return np.floor((np.asarray(xyz, F) - np.asarray(lo, F)) * (F(1.0) / np.asarray(vs, F)))


def cells_fp64(xyz, lo, vs):
    """The same carried out in float64 on the fp32 inputs."""
    return np.floor((np.asarray(xyz, F).astype(np.float64) - np.asarray(lo, F).astype(np.float64)) / np.asarray(vs, F).astype(np.float64))


def face_points(lo, vs, grid, n, seed):
    """(4n + 6, 3) fp32 points on and next to cell faces: for n random integer triples k in [0, grid] the point fp32(lo + k*vs), its
    nextafter-up and nextafter-down neighbours (all three axes moved together) and one row whose axes are moved up, down or not at all
    independently; then lo and hi = fp32(lo + grid*vs) themselves with their two neighbours."""
    rng = np.random.default_rng(seed)
    lo64, vs64, g = np.asarray(lo, np.float64), np.asarray(vs, np.float64), np.asarray(grid, np.int64)
    k = np.stack([rng.integers(0, g[a] + 1, n) for a in range(3)], axis=1)
    base = (lo64 + k * vs64).astype(F)
    up, down = np.nextafter(base, F(np.inf)), np.nextafter(base, F(-np.inf))
    pick = rng.integers(0, 3, (n, 3))
    mixed = np.where(pick == 0, down, np.where(pick == 1, base, up))
    ends = []
    for e in (lo64.astype(F), (lo64 + g * vs64).astype(F)):
        ends += [e, np.nextafter(e, F(np.inf)), np.nextafter(e, F(-np.inf))]
    return np.ascontiguousarray(np.concatenate([base, up, down, mixed, np.stack(ends)]).astype(F))


def first_appearance(xyz, geom):
    """Cells in the order the sequential walk opens them, from numpy alone: (first, coords) with first[j] = index of the first point of the
    j-th cell to appear and coords[j] = its (z, y, x)."""
    c = cells_fp32(xyz, geom["lo"], geom["vs"])
    g = np.asarray(geom["grid"], np.int64)
    with np.errstate(invalid="ignore"):
        ok = ((c >= 0) & (c < g.astype(F))).all(1)
    idx = np.nonzero(ok)[0]
    ci = c[idx].astype(np.int64)
    key = (ci[:, 2] * g[1] + ci[:, 1]) * g[0] + ci[:, 0]
    _, where = np.unique(key, return_index=True)
    where = np.sort(where)
    return idx[where], ci[where][:, ::-1].astype(np.int32)


# ---------------------------------------------------------------------------------------------------- hard voxeliser scenes
SEAM_GEOM = dict(lo=[0.0, -8.0, -2.0], vs=[0.1, 0.1, 0.5], grid=[160, 160, 8], pc_range=[0, -8, -2, 16, 8, 2])


def _out_of_range(rng, xyz, rows, geom):
    """Move one random axis of xyz[rows] past a random end of the range."""
    lo, hi = np.asarray(geom["pc_range"][:3], np.float64), np.asarray(geom["pc_range"][3:], np.float64)
    axis = rng.integers(0, 3, len(rows))
    above = rng.random(len(rows)) < 0.5
    d = rng.uniform(0.01, 5.0, len(rows))
    xyz[rows, axis] = np.where(above, hi[axis] + d, lo[axis] - d)


def seam_scene(seed):
    """One scene of 1025*256 + 37 points [x, y, z, f] over SEAM_GEOM that crosses the 1024-block seam of k_hv_offsets.  About nine points in
    ten are out of range.  Points before the seam fall in the half x < 8 (one in five of them in a hot 3 x 3 x 1 block of cells, so voxels
    fill up), most points after it in the half x >= 8, whose cells are therefore first touched past point 1024*256."""
    rng = np.random.default_rng(seed)
    n = 1025 * HV_BLOCK + 37
    late = np.arange(n) >= HV_SEAM
    xyz = np.stack([rng.uniform(0, 8, n), rng.uniform(-8, 8, n), rng.uniform(-2, 2, n)], axis=1)
    far = late & (rng.random(n) < 0.8)
    xyz[far, 0] += 8.0
    hot = ~late & (rng.random(n) < 0.2)
    xyz[hot] = np.stack([rng.uniform(1.0, 1.3, hot.sum()), rng.uniform(0.0, 0.3, hot.sum()), rng.uniform(0.0, 0.5, hot.sum())], axis=1)
    out = np.nonzero(rng.random(n) < np.where(late, 0.3, 0.9))[0]
    _out_of_range(rng, xyz, out, SEAM_GEOM)
    pts = np.concatenate([xyz, rng.normal(size=(n, 1))], axis=1).astype(F)
    return np.ascontiguousarray(pts), SEAM_GEOM


TILE_GEOM = dict(lo=[0.0, 0.0, 0.0], vs=[1.0, 1.0, 1.0], grid=[32, 32, 2], pc_range=[0, 0, 0, 32, 32, 2])


def tile_edge_scenes(seed):
    """(big, small, geom): a scene of 1024*256 + 1 points [x, y, z, f] -- 1025 point blocks, one past the tile of the scan of the block counts,
    the last block holding one point -- and a scene of 255 points, over the coarse TILE_GEOM (2048 cells).  In the big scene the cells open
    gradually (point i falls among the first 1 + i * 2046 // n cells of a shuffled list), so first points lie in blocks all along the scene,
    and the very last point opens the one cell kept back for it: its voxel number is the sum of all 1024 block counts before it."""
    rng = np.random.default_rng(seed)
    g = np.asarray(TILE_GEOM["grid"])
    order = rng.permutation(int(g.prod()))
    n = 1024 * HV_BLOCK + 1
    pick = (rng.random(n) * (1 + np.arange(n) * (len(order) - 2) // n)).astype(np.int64)
    pick[-1] = len(order) - 1
    scenes = []
    for cell in (order[pick], order[rng.integers(0, len(order), HV_BLOCK - 1)]):
        ijk = np.stack([cell % g[0], cell // g[0] % g[1], cell // (g[0] * g[1])], axis=1)
        xyz = ijk + rng.uniform(0.05, 0.95, ijk.shape)
        scenes.append(np.ascontiguousarray(np.concatenate([xyz, rng.normal(size=(len(xyz), 1))], axis=1).astype(F)))
    return scenes[0], scenes[1], TILE_GEOM


CAP_GEOM = dict(lo=[0.0, 0.0, 0.0], vs=[1.0, 1.0, 1.0], grid=[40, 40, 4], pc_range=[0, 0, 0, 40, 40, 4])
CAP_BLOCK = 4                        # the 256-point block the cap falls into


def cap_cut_scene(seed):
    """(points, geom, max_points, max_voxels): 2660 points [x, y, z, f] over CAP_GEOM and the voxel cap that makes the last admitted first
    point sit strictly inside block CAP_BLOCK: neither that block's first nor its last first point.  Every later block then holds only
    first points past the cap."""
    rng = np.random.default_rng(seed)
    n = 10 * HV_BLOCK + 100
    xyz = np.stack([rng.uniform(0, 40, n), rng.uniform(0, 40, n), rng.uniform(0, 4, n)], axis=1)
    _out_of_range(rng, xyz, np.nonzero(rng.random(n) < 0.15)[0], CAP_GEOM)
    pts = np.ascontiguousarray(np.concatenate([xyz, rng.normal(size=(n, 1))], axis=1).astype(F))
    first, _ = first_appearance(pts[:, :3], CAP_GEOM)
    block = first // HV_BLOCK
    before, inside = int((block < CAP_BLOCK).sum()), int((block == CAP_BLOCK).sum())
    assert inside >= 3
    return pts, CAP_GEOM, 4, before + inside // 2 + 1


DENSE_GEOM = dict(lo=[-2.0, -2.0, 0.0], vs=[1.0, 1.0, 2.0], grid=[4, 4, 2], pc_range=[-2, -2, 0, 2, 2, 4])
DENSE_HEAVY, DENSE_EXACT, DENSE_PLUS1 = (1, 2, 0), (3, 0, 1), (0, 3, 1)        # (x, y, z) cells


def dense_cells(seed, max_points, stride, xyz_offset):
    """(N, stride) rows over the 4 x 4 x 2 DENSE_GEOM with xyz in columns xyz_offset..+2 and random values everywhere else: cell DENSE_HEAVY
    holds 20*max_points + 7 points, DENSE_EXACT exactly max_points, DENSE_PLUS1 max_points + 1; 1200 more points are spread over the other
    29 cells and 200 lie out of range.  Shuffled."""
    rng = np.random.default_rng(seed)
    others = [(x, y, z) for x in range(4) for y in range(4) for z in range(2) if (x, y, z) not in (DENSE_HEAVY, DENSE_EXACT, DENSE_PLUS1)]
    cells = [DENSE_HEAVY] * (20 * max_points + 7) + [DENSE_EXACT] * max_points + [DENSE_PLUS1] * (max_points + 1)
    cells += [others[i] for i in rng.integers(0, len(others), 1400)]
    cells = np.asarray(cells, np.float64)
    n = len(cells)
    xyz = np.asarray(DENSE_GEOM["lo"]) + (cells + rng.uniform(0.05, 0.95, (n, 3))) * np.asarray(DENSE_GEOM["vs"])
    _out_of_range(rng, xyz, np.arange(n - 200, n), DENSE_GEOM)
    rows = rng.normal(size=(n, stride))
    rows[:, xyz_offset:xyz_offset + 3] = xyz
    if xyz_offset:
        rows[:, :xyz_offset] = 0.0                                                  # a batch column in front
    return np.ascontiguousarray(rows[rng.permutation(n)].astype(F)), DENSE_GEOM


# ---------------------------------------------------------------------------------------------------- dynamic voxeliser
CUT_GEOM = dict(lo=[-65536.0] * 3, vs=[65536.0] * 3, grid=[2, 2, 2], pc_range=[-65536.0] * 3 + [65536.0] * 3)
VMAX = float(np.nextafter(F(32768.0), F(0.0)))            # the largest fp32 below 2^15
FIXED_MAX_POINTS = 65536


def cutover_points(seed):
    """Points [b, x, y, z, f] on the 2 x 2 x 2 CUT_GEOM (cells of side 2^16 around the origin, so the sign pattern of xyz picks the cell and
    all four features of a voxel can sit at the limits of the fixed-point sums).  Returns (points, voxels) with voxels[name] = the sign
    pattern (sx, sy, sz) of the voxel:
      a  65536 points, every feature = VMAX                 b  the same, every feature = -VMAX
      c  65536 + 64 points, |features| in [0.5, 1)          d  65536 + 4464 points, |features| in [0.5, 1)
      e  40 ordinary values and one f = 2^15 exactly        f  65536 + 1 points, |features| = VMAX
      g  65536 points, |features| = 2^15 exactly
    c and d draw multiples of 2^-10: the fp32 side sum of the points past the 65536th (fewer than 2^13 values below 1) is then exact
    whichever points arrive late and in whatever order, so the result cannot depend on the permutation.  f overflows the 64-bit sum if
    the 65537th point is added in fixed point, g if a value of exactly 2^15 is."""
    rng = np.random.default_rng(seed)
    voxels = dict(a=(1, 1, 1), b=(-1, -1, -1), c=(1, 1, -1), d=(1, -1, 1), e=(-1, 1, 1), f=(-1, -1, 1), g=(1, -1, -1))
    counts = dict(a=65536, b=65536, c=65536 + 64, d=65536 + 4464, e=41, f=65537, g=65536)
    rows = []
    for name, sign in voxels.items():
        n = counts[name]
        if name in "abf":
            mag = np.full((n, 4), VMAX)
        elif name == "g":
            mag = np.full((n, 4), 32768.0)
        elif name in "cd":
            mag = rng.integers(512, 1024, (n, 4)) / 1024.0
        else:
            mag = rng.uniform(0.5, 900.0, (n, 4))
            mag[17, 3] = 32768.0
        s = np.asarray(list(sign) + [-1.0 if name == "b" else 1.0])
        rows.append(np.concatenate([np.zeros((n, 1)), mag * s], axis=1))
    return np.ascontiguousarray(np.concatenate(rows).astype(F)), voxels


def cut_voxel_rows(points, sign):
    """Rows of `points` that fall in the voxel with sign pattern `sign`."""
    return np.nonzero(((points[:, 1:4] >= 0) == (np.asarray(sign) > 0)).all(1))[0]


def fixed_mean_tol(want64):
    """Bound of test_voxelize.py for a mean whose sum was taken in fixed point: one ulp of the fp32-rounded float64 mean, plus 2^-32."""
    return np.spacing(np.abs(want64.astype(F))).astype(np.float64) + 2.0 ** -32


def atomic_mean_tol(values):
    """Bound for the fp32-only path (more than 4 features) on the mean of values (n, C) of one voxel: fp32 atomic adds accumulate the n
    terms one after another in arrival order, each rounded to nearest, so the sum is off by at most (n - 1) * u * sum|v| in any order; the
    correctly rounded divide by n adds half an ulp of the quotient, whose magnitude is at most (|sum| + sum error) / n."""
    v = np.abs(values.astype(np.float64))
    n = len(v)
    esum = (n - 1) * U * v.sum(0)
    return esum / n + half_ulp((np.abs(values.astype(np.float64).sum(0)) + esum) / n)


# ---------------------------------------------------------------------------------------------------- MeanVFE and the decoration
def vfe_case(seed, V, max_points, C, geom, nonzero_padding):
    """Hard-voxel shaped inputs: voxels (V, max_points, C) whose xyz lie inside their pillar, counts spanning 0..max_points (count 0 and
    count max_points both present from V >= 2 on), coords (V, 4) [b, z, y, x] including the origin cell and the grid's far corner.  Slots past
    the count are zero, or left holding points when `nonzero_padding`."""
    rng = np.random.default_rng(seed)
    g = np.asarray(geom["grid"], np.int64)
    nump = rng.integers(0, max_points + 1, V).astype(np.int32)
    if V >= 1:
        nump[-1] = max_points
    if V >= 2:
        nump[0] = 0
    if V >= 3:
        nump[1] = 1
    xyz_cell = np.stack([rng.integers(0, g[a], V) for a in range(3)], axis=1)
    if V >= 2:
        xyz_cell[0], xyz_cell[-1] = 0, g - 1
    coords = np.concatenate([rng.integers(0, 2, (V, 1)), xyz_cell[:, ::-1]], axis=1).astype(np.int32)
    lo, vs = np.asarray(geom["lo"]), np.asarray(geom["vs"])
    vox = rng.normal(size=(V, max_points, C))
    xyz = lo + (xyz_cell[:, None, :] + rng.uniform(0.0, 1.0, (V, max_points, 3))) * vs
    ncopy = min(C, 3)
    vox[:, :, :ncopy] = xyz[:, :, :ncopy]
    if not nonzero_padding:
        vox[np.arange(max_points)[None, :] >= nump[:, None]] = 0.0
    return np.ascontiguousarray(vox.astype(F)), nump, np.ascontiguousarray(coords)


def mean_vfe_ref(voxels, nump):
    """MeanVFE from its definition in float64: the sum over ALL slots divided by max(count, 1).  Returns (mean, tol): the slot sum loses at
    most (max_points - 1) * u * sum|x|, the divide passes that on divided by the count and adds half an ulp of the quotient."""
    v = voxels.astype(np.float64)
    mp = v.shape[1]
    d = np.maximum(np.asarray(nump, np.float64), 1.0)[:, None]
    want = v.sum(1) / d
    esum = (mp - 1) * U * np.abs(v).sum(1)
    return want, esum / d + half_ulp(np.abs(want) + esum / d)


def pillar_decorate_ref(voxels, nump, coords, voxel_size, pc_range, use_absolute_xyz=True, with_distance=False):
    """The PillarVFE decoration from its definition in float64; returns (features (V, mp, Co), tol of the same shape).

    [raw columns (all, or 3 onwards) | xyz - sum over ALL slots / count | xyz - (coord * voxel + offset) | optionally |xyz|], all times the
    slot mask.  voxel and offset enter as the fp32 values the module uses (offset = voxel/2 + range start of the configured values in float64,
    rounded to fp32 when it meets the fp32 tensor).
    A pillar of count 0 divides by zero: NaN in the cluster columns of every slot (x/0 times the mask 0), as in the module.
    Tolerance per column, from the error model in this file's head:
      raw       p * mask is exact: 0
      cluster   the mean carries e_m = (mp-1) u sum|x| / n + half_ulp(mean); the subtract adds half_ulp(p - mean)
      centre    t1 = coord * voxel: half_ulp; t2 = t1 + offset: + half_ulp; p - t2: + half_ulp
      distance  three squares and two adds, each half an ulp: error e_S of S = x^2 + y^2 + z^2; through the correctly rounded sqrt
                e_S / (sqrt(S) + sqrt(max(S - e_S, 0))) + half_ulp(sqrt)"""
    v = voxels.astype(np.float64)
    V, mp, C = v.shape
    n = np.asarray(nump, np.float64)[:, None]
    mask = (np.arange(mp)[None, :] < np.asarray(nump)[:, None]).astype(np.float64)[..., None]
    xyz = v[:, :, :3]
    cols, tols = [], []
    raw = v if use_absolute_xyz else v[:, :, 3:]
    cols.append(raw)
    tols.append(np.zeros_like(raw))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = xyz.sum(1) / n                                                                    # (V, 3)
        e_m = (mp - 1) * U * np.abs(xyz).sum(1) / n
        e_m = e_m + half_ulp(np.abs(mean) + e_m)
        cluster = xyz - mean[:, None, :]
        cols.append(cluster)
        tols.append(e_m[:, None, :] + half_ulp(np.abs(cluster) + e_m[:, None, :]))
    vs = np.asarray(voxel_size, F).astype(np.float64)
    off = np.asarray([float(F(float(voxel_size[a]) / 2 + float(pc_range[a]))) for a in range(3)])
    cell = coords[:, [3, 2, 1]].astype(np.float64)                                               # x, y, z
    t1 = cell * vs
    e1 = half_ulp(t1)
    t2 = t1 + off
    e2 = e1 + half_ulp(np.abs(t2) + e1)
    centre = xyz - t2[:, None, :]
    cols.append(centre)
    tols.append(e2[:, None, :] + half_ulp(np.abs(centre) + e2[:, None, :]))
    if with_distance:
        sq = xyz * xyz
        S = sq.sum(2, keepdims=True)
        e_sq = half_ulp(sq)
        e_xy = e_sq[..., 0:1] + e_sq[..., 1:2] + half_ulp(sq[..., 0:1] + sq[..., 1:2] + e_sq[..., 0:1] + e_sq[..., 1:2])
        e_S = e_xy + e_sq[..., 2:3]
        e_S = e_S + half_ulp(S + e_S)
        root = np.sqrt(S)
        den = root + np.sqrt(np.maximum(S - e_S, 0.0))
        e_r = np.where(den > 0, e_S / np.where(den > 0, den, 1.0), 0.0)
        cols.append(root)
        tols.append(e_r + half_ulp(root + e_r))
    with np.errstate(invalid="ignore"):
        want = np.concatenate(cols, axis=2) * mask
    tol = np.concatenate(tols, axis=2) * mask
    return want, tol
