"""Numpy restatement of what the VC training transforms compute (see/surface_completion/models/vcn/datasets/data_transforms.py), and the clouds the
tests run on.  Nothing here imports the package under test.

  * ring index: np.histogram's equal bins by the edge rule (edges = lo + k * step with the last edge = hi; a point's bin is the b with
    edges[b] <= e < edges[b + 1], the last bin closed) and the 1-based rank of that bin among the non-empty bins, which is what
    np.digitize(e, left edges of the non-empty bins) returns;
  * selection: rows[in1d(ring, chosen)][first::step], rows untouched (the reference's spherical round trip moves a float64 component by about
    1e-15 r, which the float32 cast does not see unless |c| < 2^-24 r);
  * point-wise and rigid transforms in float64.
"""
import numpy as np

MAX_RINGS = 1024
N_POINTS = 1024
VC_CARS_TRAIN = [{'callback': 'LidarSimulation', 'parameters': {}, 'objects': ['partial']},
                 {'callback': 'ResamplePoints', 'parameters': {'n_points': N_POINTS}, 'objects': ['partial']}]
LIDAR_EXITS = {159: "small", 191: "onetwo_fallback", 194: "onetwo", 198: "out", 201: "original"}      # return statements of LidarSimulation.__call__
DOWNSAMPLE_EXITS = {125: "small", 138: "out", 140: "original"}


# ------------------------------------------------------------------------------------------------------------ clouds
def ring_cloud(seed, n, n_rings, row_step_deg=0.4, base_deg=88.0):
    """A ring-like patch 10-14 m from the origin: n points on n_rings elevation rows row_step_deg apart plus 1e-4 rad noise, every row used, rows
    in random order.  Elevation is measured from +z, as cart2sph does.  Returns (n, 3) float32."""
    rng = np.random.RandomState(seed)
    row = np.concatenate([np.arange(n_rings), rng.randint(0, n_rings, n - n_rings)]) if n >= n_rings else np.arange(n)
    row = row[rng.permutation(n)]
    elev = np.deg2rad(base_deg + row * row_step_deg) + 1e-4 * rng.randn(n)
    az = rng.uniform(-0.2, 0.2, n) + rng.uniform(-np.pi, np.pi)
    r = rng.uniform(10.0, 14.0, n)
    return np.stack([r * np.sin(elev) * np.cos(az), r * np.sin(elev) * np.sin(az), r * np.cos(elev)], 1).astype(np.float32)


def make_cases():
    """(names, clouds): the 14 clouds of tests/golden/vc_transforms.npz.  n = 99 (untouched), 100, 101, 256, 257, 1024 (32 bins), 1025 (33 bins),
    4097 (65 bins); 1, 2 and 3 rings; 120 copies of one point (lo == hi); rows 2 degrees apart (empty bins between the rings); one point alone
    on the highest row (the maximum elevation, which the last bin includes)."""
    cases = [("n99", ring_cloud(1, 99, 8)), ("n100", ring_cloud(2, 100, 8)), ("n101", ring_cloud(3, 101, 9)), ("n256", ring_cloud(4, 256, 12)),
             ("n257", ring_cloud(5, 257, 12)), ("n1024", ring_cloud(6, 1024, 16)), ("n1025", ring_cloud(7, 1025, 16)),
             ("n4097", ring_cloud(8, 4097, 24)), ("rings1", ring_cloud(9, 150, 1)), ("rings2", ring_cloud(10, 200, 2)),
             ("rings3", ring_cloud(11, 300, 3))]
    one = ring_cloud(12, 1, 1)
    cases.append(("copies120", np.repeat(one, 120, 0)))
    cases.append(("gaps", ring_cloud(13, 400, 6, row_step_deg=2.0)))
    top = ring_cloud(14, 299, 7)
    e = elevation(top)
    lone = ring_cloud(15, 1, 1, base_deg=float(np.rad2deg(e.max())) + 0.4)
    cases.append(("lone_top", np.concatenate([top[:150], lone, top[150:]])))
    return [c[0] for c in cases], [c[1] for c in cases]


def make_boxes(clouds, seed=77):
    """One box (x, y, z, l, w, h, heading) float64 per cloud, centred near the cloud."""
    rng = np.random.RandomState(seed)
    return np.stack([np.concatenate([c.astype(np.float64).mean(0) + rng.uniform(-0.5, 0.5, 3), rng.uniform([3.5, 1.5, 1.4], [4.8, 2.0, 1.9]),
                                     rng.uniform(-np.pi, np.pi, 1)]) for c in clouds])


def make_complete(clouds, seed=78, n=64):
    """A small 'complete' cloud per object: n points around the partial cloud's mean, float32."""
    rng = np.random.RandomState(seed)
    return [(c.astype(np.float64).mean(0) + rng.uniform(-2.0, 2.0, (n, 3))).astype(np.float32) for c in clouds]


# ------------------------------------------------------------------------------------------------------------ ring index
def elevation(p32):
    """cart2sph's elevation of float32 rows taken to float64: arctan2(sqrt(x * x + y * y), z)."""
    p = np.asarray(p32, np.float64)
    return np.arctan2(np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]), p[:, 2])


def bin_count(elev, bins):
    """The number of equal bins: `bins` itself, or for 'sqrt' ceil(ptp / (ptp / sqrt(n))) in numpy's float64 steps (1 when ptp == 0)."""
    if bins != 'sqrt':
        return int(bins)
    lo, hi = elev.min(), elev.max()
    width = (hi - lo) / np.sqrt(elev.size)
    return int(np.ceil((hi - lo) / width)) if width else 1


def bin_edges(lo, hi, nb):
    step = (hi - lo) / nb
    edges = np.arange(0, nb + 1) * step + lo
    edges[-1] = hi
    return edges


def ring_index(elev, bins='sqrt'):
    """(ring (n,) 1-based, num_rings, ring_cnt (MAX_RINGS,)) by the edge rule."""
    lo, hi = elev.min(), elev.max()
    ring_cnt = np.zeros(MAX_RINGS, np.int64)
    if lo == hi:                                                     # np.histogram widens the range to lo -+ 0.5: one non-empty bin
        ring_cnt[0] = len(elev)
        return np.ones(len(elev), np.int64), 1, ring_cnt
    nb = bin_count(elev, bins)
    edges = bin_edges(lo, hi, nb)
    b = np.minimum(np.searchsorted(edges, elev, side='right') - 1, nb - 1)
    hist = np.bincount(b, minlength=nb)
    rank = np.cumsum(hist > 0)                                       # 1-based rank of a non-empty bin
    ring = rank[b]
    num_rings = int(rank[-1])
    ring_cnt[:num_rings] = hist[hist > 0]
    return ring.astype(np.int64), num_rings, ring_cnt


def ring_table(p32, bins='sqrt', min_in_pts=0):
    """What sv_vc_rings returns for one object: a cloud below min_in_pts is not looked at."""
    if len(p32) < min_in_pts:
        return np.zeros(len(p32), np.int64), 0, np.zeros(MAX_RINGS, np.int64)
    return ring_index(elevation(p32), bins)


def edge_distance_ulps(elev, bins='sqrt'):
    """The smallest distance, in ulps of the elevation, between a point that is neither the minimum nor the maximum and an inner bin edge
    (inf when there is no such pair)."""
    lo, hi = elev.min(), elev.max()
    if lo == hi:
        return np.inf
    nb = bin_count(elev, bins)
    inner = bin_edges(lo, hi, nb)[1:-1]
    e = elev[(elev != lo) & (elev != hi)]
    if len(inner) == 0 or len(e) == 0:
        return np.inf
    d = np.abs(e[:, None] - inner[None, :]).min(1)
    return float((d / np.spacing(np.abs(e))).min())


# ------------------------------------------------------------------------------------------------------------ selection
def select(p32, ring, plan, keep=None):
    """The rows a plan keeps: pass-through, or rows[mask][first::step] with mask = chosen rings (and the keep mask)."""
    if plan["pass"]:
        return p32
    mask = np.ones(len(p32), bool) if plan["rings"] is None else np.isin(ring, plan["rings"])
    if keep is not None:
        mask &= np.asarray(keep, bool)
    return p32[mask][plan["first"]::plan["step"]]


def is_ordered_subset(rows, p32):
    """rows is a subsequence of p32's rows, bit for bit."""
    a, b = np.ascontiguousarray(rows, np.float32).view(np.uint32), np.ascontiguousarray(p32, np.float32).view(np.uint32)
    j = 0
    for row in a:
        while j < len(b) and not np.array_equal(b[j], row):
            j += 1
        if j == len(b):
            return False
        j += 1
    return True


# ------------------------------------------------------------------------------------------------------------ point-wise, float64
def jitter(p32, noise):
    return np.asarray(p32, np.float64) + noise


def gn_spherical(p32, noise):
    """sph2cart(cart2sph(p) with r += noise), the spherical route in float64."""
    p = np.asarray(p32, np.float64)
    r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    el, az = elevation(p32), np.arctan2(p[:, 1], p[:, 0])
    r = r + noise
    return np.stack([r * np.sin(el) * np.cos(az), r * np.sin(el) * np.sin(az), r * np.cos(el)], 1)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ rigid and scale, float64
def rotate_z(p, angle):
    """points @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] in float64; also returns |x||c| + |y||s| per x / y component for the fp32 matmul's bound."""
    p = np.asarray(p, np.float64)
    c, s = np.cos(angle), np.sin(angle)
    out = np.stack([p[:, 0] * c - p[:, 1] * s, p[:, 0] * s + p[:, 1] * c, p[:, 2]], 1)
    mag = np.stack([np.abs(p[:, 0] * c) + np.abs(p[:, 1] * s), np.abs(p[:, 0] * s) + np.abs(p[:, 1] * c), np.zeros(len(p))], 1)
    return out, mag


def world_flip(p, axis):
    out = np.array(p, np.float64)
    out[:, 1 if axis == "flip_x" else 0] *= -1
    return out


def flip_box(box, axis):
    box = np.array(box, np.float64)
    if axis == "flip_x":
        box[1], box[6] = -box[1], -box[6]
    else:
        box[0], box[6] = -box[0], -(box[6] + np.pi)
    return box


def object_scaling(p, box, scale):
    """Into the box frame, times the scale, back, in float64.  Also returns M (n, 1) = 2 max|scale| (|dx| + |dy| + |dz|) with d = p - centre, which no
    intermediate component of the reference's fp32 route exceeds.  That route rounds to fp32 after the difference (1 unit of 2^-24 M), in the first
    rotation (4, the bound of the fp32 matmul, + 1 for the rounded input), after the scaling (1) and in the second rotation (4): 11 units; OBJECT_SCALE_UNITS
    adds one for fp32 cos / sin that differ by an ulp between two libraries."""
    p = np.asarray(p, np.float64)
    d = p - box[:3]
    cn, _ = rotate_z(d, -box[6])
    out, _ = rotate_z(cn * scale, box[6])
    return out + box[:3], 2 * np.max(np.abs(scale)) * np.abs(d).sum(1, keepdims=True)


OBJECT_SCALE_UNITS = 12
