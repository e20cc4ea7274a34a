"""Inputs that sit on the branch points of csrc/postprocess.hip, the expectations the kernels are held to on them (oracle/postprocess.py, numpy, or a
float64 restatement written here) and nothing else: tests/test_postprocess_edges.py proves on the CPU that every family does what it claims and holds the
kernels to it on the GPU.  Plain module, no fixtures; everything is computed once (lru_cache) and handed out read-only."""
import functools

import numpy as np

from oracle import postprocess as opp

F32 = np.float32


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------------------------------------- surface selection: query slices
SLICE_BATCHES = (1, 65, 1000, 1366, 2049)
SLICE_N, SLICE_M, SLICE_K, SLICE_SP = 40, 33, 3, 64
NQ_CYCLE = (17, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 31, 33, 40)             # distinct partial rows of object b: NQ_CYCLE[b % 14]
KNN_WAVES = 4                                                         # queries one slice takes per round of k_surface_knn's stride loop


def nsplit_of(batch):
    """sv_vcn_surface_select's query slices per object: clamp(4096 / batch, 1, 64).  Change this with the kernel's formula."""
    return min(max(4096 // batch, 1), 64)


@functools.lru_cache(maxsize=None)
def slice_case(batch):
    """(partial (B, 40, 3), coarse (B, 33, 3), nq (B)): object b has nq[b] distinct partial rows, the other rows are copies of them, shuffled."""
    rng = np.random.default_rng(100 + batch)
    coarse = rng.normal(size=(batch, SLICE_M, 3)).astype(F32)
    base = rng.normal(size=(batch, SLICE_N, 3)).astype(F32)
    nq = np.array([NQ_CYCLE[b % len(NQ_CYCLE)] for b in range(batch)])
    col = np.arange(SLICE_N)[None, :]
    src = np.where(col < nq[:, None], col, rng.integers(0, 1 << 30, (batch, SLICE_N)) % nq[:, None])
    src = np.take_along_axis(src, np.argsort(rng.random((batch, SLICE_N)), axis=1), axis=1)
    partial = np.take_along_axis(base, src[:, :, None], axis=1)
    return _frozen(partial, coarse, nq)


def oracle_surface_batch(partial, coarse, k, surface_pts):
    """oracle.postprocess.partial_with_kdtree per object -> (surface (B, surface_pts, 3) float32, n_selected (B))."""
    res = [opp.partial_with_kdtree(p, c, k, surface_pts) for p, c in zip(partial, coarse)]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res])


@functools.lru_cache(maxsize=None)
def slice_want(batch):
    partial, coarse, _ = slice_case(batch)
    return _frozen(*oracle_surface_batch(partial, coarse, SLICE_K, SLICE_SP))


@functools.lru_cache(maxsize=None)
def full_size_case():
    rng = np.random.default_rng(11)
    partial = (rng.normal(size=(2, 1024, 3)) * 0.4).astype(F32)
    coarse = (rng.normal(size=(2, 1024, 3)) * 0.4).astype(F32)
    return _frozen(partial, coarse)


@functools.lru_cache(maxsize=None)
def full_size_want():
    return _frozen(*oracle_surface_batch(*full_size_case(), 30, 1024))


# ---------------------------------------------------------------------------------------------------------- surface selection: exact distance ties
TIE_SP = 1024                                    # every selected row shows, in set order
TIE_K = tuple(range(1, 10))                      # 8 cell corners tie at a cell centre; a lattice point has itself (and a copy) at 0, then 6 at 1: 1 .. 8 + 1
TIE_CONFIGS = {                                  # name -> (lattice, distinct queries of object 0; object 1 takes all of them)
    "m33": ((3, 3, 3), 4),                       # 27 lattice rows + 6 copies: fewer coarse rows than lanes
    "m113": ((5, 5, 4), 12),                     # 100 + 13 copies: two candidates in lanes 0 .. 48, one in the others
    "m1000": ((10, 10, 10), 40),                 # 992 + 8 copies: 16 candidates in lanes 0 .. 39, 15 in the others
}


def _lattice(shape):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return g.astype(F32)


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """(partial (2, n, 3), coarse (2, m, 3)).  Coarse: an integer lattice in shuffled index order with copies of some rows -- copies of rows 0 .. 64 rows
    behind their originals (the same lane of k_surface_knn), and further copies in other lanes.  Partial: cell centres (8 corners at squared distance
    0.75) and lattice points (the row and its copy at 0, 6 rows at 1, 12 at 2); every coordinate is a small multiple of 0.5, so float64 squared distances
    are exact and equal ones are equal bit for bit.  Object 0 asks few distinct queries (a small selection, whose set order shows every swap), object 1 all."""
    shape, few = TIE_CONFIGS[name]
    partial, coarse = [], []
    for obj in range(2):
        rng = np.random.default_rng(200 + 10 * len(name) + obj + sum(shape))
        L = rng.permutation(_lattice(shape))
        if name == "m33":
            c = np.concatenate([L, L[:6]])
        elif name == "m113":
            c = np.concatenate([L[:64], L[:10], L[64:], L[20:23]])
        else:
            c = np.concatenate([L[:64], L[:8], L[64:992]])
        centres = rng.permutation(_lattice(tuple(s - 1 for s in shape)) + F32(0.5))
        points = np.concatenate([L[:2], rng.permutation(L[2:])])                 # rows 0 and 1 have copies: ties at distance 0
        half = min(len(centres), 500)
        q = np.concatenate([centres[:half], points[:min(len(points), 1000 - half)]])
        if obj == 0:                                                             # few distinct queries, centres and points alternating, then copies
            pick = np.concatenate([centres[:few // 2], points[:few - few // 2]])
            q = np.concatenate([pick, pick[rng.integers(0, few, len(q) - few)]])
        partial.append(rng.permutation(q))
        coarse.append(c)
    return _frozen(np.stack(partial).astype(F32), np.stack(coarse).astype(F32))


def tie_census(partial, coarse, k):
    """By float64 computation, over the distinct queries of one object: (queries with >= 2 equal squared distances among their k nearest, those where
    two of the equal ones have coarse indices congruent mod 64, those where two have not)."""
    c = coarse.astype(np.float64)
    any_tie = in_lane = cross_lane = 0
    for q in np.unique(partial, axis=0).astype(np.float64):
        d = c - q
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        top = np.argsort(d2, kind="stable")[:k]
        t = a = x = False
        for v in np.unique(d2[top]):
            lanes = top[d2[top] == v] % 64
            if len(lanes) >= 2:
                t = True
                a |= len(set(lanes.tolist())) < len(lanes)
                x |= len(set(lanes.tolist())) > 1
        any_tie, in_lane, cross_lane = any_tie + t, in_lane + a, cross_lane + x
    return any_tie, in_lane, cross_lane


@functools.lru_cache(maxsize=None)
def tie_want(name, k):
    partial, coarse = tie_case(name)
    return _frozen(*oracle_surface_batch(partial, coarse, k, TIE_SP))


LOW_WORD_K = (1, 2, 3, 5, 8, 15, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def low_word_case():
    """(partial (2, 8, 3), coarse (2, 100, 3)).  Coarse rows (1, i * 2^-14, 0), i = 0 .. 15: seen from the z axis their float64 squared distances
    1 + z^2 + i^2 * 2^-28 are exact, agree in the high 32 bits and differ in the low 32 -- the second wave-wide minimum of k_surface_knn decides, not the
    index.  Object 0 also holds the mirrored rows (-1, ...): exact ties on top.  Shuffled among rows that are farther away."""
    partial, coarse = [], []
    i = np.arange(16)
    close = np.stack([np.ones(16), i * 2.0 ** -14, np.zeros(16)], axis=1)
    q = np.array([[0, 0, 0], [0, 0, 0.125], [0, 0, -0.25], [0, 0, 0.5]])
    for obj in range(2):
        rng = np.random.default_rng(41 + obj)
        rows = np.concatenate([close, close * [-1, 1, 1]]) if obj == 0 else close
        far = rng.normal(size=(100 - len(rows), 3)) * 0.3 + [0, 4, 0]
        coarse.append(rng.permutation(np.concatenate([rows, far])))
        partial.append(rng.permutation(np.concatenate([q, q])))
    return _frozen(np.stack(partial).astype(F32), np.stack(coarse).astype(F32))


@functools.lru_cache(maxsize=None)
def low_word_want(k):
    return _frozen(*oracle_surface_batch(*low_word_case(), k, 64))


# ---------------------------------------------------------------------------------------------------------- surface selection: set order, tiling
SET_SIZES = (1, 4, 5, 18, 19, 76, 77, 306, 307, 1024)          # either side of every table switch of k_surface_finish, and the ends
SET_VARIANTS = ("spread", "mod8", "mod32", "mod128")           # which coarse indices are selected: collisions in the 8, 32 and 128 slot tables
SP_KINDS = ("one", "below", "equal", "ragged", "default")


def surface_pts_of(count, kind):
    """surface_pts = 1; below n_selected; equal to it; not a multiple of it (n_selected > 1); the pipeline's 1024."""
    return {"one": 1, "below": max(count - 1, 1), "equal": count, "ragged": count + count // 2 + 1, "default": 1024}[kind]


@functools.lru_cache(maxsize=None)
def set_case(count):
    """(partial (4, n, 3), coarse (4, 1024, 3), selected index sets): partial rows are exact copies of `count` distinct coarse rows (some repeated),
    so with k = 1 every query selects the row it copies and n_selected == count.  Insert order into the set == lexicographic order of the rows."""
    rng = np.random.default_rng(300 + count)
    n = min(1024, count + 7)
    coarse = rng.normal(size=(len(SET_VARIANTS), 1024, 3)).astype(F32)
    partial, chosen = [], []
    for v, mod in enumerate((None, 8, 32, 128)):
        if mod is None:
            idx = rng.choice(1024, count, replace=False)
        else:
            cls = rng.permutation(np.arange(int(rng.integers(mod)), 1024, mod))
            rest = rng.permutation(np.setdiff1d(np.arange(1024), cls))
            idx = np.concatenate([cls[:count], rest[:max(count - len(cls), 0)]])
        rows = coarse[v][idx]
        partial.append(rng.permutation(np.concatenate([rows, rows[rng.integers(0, count, n - count)]])))
        chosen.append(np.sort(idx))
    return _frozen(np.stack(partial), coarse) + (chosen,)


@functools.lru_cache(maxsize=None)
def set_want(count, kind):
    partial, coarse, _ = set_case(count)
    return _frozen(*oracle_surface_batch(partial, coarse, 1, surface_pts_of(count, kind)))


UNIQUE_K = 5


@functools.lru_cache(maxsize=None)
def unique_edge_case():
    """(partial (3, 24, 3), coarse (3, 1024, 3)).  Object 0: x is +0.0 or -0.0 and y decides the order: 12 distinct rows, 4 of them with both zeros, 8 copied bit for
    bit; object 1: the same with the zeros in y, one x for all rows and z deciding; object 2: all rows equal.  np.unique compares field by field as floats, -0.0 ==
    0.0: an order that looks at the sign of a zero visits the queries in another order, and the set order of the selection follows the visits."""
    rng = np.random.default_rng(17)
    coarse = (rng.normal(size=(3, 1024, 3)) * 0.5).astype(F32)
    sign = np.where(np.arange(12) % 2 == 1, F32(-0.0), F32(0.0)).astype(F32)
    a = np.stack([sign, rng.permutation(12).astype(F32) * F32(0.1) - F32(0.5), rng.normal(size=12).astype(F32) * F32(0.3)], axis=1)
    a = np.concatenate([a, a[:4] * np.array([-1, 1, 1], F32), a[4:]])           # 4 rows with the other zero as well (x: 0.0 <-> -0.0), 8 exact copies
    b = np.stack([np.full(12, 0.125), sign, rng.normal(size=12) * 0.3], axis=1).astype(F32)     # x ties everywhere: z decides, across the zeros in y
    b = np.concatenate([b, b[:4] * np.array([1, -1, 1], F32), b[4:]])
    c = np.tile(np.array([[0.125, -0.0, 0.3]], F32), (24, 1))
    partial = np.stack([rng.permutation(a), rng.permutation(b), c]).astype(F32)
    return _frozen(partial, coarse)


@functools.lru_cache(maxsize=None)
def unique_edge_want():
    return _frozen(*oracle_surface_batch(*unique_edge_case(), UNIQUE_K, 64))


# ---------------------------------------------------------------------------------------------------------- largest cluster
def _blobs(sizes, rng, first_index_order):
    """Tight blobs 10 apart along x (each one component at eps = 0.4), stored so that the smallest index of blob first_index_order[i] is i; the other
    rows in shuffled order."""
    pts = np.concatenate([rng.normal(size=(s, 3)) * 0.03 + np.array([10.0 * i, 0, 0]) for i, s in enumerate(sizes)]).astype(F32)
    comp = np.repeat(np.arange(len(sizes)), sizes)
    head = [int(np.nonzero(comp == c)[0][0]) for c in first_index_order]
    rest = rng.permutation(np.setdiff1d(np.arange(len(pts)), head))
    order = np.concatenate([head, rest]).astype(np.int64)
    return pts[order], comp[order]


def _tiled(base, n):
    return np.tile(base, (-(-n // len(base)), 1))[:n]


@functools.lru_cache(maxsize=None)
def cluster_cases():
    """name -> (cloud (n, 3) float32, eps, min_points to run, period hint or None).  Every case has a cluster for every listed min_points."""
    rng = np.random.default_rng(23)
    cases = {}
    half, up = 0.5, float(np.nextafter(0.5, np.inf))
    # spacing exactly eps: d^2 == eps^2 bit for bit in float64 -> no edge (strict <); one float64 step more -> every lattice edge
    lat = rng.permutation(_lattice((6, 6, 6)) * F32(0.5))
    cases["lattice_pure_eps_exact"] = (lat, half, (0, 1), None)                  # singletons: the first label, point 0, wins
    cases["lattice_pure_eps_next"] = (lat, up, (0, 1, 2), None)
    lat_pair = np.concatenate([lat[:100], lat[7:8] + np.array([[0.25, 0, 0]], F32), lat[100:]])   # one row between two lattice rows: the only edges
    cases["lattice_pair_eps_exact"] = (lat_pair, half, (1, 2), None)
    cases["lattice_pair_eps_next"] = (lat_pair, up, (1, 2), None)
    pyth = np.array([[3 * i, 4 * i, 12 * j] for i in range(12) for j in range(3)], F32)     # neighbours along (3, 4, 0): d^2 == 25 == 5.0^2
    pyth = rng.permutation(np.concatenate([pyth, [[1.5, 2.0, 0.0]]]).astype(F32))
    cases["pythagoras_eps_exact"] = (pyth, 5.0, (1, 2), None)
    cases["pythagoras_eps_next"] = (pyth, float(np.nextafter(5.0, np.inf)), (1, 2), None)
    # equal largest components: a small one holds index 0, the large ones first appear in the opposite of cloud order
    cases["equal_two"] = (_blobs((40, 40, 9), rng, (2, 1, 0))[0], 0.4, (1, 2), None)
    cases["equal_three"] = (_blobs((30, 30, 30, 7), rng, (3, 2, 0, 1))[0], 0.4, (1, 2), None)
    path = np.zeros((1024, 3), F32)
    path[:, 0] = np.arange(1024, dtype=F32) * F32(0.3)                             # neighbours 0.3 apart, next ones 0.6: a path at eps = 0.4
    cases["path_1024_shuffled"] = (rng.permutation(path), 0.4, (2,), None)
    cases["one_component"] = ((rng.normal(size=(300, 3)) * 0.1).astype(F32), 0.4, (1, 2), None)
    cases["n1"] = (np.array([[0.3, -0.2, 0.1]], F32), 0.4, (0, 1), None)
    cases["n2_close"] = (np.array([[0, 0, 0], [0.1, 0, 0]], F32), 0.4, (0, 1, 2), None)
    cases["n2_far"] = (np.array([[5, 0, 0], [0, 0, 0]], F32), 0.4, (0, 1), None)
    iso = rng.permutation(_lattice((2, 3, 2)) * F32(7.0))
    cases["isolated"] = (iso, 0.4, (0, 1), None)
    cases["isolated_plus_pair"] = (np.concatenate([iso[:5], iso[2:3] + F32(0.1), iso[5:]]), 0.4, (0, 1, 2), None)
    # periodic clouds: the base tiled so that the last copy is partial
    pl = np.concatenate([rng.permutation(_lattice((4, 4, 4)) * F32(0.5))[:63], [[0.25, 0.5, 0.5]]]).astype(F32)       # U = 64, even
    cases["periodic_lattice_eps_exact"] = (_tiled(pl, 149), half, (1, 2), 64)
    cases["periodic_lattice_eps_next"] = (_tiled(pl, 149), up, (1, 2), 64)
    cases["periodic_equal_three"] = (_tiled(_blobs((20, 20, 20, 5), rng, (3, 1, 2, 0))[0], 150), 0.4, (1, 2), 65)   # U = 65, odd
    cases["periodic_pair_close"] = (_tiled(np.array([[0, 0, 0], [0.1, 0, 0]], F32), 5), 0.4, (0, 1, 2), 2)          # the only pair sits at s == U/2
    cases["periodic_pair_far"] = (_tiled(np.array([[5, 0, 0], [0, 0, 0]], F32), 5), 0.4, (0, 1, 2), 2)
    ring4 = np.array([[0, 0, 0], [0.3, 0, 0], [0.3, 0.3, 0], [0, 0.3, 0]], F32)                                      # U = 4: s == 2 are the diagonals (no edge)
    cases["periodic_ring4"] = (_tiled(ring4, 7), 0.4, (1, 2), 4)
    cases["periodic_opposite4"] = (_tiled(np.array([[0, 0, 0], [9, 0, 0], [0.3, 0, 0], [9.3, 0, 0]], F32), 7), 0.4, (1, 2), 4)   # edges ONLY at s == U/2
    cases["periodic_u1"] = (_tiled(np.array([[1, 2, 3]], F32), 4), 0.4, (0, 1, 2), 1)
    cases["periodic_isolated"] = (_tiled(iso[:10], 25), 0.4, (0, 1, 2), 10)         # originals 0 .. 4 have two copies, 5 .. 9 one
    ppath = np.zeros((400, 3), F32)
    ppath[:, 1] = np.arange(400, dtype=F32) * F32(0.3)
    ppath[200:, 1] += F32(5.0)                                                     # two paths of 200 rows; the first 224 stored rows get a third copy
    cases["periodic_path_1024"] = (_tiled(rng.permutation(ppath), 1024), 0.4, (2,), 400)
    cases["periodic_equal_1024"] = (_tiled(_blobs((100, 100, 100, 33), rng, (3, 2, 0, 1))[0], 1024), 0.4, (2,), 333)
    for name, (cloud, *_rest) in cases.items():
        assert cloud.dtype == F32 and (len(cloud) <= 300 or len(cloud) == 1024), name
        cloud.setflags(write=False)
    assert sum(len(c[0]) == 1024 for c in cases.values()) <= 6
    return cases


@functools.lru_cache(maxsize=None)
def cluster_want(name, min_points, total_pts=1024):
    cloud, eps, _, _ = cluster_cases()[name]
    pts, size = opp.largest_cluster(cloud, eps=eps, min_points=min_points, total_pts=total_pts)
    return _frozen(pts), size


@functools.lru_cache(maxsize=None)
def noise_batch():
    """(clouds (3, 10, 3), eps, min_points): objects 0 and 2 are all noise (isolated rows, min_points 2), object 1 is one component."""
    rng = np.random.default_rng(29)
    iso = rng.permutation(_lattice((2, 5, 1)) * F32(3.0))
    blob = (rng.normal(size=(10, 3)) * 0.05).astype(F32)
    return _frozen(np.stack([iso, blob, iso[::-1] + F32(1.0)]).astype(F32)), 0.4, 2


# ---------------------------------------------------------------------------------------------------------- duplicate rows
DEDUP_SIZES = (1, 2, 255, 256, 257, 512, 513, 4096)             # the table has 1024 slots up to n = 512 and 2048 from 513
DEDUP_FAMILIES = ("all_equal", "all_distinct", "far_duplicates", "signed_zeros", "nan_rows", "dropped_rows")


def _distinct_rows(n, rng):
    rows = np.empty((n, 4), F32)
    rows[:, 0] = rng.integers(0, 3, n)
    rows[:, 1:] = rng.normal(size=(n, 3))
    rows[:, 3] = np.arange(n, dtype=F32) + F32(0.5)              # distinct whatever the other columns hold
    return rows


@functools.lru_cache(maxsize=None)
def dedup_case(family, n):
    rng = np.random.default_rng(400 + n + 7 * DEDUP_FAMILIES.index(family))
    if family == "all_equal":
        rows = np.tile(np.array([[1, 0.25, -3.5, 2.0]], F32), (n, 1))
    elif family == "all_distinct":
        rows = rng.permutation(_distinct_rows(n, rng))
    elif family == "far_duplicates":                              # row i + ceil(n / 2) is a copy of row i
        first = rng.permutation(_distinct_rows(-(-n // 2), rng))
        rows = np.concatenate([first, first])[:n]
    elif family == "signed_zeros":                                # every sign pattern of the zeros of two rows: two survivors
        z = np.array([[F32(-0.0) if (p >> c) & 1 else F32(0.0) for c in range(4)] for p in range(16)], F32)
        w = z.copy()
        w[:, 0], w[:, 2] = 1.0, 2.0
        rows = np.concatenate([z, w])[rng.integers(0, 32, n)]
    elif family == "nan_rows":                                    # NaN equals nothing: copies of a NaN row all survive; the rest behave as ever
        pool = _distinct_rows(6, rng)
        pool[1, 2] = pool[2, 3] = pool[3, 1] = pool[4, 0] = np.nan
        pool[4, 1:] = pool[0, 1:]
        rows = pool[rng.integers(0, 6, n)]
    else:                                                          # rows that arrive dropped (scene id < 0) in front of live rows with the same x, y, z
        pool = _distinct_rows(5, rng)
        pool = np.concatenate([pool, pool])
        pool[:5, 0] = [-1.0, -1.0, -2.0, -0.5, -1.0]
        rows = pool[np.concatenate([np.arange(min(n, 5)), rng.integers(0, 10, max(n - 5, 0))])]
    return _frozen(np.ascontiguousarray(rows, F32))


def dedup_expect(rows):
    """Row i gets scene id -1 iff some j < i holds a numpy-equal row that did not arrive dropped (scene id < 0); nothing else changes."""
    rows = np.asarray(rows)
    live = ~(rows[:, 0] < 0)
    flag = np.zeros(len(rows), bool)
    for i in range(1, len(rows)):
        if live[i]:
            flag[i] = bool(((rows[:i] == rows[i]).all(axis=1) & live[:i]).any())
    out = rows.copy()
    out[flag, 0] = -1.0
    return out, flag


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------- points near a set
NB_TILE, NS_TILE = 128, 256                                     # reference rows per tile of the boxed and of the workgroup-tiled kernel
NEAR_REF_SIZES = (0, 1, 127, 128, 129, 255, 256, 257)
NEAR_QUERY_SIZES = (0, 1, 255, 257)
F01 = F32(0.1)


def near_want(query, ref, thresh):
    """near[i] = sqrt(min_j d2(q_i, r_j)) < thresh in float64; with 4 columns j runs over the reference rows of query i's scene (column 0) that are
    not dropped (scene id < 0): a query whose scene has none is near nothing."""
    q, r = np.asarray(query, np.float64), np.asarray(ref, np.float64)
    D = q.shape[1]
    out = np.zeros(len(q), bool)
    if D == 4:
        r = r[r[:, 0] >= 0]
    groups = [(np.ones(len(q), bool), r)] if D == 3 else [(q[:, 0] == s, r[r[:, 0] == s]) for s in np.unique(q[:, 0])]
    for qm, rs in groups:
        if not len(rs) or not qm.any():
            continue
        qi = np.nonzero(qm)[0]
        for s in range(0, len(qi), 512):
            d = q[qi[s:s + 512], None, D - 3:] - rs[None, :, D - 3:]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            out[qi[s:s + 512]] = np.sqrt(d2.min(axis=1)) < thresh
    return out


def _with_scene(xyz, scene):
    return np.concatenate([np.full((len(xyz), 1), scene, F32), np.asarray(xyz, F32)], axis=1)


def rows_of(case, row_dim):
    q, r, thresh = case
    return (q, r, thresh) if row_dim == 4 else (np.ascontiguousarray(q[:, 1:]), np.ascontiguousarray(r[:, 1:]), thresh)


@functools.lru_cache(maxsize=None)
def near_threshold_cases():
    """name -> (query (nq, 4), ref (nr, 4), thresh), one scene.  `pythagoras_*`: reference rows at the origin and elsewhere, queries at (3, 4, 0) and
    its permutations -- distance exactly 5.0 -- and at the float32 neighbours of 3 on either side; `tenth`: queries on each axis at float32(0.1)
    (above the double 0.1) and its float32 neighbours; `zero`: thresh 0 with queries ON reference rows."""
    below3, above3 = np.nextafter(F32(3), F32(0)), np.nextafter(F32(3), F32(9))
    ref = np.array([[0, 0, 0], [100, 0, 0], [0, -50, 7]], F32)
    q = [[3, 4, 0], [0, 3, 4], [4, 0, 3], [-3, -4, 0], [below3, 4, 0], [above3, 4, 0], [0, below3, -4], [0, above3, -4], [103, 0, 4], [100 + 3, 0, -4],
         [3, -50, 11], [0, 0, 5], [0, 0, 0]]
    q, ref4 = _with_scene(np.array(q, F32), 0), _with_scene(ref, 0)
    lo, hi = np.nextafter(F01, F32(0)), np.nextafter(F01, F32(1))
    tenth = np.array([[v if a == c else 0 for c in range(3)] for a in range(3) for v in (lo, F01, hi, -lo, -F01, -hi)], F32)
    on = np.concatenate([ref, ref + F32(1e-3)])
    cases = {
        "pythagoras_5": (q, ref4, 5.0),
        "pythagoras_5_next": (q, ref4, float(np.nextafter(5.0, np.inf))),
        "tenth": (_with_scene(tenth, 0), ref4, 0.1),
        "zero": (_with_scene(on, 0), ref4, 0.0),
    }
    for c in cases.values():
        _frozen(c[0], c[1])
    return cases


@functools.lru_cache(maxsize=None)
def near_size_case(n_ref, n_query):
    """The reference rows lie far away except the LAST one -- the only row of the last tile, or its last row -- which sits among the queries."""
    rng = np.random.default_rng(500 + 1000 * n_ref + n_query)
    ref = (rng.normal(size=(n_ref, 3)) * 0.5 + 50.0).astype(F32)
    if n_ref:
        ref[-1] = [0.1, -0.2, 0.3]
    q = (rng.normal(size=(n_query, 3)) * 0.12 + np.array([0.1, -0.2, 0.3])).astype(F32)
    return _frozen(_with_scene(q, 1), _with_scene(ref, 1)) + (0.1,)


@functools.lru_cache(maxsize=None)
def near_dropped_input(tile):
    """(ref rows (4 * tile + 9, 4) BEFORE sv_dedup_rows, query rows).  After it, with T = tile: rows [0, T) cluster A, live; [T, 2T) copies of them: a
    tile dropped whole; row 2T a copy of row 0 and [2T + 1, 3T) cluster B: only the first row dropped; [3T, 4T - 1) copies of earlier rows and rows
    that ARRIVE dropped at a place D where nothing is live, row 4T - 1 the single row C: only the last row live; then 9 rows, copies and new ones.
    Queries of scene 0 and of scene -1 at A, B, C and D; nothing at D may be near."""
    rng = np.random.default_rng(600 + tile)
    T = tile
    at = {"A": np.array([0, 0, 0]), "B": np.array([3, 0, 0]), "C": np.array([0, 4, 0]), "D": np.array([0, 0, 5]), "E": np.array([6, 6, 0])}
    cloud = lambda key, n: _with_scene((rng.normal(size=(n, 3)) * 0.15 + at[key]).astype(F32), 0)
    A, B, C, E = cloud("A", T), cloud("B", T - 1), cloud("C", 1), cloud("E", 4)
    D = cloud("D", T // 2)
    D[:, 0] = -1.0
    copies = np.concatenate([A, B])[rng.integers(0, 2 * T - 1, T - 1 - len(D))]
    ref = np.concatenate([A, rng.permutation(A), A[:1], B, rng.permutation(np.concatenate([copies, D])), C, E, A[:5]])
    q = np.concatenate([cloud(key, 40) for key in "ABCDE"] + [C + np.array([0, 0.01, 0.01, 0.01], F32)])
    gone = q.copy()
    gone[:, 0] = -1.0
    return _frozen(np.ascontiguousarray(ref), np.ascontiguousarray(np.concatenate([q, gone])))


@functools.lru_cache(maxsize=None)
def near_seam_case(sort_rows):
    """Reference rows of scenes 0 (100 rows), 1 (10), 2 (100) and 4 (60), all in the same place, so that the scene id alone decides: in scene order the
    first 128 and the first 256 rows span three scenes, and the rows of scenes 2 and 4 share a tile that has no row of scene 3.  Queries of scenes
    0 .. 5 (3 and 5 have no reference rows) in that place.  sort_rows False: the same rows in shuffled order (every tile box spans all scenes)."""
    rng = np.random.default_rng(700)
    ref = np.concatenate([_with_scene((rng.normal(size=(n, 3)) * 0.4).astype(F32), s) for s, n in ((0, 100), (1, 10), (2, 100), (4, 60))])
    ref = ref[np.lexsort(ref.T[::-1])] if sort_rows else rng.permutation(ref)
    q = rng.permutation(np.concatenate([_with_scene((rng.normal(size=(60, 3)) * 0.45).astype(F32), s) for s in range(6)]))
    return _frozen(np.ascontiguousarray(q), np.ascontiguousarray(ref)) + (0.1,)


@functools.lru_cache(maxsize=None)
def near_dense_case(sort_rows, offset=0.0):
    """Two scenes of clustered points, 1000 reference rows and 2000 queries; offset 1.0e4 moves every coordinate to where floats are 2^-10 apart
    (the float pre-screen of the boxed kernel then works with a hundredth of the threshold as its unit)."""
    rng = np.random.default_rng(800)
    centres = rng.normal(size=(12, 3)) * 2.0
    ref = centres[rng.integers(0, 12, 1000)] + rng.normal(size=(1000, 3)) * 0.25 + offset
    q = centres[rng.integers(0, 12, 2000)] + rng.normal(size=(2000, 3)) * 0.35 + offset
    ref = np.concatenate([rng.integers(0, 2, (1000, 1)), ref], axis=1).astype(F32)
    q = np.concatenate([rng.integers(0, 2, (2000, 1)), q], axis=1).astype(F32)
    if sort_rows:
        ref = ref[np.lexsort(ref.T[::-1])]
    return _frozen(np.ascontiguousarray(q), np.ascontiguousarray(ref)) + (0.1,)
