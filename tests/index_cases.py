"""Coordinate sets that sit on the structural boundaries of the coordinate index (csrc/common.h, coord_index.hip, rulebook.hip), the oracle tables
the builders are held to on them, and the one comparison every test of tests/test_index_edges.py goes through.  Plain module, no fixtures."""
import functools

import numpy as np

from oracle import spconv as osp

# cells per structural unit of the index: bitmap word, chunk (32 words), wave step of k_index_prefix (64 chunks), chain block (CH_BLOCK = 256
# chunks), scan tile (SCAN_TILE = 4096 chunks)
BLOCKS = (32, 1024, 65536, 262144, 4194304)

GRIDS = {  # name -> (batch, (Z, Y, X))
    "A": (1, (5, 7, 33)),          # odd X just over a word: every word spans rows
    "B": (3, (4, 8, 32)),          # one batch item == one chunk
    "C": (2, (9, 20, 5)),          # X = 5: every word spans rows and z-slices
    "D": (2, (9, 64, 128)),        # 147 456 cells: crosses the 64-chunk wave step
    "E": (2, (21, 128, 112)),      # 602 112 cells: 3 chain blocks
    "F": (2, (41, 320, 352)),      # 9 236 480 cells: 3 scan tiles, 36 chain blocks
}
N_RANDOM = 2000

# the convolutions of tests/test_spconv.py::test_hip_network_index_equals_the_layer_by_layer_build: (key, subm, ksize, stride, padding, dilation, cin, cout)
NETWORK_SPECS = [
    ("subm1", True, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 16, 16), ("subm1", True, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 16, 16),
    ("sp2", False, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), 16, 32), ("subm2", True, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 32, 32),
    ("sp3", False, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), 32, 64), ("subm3", True, (3, 1, 3), (1, 1, 1), (1, 0, 1), (1, 1, 1), 64, 64),
    ("sp4", False, (3, 3, 3), (2, 2, 2), (0, 1, 1), (1, 1, 1), 64, 64), ("subm4", True, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 64, 64),
    ("down", False, (3, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), 64, 128)]


def keys_of(coords, shape):
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    return ((c[:, 0] * shape[0] + c[:, 1]) * shape[1] + c[:, 2]) * shape[2] + c[:, 3]


def coords_of(keys, shape):
    k = np.asarray(keys, np.int64)
    x, t = k % shape[2], k // shape[2]
    y, t = t % shape[1], t // shape[1]
    return np.stack([t // shape[0], t % shape[0], y, x], axis=1)


def empty_item(batch, moved=False):
    """The batch item edge_coords leaves without a single site (None below 3 items): a middle one, so that key 0 and the last item's corner stay;
    the first one in the moved set, so that a rebuild meets occupied cells where the set before had none and the other way round."""
    if batch < 3:
        return None
    return 0 if moved else batch - 2


def edge_coords(batch, shape, rng, n_random, moved=False):
    """Unique (n, 4) int32 [b, z, y, x] on the grid, shuffled: the first and last key; the keys m*B - 1, m*B, m*B + 1 around the first, a middle and
    the last multiple of every block size in BLOCKS; two full words (one the grid's last whole word); one full chunk; the 8 corners of every batch
    item; a full edge line along each axis; a dense 6 x 6 x 6 cube in a corner of the last batch item; n_random uniform cells -- and one batch item
    left empty when there are 3 or more (it is exempt from all of the above).  moved: another set on the same grid -- another chunk, word and empty
    item, the lines on other edges and the cube in the opposite corner."""
    Z, Y, X = (int(v) for v in shape)
    per = Z * Y * X
    ncells = batch * per
    hole = empty_item(batch, moved)

    def run(preferred, size):
        """`size` consecutive keys from a multiple of `size` that stay clear of the empty item: the preferred one, else the nearest below, else above"""
        n_runs = ncells // size
        for i in list(range(min(preferred, n_runs - 1), -1, -1)) + list(range(preferred + 1, n_runs)):
            if hole is None or (i * size + size - 1) // per < hole or (i * size) // per > hole:
                return np.arange(i * size, (i + 1) * size, dtype=np.int64)
        return np.zeros(0, np.int64)

    keys = [np.array([0, ncells - 1], np.int64)]
    for B in BLOCKS:
        last = (ncells - 1) // B
        for m in sorted({1, (1 + last) // 2, last}):
            if 1 <= m <= last:
                keys.append(np.array([m * B - 1, m * B, m * B + 1], np.int64))
    n_words, n_chunks = ncells // 32, ncells // 1024
    if n_words:
        keys += [run(n_words - 1, 32), run(n_words // (3 if moved else 2), 32)]
    if n_chunks:
        keys.append(run(n_chunks - 1 if moved else n_chunks // 2, 1024))
    first = 0 if hole != 0 else 1                      # first and last item that hold sites
    last_b = batch - 1
    pts = [[b, z, y, x] for b in range(batch) for z in (0, Z - 1) for y in (0, Y - 1) for x in (0, X - 1)]
    if not moved:
        pts += [[first, 0, 0, x] for x in range(X)] + [[last_b, Z - 1, y, X - 1] for y in range(Y)] + [[first, z, Y - 1, 0] for z in range(Z)]
        cube = [range(max(Z - 6, 0), Z), range(max(Y - 6, 0), Y), range(max(X - 6, 0), X)]
    else:
        pts += [[last_b, Z - 1, Y - 1, x] for x in range(X)] + [[first, 0, y, 0] for y in range(Y)] + [[last_b, z, 0, X - 1] for z in range(Z)]
        cube = [range(0, min(6, Z)), range(0, min(6, Y)), range(0, min(6, X))]
    pts += [[last_b, z, y, x] for z in cube[0] for y in cube[1] for x in cube[2]]
    keys.append(keys_of(np.array(pts, np.int64), shape))
    keys.append(rng.integers(0, ncells, size=int(n_random), dtype=np.int64))
    k = np.unique(np.concatenate(keys))
    k = k[(k >= 0) & (k < ncells)]
    if hole is not None:
        k = k[k // per != hole]
    return coords_of(k[rng.permutation(len(k))], shape).astype(np.int32)


def straddled(coords, batch, shape, adjacent=False):
    """{block size: do occupied cells exist on both sides of some multiple of it}.  adjacent: the two cells next to one multiple, m*B - 1 and m*B,
    are both occupied (what edge_coords builds wherever the boundary does not border the empty batch item)."""
    k = np.unique(keys_of(coords, shape))
    out = {}
    for B in BLOCKS:
        if not len(k):
            out[B] = False
        elif adjacent:
            below = k[k % B == B - 1]
            out[B] = bool(np.isin(below + 1, k).any())
        else:
            out[B] = bool(k[0] // B != k[-1] // B)
    return out


def preimage_coords(batch, in_shape, ksize, stride, padding, rng, n_random, dilation=1, moved=False):
    """Input coordinates of a strided convolution whose candidate outputs hold the edge_coords of the OUTPUT grid (the strided builders index that
    grid): in = out * stride - pad + k * dilation for every kernel offset k, kept where inside the input grid, unique, shuffled."""
    s3, p3, d3 = osp._triple(stride), osp._triple(padding), osp._triple(dilation)
    oshape = osp.out_shape(in_shape, ksize, stride, padding, dilation)
    out = edge_coords(batch, oshape, rng, n_random, moved).astype(np.int64)
    parts = []
    for off in osp._offsets(ksize):
        c = [out[:, 1 + a] * s3[a] - p3[a] + off[a] * d3[a] for a in range(3)]
        ok = np.ones(len(out), bool)
        for a in range(3):
            ok &= (c[a] >= 0) & (c[a] < in_shape[a])
        parts.append(np.stack([out[:, 0]] + c, axis=1)[ok])
    c = np.unique(np.concatenate(parts), axis=0)
    return c[rng.permutation(len(c))].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------- oracle tables
def twin_and_masks(nbr):
    """What the planned conv kernels read: the row-major twin (n, 32) of a k-major table (K <= 27, n) -- the table transposed, padded with -1 -- and
    the neighbour masks (n): bit k set iff nbr[k][i] >= 0."""
    K, n = nbr.shape
    assert K <= 27
    rows = np.full((n, 32), -1, np.int32)
    rows[:, :K] = nbr.T
    masks = np.zeros(n, np.int64)
    for k in range(K):
        masks |= (nbr[k] >= 0).astype(np.int64) << k
    return rows, masks.astype(np.int32)


def subm_tables(coords, shape, ksize, dilation=1):
    nbr = osp.rulebook_subm(coords, shape, ksize, dilation)
    rows, masks = twin_and_masks(nbr)
    return {"n_in": len(coords), "nbr_out": nbr, "nbr_bwd": np.ascontiguousarray(nbr[::-1]), "rows_out": rows, "masks_out": masks}


def sparse_tables(coords, shape, ksize, stride, padding, dilation=1):
    oc, nbr_out, nbr_in, oshape = osp.rulebook_sparse(coords, shape, ksize, stride, padding, dilation)
    t = {"n_in": len(coords), "out_indices": oc, "out_shape": tuple(int(v) for v in oshape), "n_out": len(oc), "nbr_in": nbr_in, "nbr_out": nbr_out,
         "pair_counts": osp.pair_counts(nbr_out)}
    t["rows_out"], t["masks_out"] = twin_and_masks(nbr_out)
    t["rows_in"], t["masks_in"] = twin_and_masks(nbr_in)
    return t


def network_tables(coords, shape, specs):
    """The oracle chained level by level over NETWORK_SPECS-style rows: the output sites of strided level l are the input of level l + 1.
    -> ({key: tables}, number of leading specs that have an output grid).  A level whose kernel no longer fits its padded input has none (a zero in
    oracle.spconv.out_shape; spconv refuses it): the walk ends in front of it."""
    want, idx, sh = {}, coords, tuple(int(v) for v in shape)
    for i, (key, subm, ksize, stride, padding, dilation, *_rest) in enumerate(specs):
        if key in want:
            continue
        if subm:
            want[key] = subm_tables(idx, sh, ksize, dilation)
        else:
            if min(osp.out_shape(sh, ksize, stride, padding, dilation)) <= 0:
                return want, i
            want[key] = t = sparse_tables(idx, sh, ksize, stride, padding, dilation)
            idx, sh = t["out_indices"], t["out_shape"]
    return want, len(specs)


TWINS = ("rows_out", "masks_out", "rows_in", "masks_in")


def assert_same_tables(got, want, tag="", optional=()):
    """Every entry of `want` (oracle tables) against `got`, bit for bit: sizes and shapes as values, tables as integer arrays of the same shape.
    Only names in `optional` may be None in `got` (a route that does not produce the twins)."""
    for name, w in want.items():
        g = got.get(name)
        if g is None:
            assert name in optional, (tag, name, "missing")
            continue
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            assert g.dtype.kind == "i" and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.shape)
            if not np.array_equal(g, w):
                bad = np.argwhere(g != w)
                raise AssertionError((tag, name, f"{len(bad)} of {w.size} entries differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"))
        else:
            assert (tuple(g) if isinstance(w, tuple) else g) == w, (tag, name, g, w)


# ---------------------------------------------------------------------------------------------------------- the cases, computed once
def _seed(grid, moved, strided=False):
    return sum(ord(ch) for ch in grid) * 2 + int(moved) + (1000 if strided else 0)


@functools.lru_cache(maxsize=None)
def case_coords(grid, moved=False):
    batch, shape = GRIDS[grid]
    c = edge_coords(batch, shape, np.random.default_rng(_seed(grid, moved)), N_RANDOM, moved)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case_out_edges(grid, geom, moved=False):
    """The edge_coords on the OUTPUT grid that case_preimage is the preimage of (the same generator state)."""
    batch, shape = GRIDS[grid]
    return edge_coords(batch, osp.out_shape(shape, *geom), np.random.default_rng(_seed(grid, moved, True)), N_RANDOM, moved)


@functools.lru_cache(maxsize=None)
def case_preimage(grid, geom, moved=False):
    batch, shape = GRIDS[grid]
    ksize, stride, padding = geom
    c = preimage_coords(batch, shape, ksize, stride, padding, np.random.default_rng(_seed(grid, moved, True)), N_RANDOM, moved=moved)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case_subm_tables(grid, ksize, dilation, moved=False):
    return subm_tables(case_coords(grid, moved), GRIDS[grid][1], ksize, dilation)


@functools.lru_cache(maxsize=None)
def case_sparse_tables(grid, geom, moved=False):
    return sparse_tables(case_preimage(grid, geom, moved), GRIDS[grid][1], *geom)


LEVEL1_GEOM = (3, 2, 1)                 # NETWORK_SPECS' first strided level ("sp2")


def case_network_coords(grid, moved=False, level1=False):
    """Input of the network index: edge_coords of the grid, or (level1) the preimage of edge_coords laid on the first strided level's OUTPUT grid --
    the grid that the chain's count and emit kernels index, with its own word, chunk and chain-block boundaries."""
    return case_preimage(grid, LEVEL1_GEOM, moved) if level1 else case_coords(grid, moved)


@functools.lru_cache(maxsize=None)
def case_network_tables(grid, moved=False, level1=False):
    return network_tables(case_network_coords(grid, moved, level1), GRIDS[grid][1], NETWORK_SPECS)
