"""The coordinate index and every table built on it, against the oracle, on coordinate sets that sit on the index's structural boundaries
(tests/index_cases.py): word (32 cells), chunk (1024), wave step (65 536), chain block (262 144), scan tile (4 194 304), the 4 x 4 x 8 cell-map tile and
the 32-column row-major twins.  CPU: the oracle itself against a dictionary brute force at the faces and corners, the generator's promise, and the
comparison's sensitivity to seeded faults.  GPU: the submanifold builder on both routes, the strided builder, the network index and the voxeliser --
tables, twins, masks and counts bit for bit, each case built twice and then on another coordinate set over the same persistent workspace."""
import numpy as np
import pytest

import index_cases as ic
from oracle import spconv as osp
from oracle import voxelize as ov
from test_spconv import GEOMS

STRIDED_GEOMS = list(GEOMS) + [(3, (2, 1, 1), 1)]                     # GEOMS holds (3, 1, 1) already: the 3 x 3 x 3 kernel as a strided conv of stride 1
SUBM_KERNELS = [((3, 3, 3), 1), ((1, 3, 3), 1), ((3, 1, 3), 1)]         # (ksize, dilation)
VOXEL_MEAN_TOL = dict(rtol=1e-5, atol=1e-5)                           # tests/test_voxelize.py's tolerance for the HIP feature means


# ---------------------------------------------------------------------------------------------------------- CPU
def _brute_subm(coords, shape, ksize, dilation):
    k3, d3 = osp._triple(ksize), osp._triple(dilation)
    row = {tuple(int(v) for v in c): i for i, c in enumerate(coords)}
    offs = [(a, b, c) for a in range(k3[0]) for b in range(k3[1]) for c in range(k3[2])]
    nbr = np.full((len(offs), len(coords)), -1, np.int32)
    for k, off in enumerate(offs):
        d = [(off[a] - k3[a] // 2) * d3[a] for a in range(3)]
        for (b, z, y, x), i in row.items():
            nbr[k, i] = row.get((b, z + d[0], y + d[1], x + d[2]), -1)      # a cell outside the grid is in no dictionary
    return nbr


def _brute_sparse(coords, shape, ksize, stride, padding, dilation=1):
    k3, s3, p3, d3 = (osp._triple(v) for v in (ksize, stride, padding, dilation))
    oshape = tuple((shape[a] + 2 * p3[a] - d3[a] * (k3[a] - 1) - 1) // s3[a] + 1 for a in range(3))
    offs = [(a, b, c) for a in range(k3[0]) for b in range(k3[1]) for c in range(k3[2])]
    pairs = []                                                            # (k, input row, output coordinate)
    for i, c in enumerate(coords):
        b, zyx = int(c[0]), [int(v) for v in c[1:]]
        for k, off in enumerate(offs):
            t = [zyx[a] + p3[a] - off[a] * d3[a] for a in range(3)]
            if all(t[a] >= 0 and t[a] % s3[a] == 0 and t[a] // s3[a] < oshape[a] for a in range(3)):
                pairs.append((k, i, (b, t[0] // s3[0], t[1] // s3[1], t[2] // s3[2])))
    sites = sorted({o for _, _, o in pairs})                             # (b, z, y, x) ascending == ascending linear key
    rank = {o: r for r, o in enumerate(sites)}
    nbr_in = np.full((len(offs), len(coords)), -1, np.int32)
    nbr_out = np.full((len(offs), len(sites)), -1, np.int32)
    for k, i, o in pairs:
        nbr_in[k, i] = rank[o]
        assert nbr_out[k, rank[o]] == -1                                  # (k, output) fixes the input cell
        nbr_out[k, rank[o]] = i
    return np.array(sites, np.int32).reshape(-1, 4), nbr_out, nbr_in, oshape


@pytest.mark.parametrize("grid", ["A", "B", "C"])
def test_oracle_equals_dictionary_brute_force_at_edges(grid):
    """oracle.spconv.rulebook_subm / rulebook_sparse (sorted keys + searchsorted) against a dict from coordinate to row looped over the offsets, on
    edge_coords: pins the oracle at the faces, corners and across batch items before the GPU is held to it."""
    batch, shape = ic.GRIDS[grid]
    ncells = batch * shape[0] * shape[1] * shape[2]
    coords = ic.edge_coords(batch, shape, np.random.default_rng(7), ncells // 6)
    assert len(np.unique(ic.keys_of(coords, shape))) == len(coords) and coords.dtype == np.int32
    for ksize, dil in SUBM_KERNELS + [((3, 3, 3), 2)]:
        assert np.array_equal(osp.rulebook_subm(coords, shape, ksize, dil), _brute_subm(coords, shape, ksize, dil)), (ksize, dil)
    for ksize, stride, padding in STRIDED_GEOMS + [((1, 3, 3), 1, (0, 1, 1)), (3, 1, 1)]:
        oc, nbr_out, nbr_in, oshape = osp.rulebook_sparse(coords, shape, ksize, stride, padding)
        b_oc, b_out, b_in, b_shape = _brute_sparse(coords, shape, ksize, stride, padding)
        tag = (ksize, stride, padding)
        assert tuple(oshape) == b_shape, tag
        assert np.array_equal(oc, b_oc) and np.array_equal(nbr_out, b_out) and np.array_equal(nbr_in, b_in), tag


def _strided_cases():
    return [(g, geom) for g in "ABCDE" for geom in STRIDED_GEOMS] + [("F", (3, (2, 1, 1), 1))]


def test_every_gpu_case_straddles_every_boundary_below_its_size():
    """A test must not silently lose its edges: on every grid the GPU tests index -- the grids themselves, and the output grids of the strided
    cases -- occupied cells lie on both sides of a multiple of every block size smaller than the grid, in the first set and in the moved one; and the
    two cells next to one multiple, m*B - 1 and m*B, are both occupied unless every such boundary borders the batch item that is left empty."""
    def check(sites, batch, shape, moved, tag):
        per = shape[0] * shape[1] * shape[2]
        ncells = batch * per
        loose, tight = ic.straddled(sites, batch, shape), ic.straddled(sites, batch, shape, adjacent=True)
        hole = ic.empty_item(batch, moved)
        for B in ic.BLOCKS:
            if B >= ncells:
                continue
            assert loose[B], (tag, B)
            borders_hole = hole is not None and all(hole in ((m * B - 1) // per, (m * B) // per) for m in range(1, (ncells - 1) // B + 1))
            assert tight[B] or borders_hole, (tag, B, "adjacent")
        if hole is not None:
            assert not (np.asarray(sites)[:, 0] == hole).any(), (tag, "empty item")

    for moved in (False, True):
        for grid, (batch, shape) in ic.GRIDS.items():
            check(ic.case_coords(grid, moved), batch, shape, moved, (grid, moved))
        for grid, geom in _strided_cases() + [("F", ic.LEVEL1_GEOM)]:           # the last one: the network index's level-1 case on grid F
            batch, shape = ic.GRIDS[grid]
            oshape = osp.out_shape(shape, *geom)
            # the builder indexes the candidate outputs of its inputs: a superset of the edges laid on the output grid, each of which some input reaches
            edges = ic.case_out_edges(grid, geom, moved)
            k3, s3, p3 = (osp._triple(v) for v in geom)
            reached = np.zeros(len(edges), bool)
            for off in osp._offsets(k3):
                inside = np.ones(len(edges), bool)
                for a in range(3):
                    v = edges[:, 1 + a].astype(np.int64) * s3[a] - p3[a] + off[a]
                    inside &= (v >= 0) & (v < shape[a])
                reached |= inside
            assert reached.all(), (grid, geom, moved)
            k_in = ic.case_preimage(grid, geom, moved)
            assert len(np.unique(ic.keys_of(k_in, shape))) == len(k_in)
            check(edges, batch, oshape, moved, (grid, geom, moved))
    # the sizes the issue states for the large grids
    assert [b * z * y * x for b, (z, y, x) in (ic.GRIDS[g] for g in "DEF")] == [147456, 602112, 9236480]
    assert ic.straddled(ic.case_coords("F"), *ic.GRIDS["F"], adjacent=True) == {B: True for B in ic.BLOCKS}


def test_comparison_raises_on_every_seeded_fault():
    """assert_same_tables -- what every GPU test below compares with -- on oracle tables with one fault each: ranks shifted by one behind a chunk
    boundary, one output site missing (consistently: a properties-only check passes it), one mask bit cleared, one twin row not padded with -1."""
    batch, shape = ic.GRIDS["D"]
    geom = (3, 2, 1)
    want = ic.case_sparse_tables("D", geom)
    oshape = want["out_shape"]

    def copy():
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}

    ic.assert_same_tables(copy(), want)                                    # the unharmed copy passes
    okeys = ic.keys_of(want["out_indices"], oshape)
    r0 = int(np.searchsorted(okeys, 1024 * (okeys[len(okeys) // 2] // 1024)))     # first site of the chunk that holds the middle site
    assert 0 < r0 < len(okeys) and okeys[r0 - 1] // 1024 != okeys[r0] // 1024
    faults = {}
    f = copy()
    f["nbr_in"][f["nbr_in"] >= r0] += 1
    faults["ranks shifted behind a chunk boundary"] = f
    f = copy()
    f["out_indices"] = np.delete(f["out_indices"], r0, axis=0)
    ni = f["nbr_in"]
    ni[ni == r0] = -1
    ni[ni > r0] -= 1
    for name in ("nbr_out",):
        f[name] = np.delete(f[name], r0, axis=1)
    for name in ("rows_out", "masks_out"):
        f[name] = np.delete(f[name], r0, axis=0)
    f["rows_in"], f["masks_in"] = ic.twin_and_masks(ni)
    f["n_out"], f["pair_counts"] = f["n_out"] - 1, osp.pair_counts(f["nbr_out"])
    faults["one output site missing"] = f
    f = copy()
    i = int(np.flatnonzero(f["masks_out"])[0])
    f["masks_out"][i] &= f["masks_out"][i] - 1
    faults["one mask bit cleared"] = f
    f = copy()
    f["rows_out"][r0, 31] = 0
    faults["one twin row not padded"] = f
    f = copy()
    f["rows_in"][5, 27] = 0
    faults["one input twin row not padded"] = f
    for name, f in faults.items():
        with pytest.raises(AssertionError):
            ic.assert_same_tables(f, want, name)
    # the same for a submanifold table set; a route without twins may leave them out, but not a table
    sw = ic.case_subm_tables("D", (3, 3, 3), 1)
    f = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sw.items()}
    f["rows_out"] = f["masks_out"] = None
    ic.assert_same_tables(f, sw, optional=ic.TWINS)
    with pytest.raises(AssertionError):
        ic.assert_same_tables(f, sw)
    f["nbr_bwd"] = None
    with pytest.raises(AssertionError):
        ic.assert_same_tables(f, sw, optional=ic.TWINS)


def test_library_output_shape_is_the_floor_formula(hip_lib):
    """sv_conv_out_shape (host code, the one place the builders take an output grid from) against oracle.spconv.out_shape, per axis, kernels up to 3:
    equal wherever the floor formula leaves a cell; where the kernel is deeper than the padded input (the formula gives 0 or less) the library
    refuses instead of rounding towards zero to a one-cell grid -- what the last level of the network index's spec list met on a 21-deep grid."""
    from seevcn_amd import _lib
    from seevcn_amd.spconv import functional as Fsp
    refused = 0
    for size in range(1, 13):
        for k in (1, 2, 3):
            for s in (1, 2, 3):
                for p in (0, 1):
                    for d in (1, 2):
                        geom = ((size, 7, 9), (k, 3, 1), (s, 2, 1), (p, 1, 0), (d, 1, 1))
                        want = osp.out_shape(*geom)
                        if min(want) > 0:
                            assert tuple(Fsp.conv_out_shape(*geom)) == want, geom
                        else:
                            refused += 1
                            with pytest.raises(_lib.SeevcnHipError, match="empty output shape"):
                                Fsp.conv_out_shape(*geom)
    assert refused > 0
    assert osp.out_shape((2, 16, 14), (3, 1, 1), (2, 1, 1), 0)[0] == 0      # grid E's last level
    with pytest.raises(_lib.SeevcnHipError, match="empty output shape"):
        Fsp.conv_out_shape((2, 16, 14), (3, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1))


# ---------------------------------------------------------------------------------------------------------- GPU
def _np(t):
    return None if t is None else t.cpu().numpy()


def _hip_tables(rb):
    t = {"n_in": rb.n_in, "nbr_out": _np(rb.nbr_out), "rows_out": _np(rb.rows_out), "masks_out": _np(rb.masks_out)}
    if rb.subm:
        t["nbr_bwd"] = _np(rb.table_for_backward_data())
    else:
        t.update(out_indices=_np(rb.out_indices), out_shape=tuple(rb.out_shape), n_out=rb.n_out, nbr_in=_np(rb.nbr_in), rows_in=_np(rb.rows_in),
                 masks_in=_np(rb.masks_in), pair_counts=_np(rb.pair_counts()))
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(ic.GRIDS))
def test_hip_subm_rulebook_at_index_edges(cuda, hip_lib, grid):
    """build_subm_rulebook on edge_coords: through the cell map (table, backward table, row-major twin, masks) and, with no cell-map budget, through
    the rank dictionary (its scan crosses 3 tiles on grid F); the same set twice, then the moved set on the same workspace."""
    import torch
    from seevcn_amd.spconv import functional as Fsp
    batch, shape = ic.GRIDS[grid]
    kernels = SUBM_KERNELS + ([((3, 3, 3), 2)] if grid == "A" else [])
    for ksize, dil in kernels:
        for cap in (Fsp.CELLMAP_MAX_BYTES, 0):
            saved, Fsp.CELLMAP_MAX_BYTES = Fsp.CELLMAP_MAX_BYTES, cap
            try:
                for rep, moved in enumerate((False, False, True)):
                    coords = torch.from_numpy(ic.case_coords(grid, moved).copy()).to(cuda)
                    rb = Fsp.build_subm_rulebook(coords, batch, shape, list(ksize), osp._triple(dil))
                    got = _hip_tables(rb)
                    if cap:
                        assert got["rows_out"] is not None and got["masks_out"] is not None          # the cell-map route makes the twins
                    ic.assert_same_tables(got, ic.case_subm_tables(grid, ksize, dil, moved), (grid, ksize, dil, "map" if cap else "ranks", rep),
                                          optional=() if cap else ic.TWINS)
            finally:
                Fsp.CELLMAP_MAX_BYTES = saved


@pytest.mark.gpu
@pytest.mark.parametrize("grid,geom", _strided_cases())
def test_hip_sparse_rulebook_at_index_edges(cuda, hip_lib, grid, geom):
    """build_sparse_rulebook on the preimage of the output grid's edge_coords: output sites, shape and count, both tables, pair counts, twins and
    masks of both sides; the same set twice, then the moved set on the same persistent index.  Grid F: 4.7 M output cells, 2 scan tiles."""
    import torch
    from seevcn_amd.spconv import functional as Fsp
    batch, shape = ic.GRIDS[grid]
    ksize, stride, padding = (osp._triple(v) for v in geom)
    for rep, moved in enumerate((False, False, True)):
        coords = torch.from_numpy(ic.case_preimage(grid, geom, moved).copy()).to(cuda)
        rb = Fsp.build_sparse_rulebook(coords, batch, shape, ksize, stride, padding)
        ic.assert_same_tables(_hip_tables(rb), ic.case_sparse_tables(grid, geom, moved), (grid, geom, rep))


@pytest.mark.gpu
@pytest.mark.parametrize("lazy_count", [False, True])
@pytest.mark.parametrize("grid,level1", [("C", False), ("E", False), ("F", False), ("E", True), ("F", True)])
def test_hip_network_index_at_index_edges(cuda, hip_lib, grid, level1, lazy_count):
    """build_network_index on edge_coords, EVERY level against the oracle chained level by level (the output sites of level l are the input of level
    l + 1): sites, both tables, twins and masks; with the row count on the host and on the device; twice, then the moved set; the persistent indices
    and cell maps are all-zero afterwards.  Where the oracle gives a level no output grid (grids C and E: the last level's (3, 1, 1) kernel is deeper
    than its input) the build must refuse the chain, and the levels in front of it are built and compared.  level1: the input is the preimage of
    edge_coords laid on the first strided level's output grid, the grid the chain's count and emit kernels index (F: 1 182 720 cells, 5 chain blocks)."""
    import torch
    from seevcn_amd import _lib
    from seevcn_amd.spconv import functional as Fsp
    batch, shape = ic.GRIDS[grid]
    all_specs = [Fsp.ConvSpec(*row) for row in ic.NETWORK_SPECS]
    n_valid = ic.case_network_tables(grid, False, level1)[1]
    assert n_valid == {"C": 8, "E": 8, "F": 9}[grid]
    _lib.workspace.reset()                    # fresh workspaces: the layer-by-layer builders of other tests leave their chunk bases behind
    if n_valid < len(all_specs):
        with pytest.raises(_lib.SeevcnHipError, match="empty output shape"):
            Fsp.build_network_index(torch.from_numpy(ic.case_network_coords(grid, False, level1).copy()).to(cuda), batch, shape, all_specs)
    specs = all_specs[:n_valid]
    for rep, moved in enumerate((False, False, True)):
        want, _ = ic.case_network_tables(grid, moved, level1)
        coords = torch.from_numpy(ic.case_network_coords(grid, moved, level1).copy()).to(cuda)
        n0 = coords.shape[0]
        if lazy_count:
            given = torch.cat([coords, torch.full((333, 4), 1 << 20, dtype=torch.int32, device=cuda)])       # capacity rows behind n0: never read
            n0_dev = torch.tensor([n0], dtype=torch.int32, device=cuda)
        else:
            given, n0_dev = coords, None
        res = Fsp.build_network_index(given, batch, shape, specs, n0_dev=n0_dev)
        assert res is not None
        got_n0, got = res
        assert got_n0 == n0 and sorted(got) == sorted(want)
        for key in want:
            ic.assert_same_tables(_hip_tables(got[key]), want[key], (grid, level1, key, rep))
    torch.cuda.synchronize()
    checked = 0
    for (kind, name, *_), buf in _lib.workspace._bufs.items():
        if kind == "p" and (name.startswith("rb_index_") or name.startswith("rb_cellmap_")):
            assert int(buf.count_nonzero()) == 0, name
            checked += 1
    assert checked >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["A", "D", "F"])
def test_hip_voxelizer_at_index_edges(cuda, hip_lib, grid):
    """The voxeliser shares the index (its key runs x slowest, z fastest: the grid's shape is taken as (X, Y, Z)): one point per cell of edge_coords,
    three in the cells next to a multiple of a block size, unit voxels, range == grid.  Coordinates, point-to-voxel rows and per-voxel point
    counts equal the oracle's; feature means within test_voxelize.py's tolerance; a second run with the moved set on the same workspace."""
    import torch
    from seevcn_amd.pcdet.ops import voxel_ops
    batch, shape = ic.GRIDS[grid]
    gx, gy, gz = shape
    for moved in (False, True):
        cells = ic.case_coords(grid, moved)                                        # [b, x, y, z] here
        keys = ic.keys_of(cells, shape)
        near = np.zeros(len(cells), bool)
        for B in ic.BLOCKS:
            near |= (keys % B == 0) | (keys % B == B - 1)
        assert near.sum() >= 4
        rng = np.random.default_rng(31 + moved)
        cells3 = np.concatenate([cells, cells[near], cells[near]]).astype(np.float32)
        pts = np.concatenate([cells3[:, :1], cells3[:, 1:] + rng.uniform(0.05, 0.95, (len(cells3), 3)).astype(np.float32),
                              rng.normal(size=(len(cells3), 1)).astype(np.float32)], axis=1)
        pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
        pc_range, vs, gsize = [0, 0, 0, gx, gy, gz], [1.0, 1.0, 1.0], [gx, gy, gz]
        fo, co, po = ov.dynamic_mean_vfe(pts, pc_range, vs, gsize)
        assert len(co) == len(cells) and (po >= 0).all()
        f, c, p = voxel_ops.voxelize_dynamic(torch.from_numpy(pts).to(cuda), pc_range, vs, gsize, batch, return_point_to_voxel=True)
        torch.cuda.synchronize()
        c, p, f = c.cpu().numpy(), p.cpu().numpy(), f.cpu().numpy()
        assert c.shape == co.shape and np.array_equal(c, co), (grid, moved)
        assert np.array_equal(p, po), (grid, moved)
        assert np.array_equal(np.bincount(p, minlength=len(c)), np.bincount(po, minlength=len(co))), (grid, moved)
        np.testing.assert_allclose(f, fo, **VOXEL_MEAN_TOL)
