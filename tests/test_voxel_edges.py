"""csrc/voxelize.hip at its edges: the dynamic voxeliser with mean VFE, the hard voxeliser, k_mean_vfe and k_pillar_decorate against the
sequential oracles (oracle/voxelize.py, oracle/hard_voxelize.py) and float64 references written from the definitions
(tests/voxel_edge_reference.py).  CPU: every generated case is shown to hit the edge it is named after.  GPU: points on cell faces and one
ulp either side, feature / stride shapes, the 2^16-point and 2^15-magnitude limits of the fixed-point sums, capacity < V, the 1024-block
seam of the hard voxeliser's scan (and a scene that ends one block past it, beside a one-block scene), a voxel cap inside a block, dense
cells up to max_points = 64, non-finite coordinates, and MeanVFE and the pillar decoration at a tolerance derived per element from fp32
arithmetic."""
import numpy as np
import pytest

import voxel_edge_reference as ve
from oracle import hard_voxelize as ohv
from oracle import voxelize as ov

F = np.float32
VOXEL_MEAN_TOL = dict(rtol=1e-5, atol=1e-5)          # tests/test_voxelize.py's tolerance for the HIP feature means vs the fp32 oracle
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _seam():
    def make():
        pts, geom = ve.seam_scene(7)
        with np.errstate(invalid="ignore"):
            return pts, geom, ohv.points_to_voxel(pts, geom["vs"], geom["pc_range"], 3, 40000)
    return _cached("seam", make)


def _tile_edge():
    def make():
        big, small, geom = ve.tile_edge_scenes(13)
        return big, small, geom, _hard_oracle(big, geom, 3, 4096), _hard_oracle(small, geom, 3, 4096)
    return _cached("tile_edge", make)


def _hard_oracle(points, geom, max_points, max_voxels):
    with np.errstate(invalid="ignore"):               # NaN / inf coordinates are cast to int before they are masked out
        return ohv.points_to_voxel(points, geom["vs"], geom["pc_range"], max_points, max_voxels)


# ---------------------------------------------------------------------------------------------------------- CPU: the cases hit their edges
@pytest.mark.parametrize("name", ["kitti", "pillar"])
def test_face_points_sit_on_the_rounding_edges(name):
    """On a grid whose voxel size is no power of two the face points tell the reference's fp32 subtract / divide / floor from its two likely
    substitutes, and hold a point below `hi` whose cell index equals the grid size."""
    g = ve.GEOMS[name]
    p = ve.face_points(g["lo"], g["vs"], g["grid"], 3000, seed=1)
    assert p.dtype == F and p.shape == (4 * 3000 + 6, 3)
    c32, crec, c64 = ve.cells_fp32(p, g["lo"], g["vs"]), ve.cells_reciprocal(p, g["lo"], g["vs"]), ve.cells_fp64(p, g["lo"], g["vs"])
    frac_rec, frac_64 = (c32 != crec).any(1).mean(), (c32 != c64).any(1).mean()
    print(name, "rows that change cell: reciprocal multiply %.3f, float64 %.3f" % (frac_rec, frac_64))
    assert frac_rec >= 0.05
    assert frac_64 >= 0.05
    grid = np.asarray(g["grid"], F)
    hi = (np.asarray(g["lo"], np.float64) + np.asarray(g["grid"]) * np.asarray(g["vs"], np.float64)).astype(F)
    assert ((c32 == grid) & (p < hi)).any()
    # both sides of the range are present on every axis
    assert (c32 < 0).any(0).all() and (c32 >= grid).any(0).all() and ((c32 >= 0) & (c32 < grid)).all(1).mean() > 0.3


def test_face_points_on_the_unit_grid_are_exact():
    """Unit voxels from the origin: every operation is exact, so this geometry is the control -- no substitute arithmetic changes a cell, a
    face point k lies in cell k, its lower neighbour in cell k - 1, and `hi` itself is out."""
    g = ve.UNIT
    n = 500
    p = ve.face_points(g["lo"], g["vs"], g["grid"], n, seed=2)
    c32 = ve.cells_fp32(p, g["lo"], g["vs"])
    assert np.array_equal(c32, ve.cells_reciprocal(p, g["lo"], g["vs"])) and np.array_equal(c32, ve.cells_fp64(p, g["lo"], g["vs"]))
    base, up, down = p[:n], p[n:2 * n], p[2 * n:3 * n]
    assert np.array_equal(base, np.round(base)) and np.array_equal(c32[:n], base) and np.array_equal(c32[n:2 * n], base)
    assert np.array_equal(c32[2 * n:3 * n], base - 1) and (up > base).all() and (down < base).all()
    assert np.array_equal(c32[-3], np.asarray(g["grid"], F)) and np.array_equal(c32[-1], np.asarray(g["grid"], F) - 1)
    assert np.array_equal(c32[-6], np.zeros(3, F)) and np.array_equal(c32[-4], -np.ones(3, F))


def test_seam_scene_has_first_points_on_both_sides_of_the_seam():
    pts, geom, (vox, crd, nump) = _seam()
    assert len(pts) == 1025 * 256 + 37
    first, coords = ve.first_appearance(pts[:, :3], geom)
    assert np.array_equal(coords, crd)                                     # the oracle's order of first appearance
    assert np.array_equal(vox[:, 0], pts[first])                           # ... and its first stored point
    assert (first >= ve.HV_SEAM).sum() >= 8
    assert (first < ve.HV_SEAM).sum() >= 100
    assert (nump == 3).any()
    block = first // ve.HV_BLOCK
    assert (block == 1023).any() and (block == 1024).any() and (block == 1025).any()
    cell = ve.cells_fp32(pts[:, :3], geom["lo"], geom["vs"])
    in_range = ((cell >= 0) & (cell < np.asarray(geom["grid"], F))).all(1).mean()
    assert 0.05 < in_range < 0.15                                          # about nine points in ten are out of range


def test_tile_edge_scene_ends_one_block_past_the_scan_tile():
    big, small, geom, (vox, crd, nump), (_, scrd, _) = _tile_edge()
    assert len(big) == 1024 * 256 + 1 and len(small) == 255
    first, coords = ve.first_appearance(big[:, :3], geom)
    assert np.array_equal(coords, crd) and np.array_equal(vox[:, 0], big[first])
    assert first[-1] == 1024 * 256                                         # the one point of block 1024 opens the last voxel
    block = first // ve.HV_BLOCK
    assert len(np.unique(block)) > 500 and (block == 1023).any() and np.bincount(block).max() > 4
    assert (nump == 3).sum() > 1000 and (nump < 3).any() and 100 < len(scrd) < 255


def test_cap_cut_scene_cuts_inside_a_block():
    pts, geom, mp, mv = ve.cap_cut_scene(11)
    assert 2000 <= len(pts) <= 5000
    _, crd_all, _ = _hard_oracle(pts, geom, mp, 100000)
    first, coords = ve.first_appearance(pts[:, :3], geom)
    assert np.array_equal(coords, crd_all) and len(first) > mv
    _, crd, _ = _hard_oracle(pts, geom, mp, mv)
    assert len(crd) == mv and np.array_equal(crd, crd_all[:mv])
    last = first[mv - 1]                                                   # the last first point under the cap
    same_block = first[first // ve.HV_BLOCK == last // ve.HV_BLOCK]
    assert same_block[0] < last < same_block[-1]
    later = first[first // ve.HV_BLOCK > last // ve.HV_BLOCK]
    assert len(later) > 0 and len(np.unique(later // ve.HV_BLOCK)) >= 2     # whole blocks whose first points are all past the cap


@pytest.mark.parametrize("mp,stride,off", [(1, 3, 0), (2, 5, 1), (33, 6, 0), (64, 4, 0)])
def test_dense_cells_hold_what_they_promise(mp, stride, off):
    pts, geom = ve.dense_cells(5, mp, stride, off)
    assert 1000 < len(pts) < 5000
    c = ve.cells_fp32(pts[:, off:off + 3], geom["lo"], geom["vs"])
    count = lambda cell: int((c == np.asarray(cell, F)).all(1).sum())
    assert count(ve.DENSE_HEAVY) >= 20 * mp and count(ve.DENSE_EXACT) == mp and count(ve.DENSE_PLUS1) == mp + 1
    assert ((c < 0) | (c >= np.asarray(geom["grid"], F))).any(1).sum() >= 100


def test_cutover_points_sit_at_the_limits():
    pts, voxels = ve.cutover_points(3)
    fo, co, po = ov.dynamic_mean_vfe(pts, ve.CUT_GEOM["pc_range"], ve.CUT_GEOM["vs"], ve.CUT_GEOM["grid"])
    assert len(co) == 7 and (po >= 0).all()
    want = dict(a=65536, b=65536, c=65536 + 64, d=65536 + 4464, e=41, f=65537, g=65536)
    for name, sign in voxels.items():
        rows = ve.cut_voxel_rows(pts, sign)
        assert len(rows) == want[name] and len(np.unique(po[rows])) == 1, name
    a = pts[ve.cut_voxel_rows(pts, voxels["a"]), 1:]
    assert (a == F(ve.VMAX)).all() and ve.VMAX < 32768.0 and np.nextafter(F(ve.VMAX), F(np.inf)) == F(32768.0)
    assert 65536 * int(ve.VMAX * 2 ** 32) < 2 ** 63 <= 65537 * int(ve.VMAX * 2 ** 32)        # a fits the 64-bit sum, f would not
    assert 65536 * int(32768.0 * 2 ** 32) == 2 ** 63                                          # g would not either
    for name in "cd":
        v = np.abs(pts[ve.cut_voxel_rows(pts, voxels[name]), 1:].astype(np.float64))
        assert (v >= 0.5).all() and (v < 1).all() and np.array_equal(v * 1024, np.round(v * 1024))
    e = pts[ve.cut_voxel_rows(pts, voxels["e"]), 1:]
    assert (np.abs(e) == 32768.0).sum() == 1 and (np.abs(e) <= 32768.0).all()


def test_references_agree_with_the_fp32_oracles():
    """The float64 references against the oracles' fp32 restatement of the same modules, inside the derived tolerance; NaN where they have it."""
    g = ve.PILLAR
    for C, pad, absxyz, dist in [(4, False, True, False), (5, True, False, True), (3, True, False, False)]:
        vox, nump, crd = ve.vfe_case(3, 257, 5, C, g, pad)
        want, tol = ve.mean_vfe_ref(vox, nump)
        assert (np.abs(ov.mean_vfe(vox, nump) - want) <= tol).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            o = ohv.pillar_decorate(vox, nump, crd, g["vs"], g["pc_range"], absxyz, dist)
        want, tol = ve.pillar_decorate_ref(vox, nump, crd, g["vs"], g["pc_range"], absxyz, dist)
        assert o.shape == want.shape and np.array_equal(np.isnan(o), np.isnan(want)) and np.isnan(want).any()
        ok = ~np.isnan(want)
        assert (np.abs(o[ok] - want[ok]) <= tol[ok]).all()
        assert tol[ok].max() < 1e-5 * np.abs(vox).max()                      # two orders below the rtol = 1e-3 of the module tests


def test_nuscenes_pillar_centre_offset_sits_on_a_rounding_edge():
    """voxel/2 + range start in float64 of the configured values, rounded once (the module), against the same sum of fp32-rounded inputs: one
    ulp apart at the nuScenes pillar geometry (0.2 / 2 - 51.2), equal at the KITTI ones -- the case that tells the two apart."""
    def offsets(g):
        exact = [F(g["vs"][a] / 2 + g["lo"][a]) for a in range(3)]
        rounded_first = [F(float(F(g["vs"][a])) / 2 + float(F(g["lo"][a]))) for a in range(3)]
        return exact, rounded_first
    exact, rounded_first = offsets(ve.NUSC)
    assert abs(float(exact[0]) - float(rounded_first[0])) == float(np.spacing(np.abs(exact[0]))) and exact[1] != rounded_first[1]
    for g in (ve.KITTI, ve.PILLAR):
        exact, rounded_first = offsets(g)
        assert exact == rounded_first


# ---------------------------------------------------------------------------------------------------------- GPU helpers
def _dyn(points, geom, batch, cuda, **kw):
    import torch
    from seevcn_amd.pcdet.ops import voxel_ops
    out = voxel_ops.voxelize_dynamic(torch.from_numpy(points).to(cuda), geom["pc_range"], geom["vs"], geom["grid"], batch,
                                     return_point_to_voxel=True, **kw)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _hard(points, xyz_offset, C, scene_cnt, geom, max_points, max_voxels, cuda):
    import torch
    from seevcn_amd.pcdet.ops import voxel_ops
    out = voxel_ops.voxelize_hard(torch.from_numpy(points).to(cuda), xyz_offset, C, scene_cnt, geom["pc_range"], geom["vs"], geom["grid"],
                                  max_points, max_voxels)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _assert_hard_scene(got, b, want, tag):
    """Scene b of a voxelize_hard result equals the oracle bit for bit: count, coordinates in order of first appearance, per-voxel counts,
    contents; everything past the count is zero."""
    vox, crd, nmp, nv = got
    ovx, ocrd, onmp = want
    n = int(nv[b])
    assert n == len(ocrd), (tag, b, n, len(ocrd))
    assert np.array_equal(crd[b, :n], ocrd), (tag, b)
    assert np.array_equal(nmp[b, :n], onmp), (tag, b)
    assert np.array_equal(vox[b, :n].view(np.uint32), ovx.view(np.uint32)), (tag, b)
    assert not vox[b, n:].view(np.uint32).any() and not crd[b, n:].any() and not nmp[b, n:].any(), (tag, b)


def _face_batch(name, n, seed, batch=2):
    """[b, x, y, z, f] face points of a geometry for `batch` scenes, shuffled."""
    g = ve.GEOMS[name]
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(batch):
        p = ve.face_points(g["lo"], g["vs"], g["grid"], n, seed=seed + 1 + b)
        rows.append(np.concatenate([np.full((len(p), 1), b, F), p, rng.normal(size=(len(p), 1)).astype(F)], axis=1))
    pts = np.concatenate(rows)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))]), g


# ---------------------------------------------------------------------------------------------------------- GPU: dynamic voxeliser
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kitti", "pillar", "unit"])
def test_hip_dynamic_face_points(cuda, hip_lib, name):
    pts, g = _face_batch(name, 1200, seed=20)
    fo, co, po = ov.dynamic_mean_vfe(pts, g["pc_range"], g["vs"], g["grid"])
    assert (po >= 0).sum() >= 1000 and (po < 0).sum() >= 12               # kept and dropped rows: both sides of the range checks
    f, c, p = _dyn(pts, g, 2, cuda)
    assert c.shape == co.shape and np.array_equal(c, co)
    assert np.array_equal(p, po)
    assert np.array_equal(np.bincount(p[p >= 0], minlength=len(c)), np.bincount(po[po >= 0], minlength=len(co)))
    np.testing.assert_allclose(f, fo, **VOXEL_MEAN_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("nf,stride", [(1, 4), (2, 7), (3, 6), (4, 5), (5, 6)])
def test_hip_dynamic_feature_and_stride_shapes(cuda, hip_lib, nf, stride):
    """Features are columns 1..nf of a row of `stride` floats.  Up to 4 of them: fixed-point sums, one ulp of the float64 mean plus 2^-32.
    Five: fp32 atomic sums, the summation bound of voxel_edge_reference.atomic_mean_tol."""
    g = dict(lo=[0.0, 0.0, 0.0], vs=[0.5, 0.5, 0.5], grid=[8, 8, 4], pc_range=[0, 0, 0, 4, 4, 2])
    rng = np.random.default_rng(40 + nf)
    n = 6000
    pts = (rng.normal(size=(n, stride)) * 100).astype(F)
    pts[:, 0] = rng.integers(0, 2, n)
    pts[:, 1:4] = rng.uniform(-0.2, 4.2, (n, 3))[:, :3]
    pts[:, 3] = rng.uniform(-0.1, 2.1, n)
    fo, co, po = ov.dynamic_mean_vfe(np.ascontiguousarray(pts[:, :1 + nf]), g["pc_range"], g["vs"], g["grid"]) if nf >= 3 else (None, None, None)
    f, c, p = _dyn(pts, g, 2, cuda, num_features=nf)
    assert f.shape == (len(c), nf)
    # rows by the definition: cells of the fp32 arithmetic in ascending [b, x, y, z] key order
    cell = ve.cells_fp32(pts[:, 1:4], g["lo"], g["vs"])
    ok = ((cell >= 0) & (cell < np.asarray(g["grid"], F))).all(1)
    key = ((pts[:, 0].astype(np.int64) * 8 + cell[:, 0].astype(np.int64)) * 8 + cell[:, 1].astype(np.int64)) * 4 + cell[:, 2].astype(np.int64)
    unq, inv = np.unique(key[ok], return_inverse=True)
    want_p = np.full(n, -1, np.int32)
    want_p[ok] = inv
    assert np.array_equal(p, want_p) and len(c) == len(unq)
    ckey = ((c[:, 0].astype(np.int64) * 8 + c[:, 3]) * 8 + c[:, 2]) * 4 + c[:, 1]
    assert np.array_equal(ckey, unq)
    if co is not None:
        assert np.array_equal(c, co) and np.array_equal(p, po)
    for row in range(len(unq)):
        vals = pts[want_p == row, 1:1 + nf]
        want = vals.astype(np.float64).mean(0)
        tol = ve.fixed_mean_tol(want) if nf <= 4 else ve.atomic_mean_tol(vals)
        assert (np.abs(f[row].astype(np.float64) - want) <= tol).all(), (row, f[row], want, tol)


@pytest.mark.gpu
def test_hip_dynamic_fixed_point_cut_over(cuda, hip_lib):
    """The limits of the 64-bit fixed-point sums (voxel_edge_reference.cutover_points): 2^16 points of the largest value below 2^15 and of
    its negative give exactly that value; points past the 65536th and values of 2^15 go to the fp32 side sum and the mixed finalize holds
    the bound 63 * 2^-24 * (sum of the 64 largest |v|) / n + one ulp + 2^-32 (c, d: their side sums are exact by construction, so the bound
    of c holds for d as well); one more point (f) or a value of exactly 2^15 (g) in fixed point would overflow.  Bit-identical under
    three permutations."""
    pts, voxels = ve.cutover_points(3)
    g = ve.CUT_GEOM
    f, c, p = _dyn(pts, g, 1, cuda)
    assert len(c) == 7
    row = {name: int(p[ve.cut_voxel_rows(pts, sign)[0]]) for name, sign in voxels.items()}
    for seed in range(3):
        perm = np.random.default_rng(50 + seed).permutation(len(pts))
        f2, c2, _ = _dyn(np.ascontiguousarray(pts[perm]), g, 1, cuda)
        assert np.array_equal(c2, c)
        for name in "abcdfg":
            assert np.array_equal(f2[row[name]].view(np.uint32), f[row[name]].view(np.uint32)), (name, seed)
    vmax = F(ve.VMAX)
    assert np.array_equal(f[row["a"]], np.full(4, vmax)), f[row["a"]]
    assert np.array_equal(f[row["b"]], np.full(4, -vmax)), f[row["b"]]
    assert np.array_equal(f[row["f"]], np.asarray([-vmax, -vmax, vmax, vmax])), f[row["f"]]
    assert np.array_equal(f[row["g"]], np.asarray([32768.0, -32768.0, -32768.0, 32768.0], F)), f[row["g"]]
    for name in "cd":
        vals = pts[ve.cut_voxel_rows(pts, voxels[name]), 1:].astype(np.float64)
        want = vals.mean(0)
        T = np.sort(np.abs(vals), axis=0)[-64:].sum(0)
        tol = 63 * 2.0 ** -24 * T / len(vals) + ve.fixed_mean_tol(want)
        assert (np.abs(f[row[name]].astype(np.float64) - want) <= tol).all(), (name, f[row[name]], want, tol)
    vals = pts[ve.cut_voxel_rows(pts, voxels["e"]), 1:].astype(np.float64)
    want = vals.mean(0)
    assert (np.abs(f[row["e"]].astype(np.float64) - want) <= ve.fixed_mean_tol(want)).all(), (f[row["e"]], want)


@pytest.mark.gpu
def test_hip_dynamic_capacity_below_voxel_count(cuda, hip_lib):
    """capacity < V with sync=False: the device count is the capacity, the rows are the oracle's first `capacity` voxels in key order, points
    of dropped voxels get -1, and the persistent index is left clean for the next call on the same grid."""
    g = dict(lo=[0.0, -4.0, -1.0], vs=[0.25, 0.25, 0.5], grid=[32, 32, 4], pc_range=[0, -4, -1, 8, 4, 1])
    rng = np.random.default_rng(60)
    n = 7000
    pts = np.concatenate([rng.integers(0, 1, (n, 1)), rng.uniform(-0.3, 8.3, (n, 1)), rng.uniform(-4.3, 4.3, (n, 1)), rng.uniform(-1.1, 1.1, (n, 1)),
                          rng.normal(size=(n, 1))], axis=1).astype(F)
    fo, co, po = ov.dynamic_mean_vfe(pts, g["pc_range"], g["vs"], g["grid"])
    V = len(co)
    assert 2500 <= V <= 3500
    for cap in (V // 2, 1, V):
        f, c, p, nv = _dyn(pts, g, 1, cuda, capacity=cap, sync=False)
        assert int(nv[0]) == cap and f.shape == (cap, 4) and c.shape == (cap, 4)
        assert np.array_equal(c, co[:cap]), cap
        np.testing.assert_allclose(f, fo[:cap], **VOXEL_MEAN_TOL)
        assert np.array_equal(p, np.where(po < cap, po, -1)), cap
        f, c, p = _dyn(pts, g, 1, cuda)                                    # default capacity on the index the capped call left behind
        assert np.array_equal(c, co) and np.array_equal(p, po), cap
        np.testing.assert_allclose(f, fo, **VOXEL_MEAN_TOL)


# ---------------------------------------------------------------------------------------------------------- GPU: hard voxeliser
@pytest.mark.gpu
def test_hip_hard_seam_scene(cuda, hip_lib):
    pts, geom, want = _seam()
    got = _hard(pts, 0, 4, [len(pts)], geom, 3, 40000, cuda)
    _assert_hard_scene(got, 0, want, "seam")


@pytest.mark.gpu
def test_hip_hard_seam_scene_between_an_empty_and_an_all_out_scene(cuda, hip_lib):
    pts, geom, want = _seam()
    rng = np.random.default_rng(70)
    outer = np.concatenate([rng.uniform(0, 16, (500, 2)), rng.uniform(2.0001, 9, (500, 1)), rng.normal(size=(500, 1))], axis=1).astype(F)
    outer[::3, 0] = -outer[::3, 0] - F(1e-3)
    assert len(_hard_oracle(outer, geom, 3, 40000)[1]) == 0
    got = _hard(np.concatenate([pts, outer]), 0, 4, [0, len(pts), len(outer)], geom, 3, 40000, cuda)
    empty = (np.zeros((0, 3, 4), F), np.zeros((0, 3), np.int32), np.zeros((0,), np.int32))
    assert got[3].tolist() == [0, len(want[1]), 0]
    _assert_hard_scene(got, 0, empty, "empty scene")
    _assert_hard_scene(got, 1, want, "seam in the middle")
    _assert_hard_scene(got, 2, empty, "all points out of range")


@pytest.mark.gpu
@pytest.mark.parametrize("big_first", [True, False])
def test_hip_hard_scan_tile_edge_beside_a_small_scene(cuda, hip_lib, big_first):
    """1025 point blocks beside a scene of one block: the scan of the block counts takes a second tile for its last element in one scene and
    scans 1024 empty blocks in the other.  Integer work: order, coordinates, counts and num_voxels are the oracle's exactly."""
    big, small, geom, want_big, want_small = _tile_edge()
    scenes = [(big, want_big), (small, want_small)][::1 if big_first else -1]
    got = _hard(np.concatenate([p for p, _ in scenes]), 0, 4, [len(p) for p, _ in scenes], geom, 3, 4096, cuda)
    assert got[3].tolist() == [len(w[1]) for _, w in scenes]
    for b, (_, want) in enumerate(scenes):
        _assert_hard_scene(got, b, want, f"scene {b}")


@pytest.mark.gpu
def test_hip_hard_cap_inside_a_block(cuda, hip_lib):
    pts, geom, mp, mv = ve.cap_cut_scene(11)
    got = _hard(pts, 0, 4, [len(pts)], geom, mp, mv, cuda)
    assert int(got[3][0]) == mv
    _assert_hard_scene(got, 0, _hard_oracle(pts, geom, mp, mv), "cap cut")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kitti", "pillar"])
def test_hip_hard_face_points(cuda, hip_lib, name):
    pts, g = _face_batch(name, 1200, seed=80, batch=1)
    pts = np.ascontiguousarray(pts[:, 1:])
    want = _hard_oracle(pts, g, 5, 20000)
    assert len(want[1]) > 500
    _assert_hard_scene(_hard(pts, 0, 4, [len(pts)], g, 5, 20000, cuda), 0, want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("mp,C,off,stride", [(1, 3, 0, 3), (2, 4, 1, 5), (33, 3, 0, 6), (64, 4, 0, 4)])
def test_hip_hard_dense_cells_max_points_and_stride(cuda, hip_lib, mp, C, off, stride):
    """A cell of more than 20 * max_points points, one of exactly max_points and one of max_points + 1; a batch column in front
    (xyz_offset 1), trailing columns that are not copied (stride 6, C 3), and max_points from 1 to 64, the largest the library admits."""
    pts, geom = ve.dense_cells(5, mp, stride, off)
    want = _hard_oracle(np.ascontiguousarray(pts[:, off:off + C]), geom, mp, 40)
    assert (want[2] == mp).sum() >= 3 and len(want[1]) == 32
    _assert_hard_scene(_hard(pts, off, C, [len(pts)], geom, mp, 40, cuda), 0, want, (mp, C, off, stride))


@pytest.mark.gpu
def test_hip_hard_refuses_more_than_64_points_per_voxel(cuda, hip_lib):
    from seevcn_amd import _lib
    pts, geom = ve.dense_cells(5, 2, 4, 0)
    with pytest.raises(_lib.SeevcnHipError, match="at most 64 points per voxel"):
        _hard(pts, 0, 4, [len(pts)], geom, 65, 40, cuda)
    _assert_hard_scene(_hard(pts, 0, 4, [len(pts)], geom, 2, 40, cuda), 0, _hard_oracle(pts, geom, 2, 40), "after the refusal")


@pytest.mark.gpu
def test_hip_hard_non_finite_and_negative_zero_coordinates(cuda, hip_lib):
    """NaN and +-inf coordinates are dropped; -0.0 lies in cell 0 of a range that starts at 0."""
    g = ve.UNIT
    rng = np.random.default_rng(90)
    pts = np.concatenate([rng.uniform(-0.5, 8.5, (300, 1)), rng.uniform(-0.5, 6.5, (300, 1)), rng.uniform(-0.5, 4.5, (300, 1)),
                          np.arange(300)[:, None]], axis=1).astype(F)
    bad = [np.nan, np.inf, -np.inf]
    for i, row in enumerate(range(5, 5 + 9 * 7, 7)):
        pts[row, i % 3] = bad[i // 3]
    zero_rows = [2, 100, 250]
    pts[2, :3] = [-0.0, 3.5, 2.5]
    pts[100, :3] = [7.5, -0.0, -0.0]
    pts[250, :3] = [-0.0, -0.0, -0.0]
    want = _hard_oracle(pts, g, 4, 300)
    stored = set(want[0][..., 3].astype(int).ravel().tolist())
    assert not stored & set(range(5, 5 + 9 * 7, 7))
    for r in zero_rows:                                                     # each -0.0 point opened or joined the voxel of cell 0 on that axis
        z, y, x = (0 if np.signbit(pts[r, 2]) else 2), (0 if np.signbit(pts[r, 1]) else 3), (0 if np.signbit(pts[r, 0]) else 7)
        v = np.nonzero((want[1] == [z, y, x]).all(1))[0]
        assert len(v) == 1 and r in want[0][v[0], :want[2][v[0]], 3].astype(int).tolist()
    _assert_hard_scene(_hard(pts, 0, 4, [len(pts)], g, 4, 300, cuda), 0, want, "non-finite")


@pytest.mark.gpu
def test_hip_point2voxel_round_trip_on_face_points(cuda, hip_lib):
    from seevcn_amd.spconv.utils import Point2VoxelCPU3d
    pts, g = _face_batch("kitti", 1200, seed=81, batch=1)
    pts = np.ascontiguousarray(pts[:, 1:])
    gen = Point2VoxelCPU3d(vsize_xyz=g["vs"], coors_range_xyz=g["pc_range"], num_point_features=4, max_num_points_per_voxel=5, max_num_voxels=20000)
    assert gen.grid_size.tolist() == g["grid"]
    vox, crd, nmp = (a.numpy() for a in gen.point_to_voxel(pts))
    ovx, ocrd, onmp = _hard_oracle(pts, g, 5, 20000)
    assert vox.dtype == F and crd.dtype == np.int32 and nmp.dtype == np.int32
    assert np.array_equal(crd, ocrd) and np.array_equal(nmp, onmp) and np.array_equal(vox.view(np.uint32), ovx.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- GPU: MeanVFE and the decoration
VFE_V = [0, 1, 255, 257, 1000]


@pytest.mark.gpu
@pytest.mark.parametrize("mp", [1, 5, 32, 100])
def test_hip_mean_vfe_against_float64(cuda, hip_lib, mp):
    """sum over ALL slots / max(count, 1) within the derived fp32 bound, for every V and C, zero and non-zero padding, counts 0..max_points."""
    import torch
    from seevcn_amd.pcdet.ops import voxel_ops
    for V in VFE_V:
        for C in (1, 3, 4, 5):
            for pad in (False, True):
                vox, nump, _ = ve.vfe_case(100 + V + C, V, mp, C, ve.KITTI, pad)
                got = voxel_ops.mean_vfe(torch.from_numpy(vox).to(cuda), torch.from_numpy(nump).to(cuda)).cpu().numpy()
                want, tol = ve.mean_vfe_ref(vox, nump)
                assert got.shape == (V, C)
                assert (np.abs(got.astype(np.float64) - want) <= tol).all(), (V, C, pad, np.abs(got - want).max())


@pytest.mark.gpu
@pytest.mark.parametrize("mp", [1, 5, 32, 100])
def test_hip_pillar_decorate_against_float64(cuda, hip_lib, mp):
    """Every column of the decoration within the per-element fp32 bound of voxel_edge_reference.pillar_decorate_ref: both values of
    use_absolute_xyz (C = 3 leaves no raw column) and with_distance, coordinates at the origin cell and the far corner, a negative range
    origin, zero and non-zero padding.  Pillars of count 0 are NaN exactly where the float64 reference is."""
    import torch
    from seevcn_amd.pcdet.ops import voxel_ops
    seen_nan = False
    for V in VFE_V:
        for C in (3, 4, 5):
            for pad, absxyz, dist, g in [(False, True, False, ve.PILLAR), (True, False, True, ve.PILLAR), (True, True, True, ve.KITTI),
                                         (False, False, False, ve.KITTI), (False, True, False, ve.NUSC)]:
                vox, nump, crd = ve.vfe_case(200 + V + C, V, mp, C, g, pad)
                got = voxel_ops.pillar_decorate(torch.from_numpy(vox).to(cuda), torch.from_numpy(nump).to(cuda), torch.from_numpy(crd).to(cuda),
                                                g["vs"], g["pc_range"], absxyz, dist).cpu().numpy()
                want, tol = ve.pillar_decorate_ref(vox, nump, crd, g["vs"], g["pc_range"], absxyz, dist)
                tag = (V, C, pad, absxyz, dist)
                assert got.shape == want.shape == (V, mp, (C if absxyz else C - 3) + 6 + int(dist)), tag
                assert np.array_equal(np.isnan(got), np.isnan(want)), tag
                ok = ~np.isnan(want)
                seen_nan |= bool((~ok).any())
                assert (np.abs(got[ok].astype(np.float64) - want[ok]) <= tol[ok]).all(), (tag, np.abs(got[ok] - want[ok]).max())
    assert seen_nan


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pillar", "nusc"])
def test_hip_pillar_decorate_bit_equal_to_the_fp32_oracle(cuda, hip_lib, name):
    """Without contraction the kernel's fp32 operations are the oracle's, slot sums included (both add slot 0, 1, 2, ... in turn): the same
    bits, sign of zero included, for every count >= 1.  At the nuScenes geometry the pillar-centre offset is one ulp off unless it is formed
    in float64 from the configured values."""
    import torch
    from seevcn_amd.pcdet.ops import voxel_ops
    g = ve.GEOMS[name]
    vox, nump, crd = ve.vfe_case(300, 257, 32, 4, g, True)
    nump = np.maximum(nump, 1)
    got = voxel_ops.pillar_decorate(torch.from_numpy(vox).to(cuda), torch.from_numpy(nump).to(cuda), torch.from_numpy(crd).to(cuda),
                                    g["vs"], g["pc_range"], True, True).cpu().numpy()
    want = ohv.pillar_decorate(vox, nump, crd, g["vs"], g["pc_range"], True, True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
