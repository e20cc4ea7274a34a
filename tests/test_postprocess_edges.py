"""csrc/postprocess.hip at its edges, bit for bit (tests/post_edge_cases.py builds the inputs): the query-slice loop, the exact-tie paths and the set-order
replay of the surface selection against oracle.postprocess.partial_with_kdtree; the strictness and tie rules of the largest cluster, plain and periodic,
against oracle.postprocess.largest_cluster; sv_dedup_rows against the first-occurrence rule; both "points near a set" entries, with 3 and 4 columns,
against a float64 restatement.  CPU: every crafted family does what it claims, by the oracle alone.  No tolerances anywhere."""
import numpy as np
import pytest
import torch

import post_edge_cases as pc
from oracle import postprocess as opp


# ---------------------------------------------------------------------------------------------------------- CPU: the inputs themselves
def test_batch_sizes_give_every_slice_count():
    """nsplit = clamp(4096 / batch, 1, 64) (sv_vcn_surface_select): the batches cover 64, 63, 4, 2 and 1 slices, and each launch holds objects with one
    query, with fewer queries than one round of all slices takes (4 waves a slice), with more, and different counts side by side."""
    assert [min(max(4096 // b, 1), 64) for b in pc.SLICE_BATCHES] == [pc.nsplit_of(b) for b in pc.SLICE_BATCHES] == [64, 63, 4, 2, 1]
    for batch in pc.SLICE_BATCHES:
        partial, coarse, nq = pc.slice_case(batch)
        assert partial.shape == (batch, pc.SLICE_N, 3) and coarse.shape == (batch, pc.SLICE_M, 3) and pc.SLICE_N <= 40 and pc.SLICE_M <= 33 and pc.SLICE_SP <= 64
        assert [len(np.unique(p, axis=0)) for p in partial[:64]] == nq[:64].tolist()
        round_size = pc.KNN_WAVES * pc.nsplit_of(batch)
        if batch > 1:
            assert (nq == 1).any() and (nq < round_size).any() and len(set(nq.tolist())) > 4
            assert (nq > round_size).any() or round_size >= pc.SLICE_N
        else:
            assert 1 < nq[0] < round_size                                   # more slices than queries


@pytest.mark.parametrize("name", list(pc.TIE_CONFIGS))
def test_tie_inputs_tie_exactly_in_float64(name):
    partial, coarse = pc.tie_case(name)
    m = coarse.shape[1]
    assert (m % 64 != 0) and (m < 64) == (name == "m33")
    for obj in range(2):
        assert len(np.unique(coarse[obj], axis=0)) < m                      # duplicated coarse rows
        ties, in_lane, cross_lane = pc.tie_census(partial[obj], coarse[obj], max(pc.TIE_K))
        assert ties >= 1 and cross_lane >= 1, (name, obj)
        assert in_lane >= 1 or m < 64, (name, obj)                          # two coarse indices congruent mod 64 need m > 64
    # the group sizes the k range is built on: 8 corners at 0.75 around a centre; the row and its copy at 0, then 6 at 1, around an inner lattice point
    c = np.unique(coarse[1], axis=0).astype(np.float64)                         # without the copies
    d2 = lambda q: np.sort(((c - np.asarray(q, np.float64)) ** 2).sum(axis=1))
    assert d2([0.5, 0.5, 0.5])[:8].tolist() == [0.75] * 8 and d2([0.5, 0.5, 0.5])[8] > 0.75
    inner = d2([1, 1, 1])
    n0 = int((inner == 0).sum())
    assert n0 == 1 and (inner == 1).sum() == 6 and max(pc.TIE_K) == 8 + 1
    # and the rule shows: with the HIGHEST index first among equal distances (the stable sort over the reversed cloud) other indices are selected
    flipped = 0
    for k in pc.TIE_K:
        for o in range(2):
            queries = np.unique(partial[o], axis=0)
            lowest = opp.knn_indices(queries, coarse[o], k)
            highest = m - 1 - opp.knn_indices(queries, coarse[o][::-1], k)
            flipped += set(np.unique(lowest).tolist()) != set(np.unique(highest).tolist())
    assert flipped > 0


def test_set_size_inputs_select_exactly_each_table_boundary():
    assert pc.SET_SIZES == (1, 4, 5, 18, 19, 76, 77, 306, 307, 1024)
    for count in pc.SET_SIZES:
        partial, coarse, chosen = pc.set_case(count)
        _, nsel = pc.set_want(count, "default")
        assert nsel.tolist() == [count] * len(pc.SET_VARIANTS)
        for v, mod in enumerate((None, 8, 32, 128)):
            idx = chosen[v]
            assert len(idx) == count and len(np.unique(partial[v], axis=0)) == count
            got = np.unique(opp.knn_indices(np.unique(partial[v], axis=0), coarse[v], 1))
            assert np.array_equal(got, idx)                                  # the oracle selects exactly the planned indices
            if mod is not None and count > 1:                                 # the replay's collisions occur: one residue class as far as it reaches
                assert np.bincount(idx % mod).max() >= min(count, 1024 // mod)
        if count > 8:
            assert chosen[0].min() < 128 and chosen[0].max() >= 896          # spread over 0 .. 1023
        sp = [pc.surface_pts_of(count, kind) for kind in pc.SP_KINDS]
        assert sp[0] == 1 and sp[2] == count and sp[1] <= count and (count == 1 or (sp[1] < count and sp[3] % count != 0)) and sp[4] == 1024
    # the order matters where it should: below 307 the set order is not the ascending one for a colliding set, from 307 on it is
    order = lambda count, v: [int(i) for i in set(np.int64(x) for x in pc.set_case(count)[2][v])]
    assert order(306, 1) != sorted(order(306, 1)) and order(307, 1) == sorted(order(307, 1)) and order(18, 1) != sorted(order(18, 1))


def test_low_word_inputs_agree_in_the_high_32_bits_only():
    partial, coarse = pc.low_word_case()
    assert max(pc.LOW_WORD_K) <= coarse.shape[1]
    for obj, group in ((0, 32), (1, 16)):
        c = coarse[obj].astype(np.float64)
        for q in np.unique(partial[obj], axis=0).astype(np.float64):
            d = c - q
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            top = np.argsort(d2, kind="stable")[:group]
            bits = d2[top].view(np.uint64)
            assert len(set((bits >> np.uint64(32)).tolist())) == 1 and len(set((bits & np.uint64(0xffffffff)).tolist())) == 16
            assert d2[top[-1]] < d2.min(initial=np.inf, where=~np.isin(np.arange(len(c)), top))          # the group is the nearest rows
            assert not np.array_equal(top, np.sort(top))                                               # index order is not distance order
            assert (len(np.unique(d2[top])) == 16) and ((group == 32) == (np.diff(d2[top]) == 0).any())   # exact ties on top in object 0


def _surface_by_visits(queries, coarse, k, surface_pts):
    """The tail of oracle.postprocess.partial_with_kdtree for queries visited in the given order."""
    idx = []
    for row in opp.knn_indices(queries, coarse, k):
        idx.extend(row)
    idx = list(set(idx))
    return np.tile(coarse[idx], [surface_pts, 1])[:surface_pts, :]


def test_unique_edge_inputs_hold_both_zeros():
    partial, coarse = pc.unique_edge_case()
    want, nsel = pc.unique_edge_want()
    for obj, col in ((0, 0), (1, 1)):
        z = partial[obj][:, col]
        assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
        assert len(np.unique(partial[obj], axis=0)) == 12 and len(np.unique(partial[obj].view(np.uint32), axis=0)) == 16
        # np.unique's order is what the output shows: visiting the rows with the sign of the zero as part of the key gives another surface
        rows = np.unique(partial[obj], axis=0)
        assert np.array_equal(_surface_by_visits(rows, coarse[obj], pc.UNIQUE_K, 64), want[obj])
        signed = partial[obj][np.lexsort([partial[obj][:, c] if c != col else ~np.signbit(z) for c in (2, 1, 0)])]
        assert not np.array_equal(_surface_by_visits(signed, coarse[obj], pc.UNIQUE_K, 64), want[obj])
    assert len(np.unique(partial[2], axis=0)) == 1
    assert nsel[2] == pc.UNIQUE_K and 4 < nsel[0] < 77 and 4 < nsel[1] < 77     # small tables: the insert order, i.e. np.unique's row order, shows


def test_cluster_inputs_sit_on_their_edges():
    cases = pc.cluster_cases()
    size = lambda name, mp: pc.cluster_want(name, mp)[1]
    d2 = lambda a, b: float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum())
    for stem in ("lattice_pure", "lattice_pair", "pythagoras", "periodic_lattice"):
        cloud, eps, _, _ = cases[stem + "_eps_exact"]
        nxt = cases[stem + "_eps_next"][1]
        assert nxt == np.nextafter(eps, np.inf) and np.array_equal(cases[stem + "_eps_next"][0], cloud)
        pairs = sum(d2(cloud[i], cloud[j]) == eps * eps for i in range(min(len(cloud), 64)) for j in range(i))
        assert pairs > 0                                                      # squared distances EQUAL to eps^2 in float64
        assert size(stem + "_eps_exact", 1) < size(stem + "_eps_next", 1)
    assert size("lattice_pure_eps_exact", 1) == 1 and size("lattice_pure_eps_next", 2) == 216
    for name, blobs in (("equal_two", 2), ("equal_three", 3)):
        cloud = cases[name][0]
        labels = opp.dbscan_labels(cloud, 0.4, 2)
        sizes = np.bincount(labels)
        assert (sizes == sizes.max()).sum() == blobs and sizes[0] < sizes.max()             # label 0 (it holds row 0) is a smaller component
        won = pc.cluster_want(name, 2)[0][0]
        assert won[0] > 5.0                                                                 # not the blob at the origin, which was generated first
    assert size("path_1024_shuffled", 2) == 1024 and size("one_component", 2) == 300
    x = cases["path_1024_shuffled"][0][:, 0]
    assert (np.diff(x) < 0).sum() > 400                                       # stored in shuffled order
    for name in ("isolated", "n1", "n2_far", "lattice_pure_eps_exact"):
        cloud, eps, mps, _ = cases[name]
        assert 2 not in mps and all(size(name, mp) == 1 for mp in mps)
        with pytest.raises(ValueError):
            opp.largest_cluster(cloud, eps=eps, min_points=2)
    noise, eps, mp = pc.noise_batch()
    for b, n in ((0, 0), (1, 10), (2, 0)):
        assert (opp.dbscan_labels(noise[b], eps, mp) >= 0).sum() == n
    for name, (cloud, eps, mps, period) in cases.items():
        if period is not None:
            assert np.array_equal(cloud, np.tile(cloud[:period], (len(cloud) // period + 1, 1))[:len(cloud)])
            assert len(cloud) % period != 0 or period == 1, name              # a partial last copy
    assert cases["periodic_lattice_eps_exact"][3] % 2 == 0 and cases["periodic_equal_three"][3] % 2 == 1


@pytest.mark.parametrize("family", pc.DEDUP_FAMILIES)
def test_dedup_expectation_is_first_occurrence_and_agrees_with_np_unique(family):
    for n in pc.DEDUP_SIZES:
        rows = pc.dedup_case(family, n)
        out, flag = pc.dedup_expect(rows)
        assert rows.shape == (n, 4) and pc.same_bits(out[:, 1:], rows[:, 1:]) and pc.same_bits(out[~flag], rows[~flag])
        live = ~(rows[:, 0] < 0)
        assert not flag[~live].any()
        nan = np.isnan(rows).any(axis=1)
        assert not flag[nan].any()                                            # NaN rows all survive
        keep = live & ~flag & ~nan
        if (live & ~nan).any():                                               # the survivors as a set == np.unique of the live rows
            assert np.array_equal(np.unique(rows[keep] + 0.0, axis=0), np.unique(rows[live & ~nan] + 0.0, axis=0))
            assert len(np.unique(rows[keep], axis=0)) == keep.sum()           # ... each once
        first = {}
        for i in np.nonzero(live & ~nan)[0]:                                  # ... and the FIRST of every group of equal rows
            first.setdefault(tuple((rows[i] + 0.0).tolist()), i)
        assert sorted(first.values()) == np.nonzero(keep)[0].tolist()
    big = pc.dedup_case(family, 4096)
    f = pc.dedup_expect(big)[1]
    want = {"all_equal": 4095, "all_distinct": 0, "far_duplicates": 2048}.get(family)
    assert want is None or f.sum() == want
    if family == "signed_zeros":
        assert (~f).sum() == 2 and np.signbit(big[big == 0]).any() and not np.signbit(big[big == 0]).all()
    if family == "nan_rows":
        assert np.isnan(big).any(axis=1).sum() > 1000 and f.sum() > 1000
    if family == "dropped_rows":
        assert (big[:5, 0] < 0).all() and (~f & (big[:, 0] >= 0)).sum() == 5 and len(np.unique(big[:, 1:], axis=0)) == 5


def test_near_inputs_hold_distances_equal_to_the_threshold():
    cases = pc.near_threshold_cases()
    q, r, thresh = cases["pythagoras_5"]
    d = np.sqrt(((q[:, None, 1:].astype(np.float64) - r[None, :, 1:].astype(np.float64)) ** 2).sum(axis=2)).min(axis=1)
    assert thresh == 5.0 and (d == 5.0).sum() >= 8
    lo, hi = np.nextafter(np.float32(3), np.float32(0)), np.nextafter(np.float32(3), np.float32(9))
    assert {float(lo), float(hi)} <= set(q[:, 1].tolist()) | set(q[:, 2].tolist()) and lo < 3 < hi
    assert ((d < 5.0) & (d > 4.9999)).sum() >= 2 and ((d > 5.0) & (d < 5.0001)).sum() >= 2           # the next float32 on either side
    want = pc.near_want(q, r, 5.0)
    assert not want[d == 5.0].any() and pc.near_want(q, r, cases["pythagoras_5_next"][2])[d == 5.0].all()
    q, r, thresh = cases["tenth"]
    x = np.abs(q[:, 1:]).max(axis=1).astype(np.float64)
    assert thresh == 0.1 and (x < 0.1).sum() == 6 and (x > 0.1).sum() == 12 and np.float64(pc.F01) in x
    assert np.array_equal(pc.near_want(q, r, 0.1), x < 0.1)
    q, r, thresh = cases["zero"]
    assert thresh == 0.0 and (q[:3, 1:] == r[:, 1:]).all() and not pc.near_want(q, r, 0.0).any() and pc.near_want(q, r, 1e-2).all()
    # the restatement against cKDTree on a dense case, and the scene rule
    from scipy.spatial import cKDTree
    q, r, thresh = pc.near_dense_case(False)
    want = pc.near_want(q, r, thresh)
    for s in (0, 1):
        dist = cKDTree(r[r[:, 0] == s][:, 1:].astype(np.float64)).query(q[q[:, 0] == s][:, 1:].astype(np.float64))[0]
        assert np.array_equal(want[q[:, 0] == s], dist < thresh)
    assert 200 < want.sum() < 1800
    q, r, thresh = pc.near_seam_case(True)
    want = pc.near_want(q, r, thresh)
    assert not want[np.isin(q[:, 0], (3, 5))].any() and all(want[q[:, 0] == s].any() for s in (0, 1, 2, 4))
    assert len(set(r[:128, 0].tolist())) == 3 and set(r[256:, 0].tolist()) == {4.0} and {2.0, 4.0} <= set(r[128:256, 0].tolist())
    assert pc.near_want(q[:, 1:], r[:, 1:], thresh)[np.isin(q[:, 0], (3, 5))].any()           # the same points ARE near without the scene rule
    far = pc.near_dense_case(False, 1.0e4)
    assert np.abs(far[1][:, 1:]).min() > 9.9e3 and np.spacing(far[1][:, 1:]).min() >= 2.0 ** -10 and 200 < pc.near_want(*far).sum() < 1800


@pytest.mark.parametrize("tile", [pc.NB_TILE, pc.NS_TILE])
def test_near_dropped_input_drops_whole_and_partial_tiles(tile):
    before, q = pc.near_dropped_input(tile)
    ref, _ = pc.dedup_expect(before)
    live, T = ref[:, 0] >= 0, tile
    assert len(ref) == 4 * T + 9 and (before[:, 0] < 0).sum() == T // 2
    assert live[:T].all() and not live[T:2 * T].any() and not live[2 * T] and live[2 * T + 1:3 * T].all() and not live[3 * T:4 * T - 1].any() and live[4 * T - 1]
    want = pc.near_want(q, ref, 0.1)
    half = len(q) // 2
    assert not want[half:].any() and not want[120:160].any()                    # scene id -1; the place of the rows that arrived dropped
    assert pc.near_want(q[120:160, 1:], before[:, 1:], 0.1).any()               # ... where the dropped rows themselves ARE within the threshold
    assert want[:40].any() and want[40:80].any() and want[200] and want[160:200].any() and not want[:half].all()


# ---------------------------------------------------------------------------------------------------------- GPU
def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)                     # a copy: the cases are read-only


def _surface(partial, coarse, k, surface_pts, cuda):
    from seevcn_amd.vcn.utils import sampling as S
    out, nsel = S.get_partial_mesh_batch_device(_dev(partial, cuda), _dev(coarse, cuda), k=k, surface_pts=surface_pts)
    assert out.dtype == torch.float32 and nsel.dtype == torch.int32
    return out.cpu().numpy(), nsel.cpu().numpy()


def _assert_surface(got, want, tag):
    (surface, nsel), (w_surface, w_nsel) = got, want
    assert np.array_equal(nsel, w_nsel), (tag, "n_selected", np.nonzero(nsel != w_nsel)[0][:8].tolist())
    bad = np.nonzero((surface.view(np.uint32) != w_surface.view(np.uint32)).any(axis=(1, 2)))[0]
    assert len(bad) == 0 and np.array_equal(surface, w_surface), (tag, "objects that differ", bad[:8].tolist(), len(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", pc.SLICE_BATCHES)
def test_hip_surface_select_query_slices(batch, cuda, hip_lib):
    """64, 63, 4, 2 and 1 query slices per object; objects with 1 .. 40 distinct queries side by side in one launch."""
    partial, coarse, _ = pc.slice_case(batch)
    _assert_surface(_surface(partial, coarse, pc.SLICE_K, pc.SLICE_SP, cuda), pc.slice_want(batch), batch)


@pytest.mark.gpu
def test_hip_surface_select_full_size_batch_of_two(cuda, hip_lib):
    _assert_surface(_surface(*pc.full_size_case(), 30, 1024, cuda), pc.full_size_want(), "1024 x 1024, k = 30")


@pytest.mark.gpu
@pytest.mark.parametrize("k", pc.TIE_K)
@pytest.mark.parametrize("name", list(pc.TIE_CONFIGS))
def test_hip_surface_select_exact_distance_ties(name, k, cuda, hip_lib):
    """Equal float64 squared distances inside one lane's candidates and across lanes, duplicated coarse rows, k from 1 through the 8-way tie group and
    one past it: the lower coarse index comes first (np.argsort(kind='stable'))."""
    partial, coarse = pc.tie_case(name)
    _assert_surface(_surface(partial, coarse, k, pc.TIE_SP, cuda), pc.tie_want(name, k), (name, k))


@pytest.mark.gpu
@pytest.mark.parametrize("k", pc.LOW_WORD_K)
def test_hip_surface_select_distances_that_differ_in_the_low_word_only(k, cuda, hip_lib):
    """16 squared distances with equal high 32 bits (32 with their exact twins): the low word orders them, the index only the twins."""
    _assert_surface(_surface(*pc.low_word_case(), k, 64, cuda), pc.low_word_want(k), k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", pc.SP_KINDS)
@pytest.mark.parametrize("count", pc.SET_SIZES)
def test_hip_surface_select_set_order_at_table_switches(count, kind, cuda, hip_lib):
    """n_selected on either side of every table switch of the set replay (5, 19, 77, 307), index sets spread out and within one residue class mod 8, 32
    and 128; surface_pts 1, below, equal to and not a multiple of n_selected."""
    partial, coarse, _ = pc.set_case(count)
    _assert_surface(_surface(partial, coarse, 1, pc.surface_pts_of(count, kind), cuda), pc.set_want(count, kind), (count, kind))


@pytest.mark.gpu
def test_hip_surface_select_unique_with_signed_zeros_and_equal_rows(cuda, hip_lib):
    _assert_surface(_surface(*pc.unique_edge_case(), pc.UNIQUE_K, 64, cuda), pc.unique_edge_want(), "np.unique edges")


def _cluster(cloud, eps, min_points, period, cuda, total_pts=1024):
    from seevcn_amd.vcn.utils import sampling as S
    per = None if period is None else torch.tensor([period], dtype=torch.int32, device=cuda)
    out, cnt = S.get_largest_cluster_batch_device(_dev(cloud[None], cuda), eps=eps, min_points=min_points, total_pts=total_pts, period=per)
    assert out.dtype == torch.float32 and cnt.dtype == torch.int32
    return out[0].cpu().numpy(), int(cnt[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pc.cluster_cases()))
def test_hip_largest_cluster_edges(name, cuda, hip_lib):
    """Plain entry against the oracle; for the tiled clouds the periodic entry with the true period as well, bit-identical to the plain one."""
    cloud, eps, min_points, period = pc.cluster_cases()[name]
    for mp in min_points:
        want, size = pc.cluster_want(name, mp)
        got, cnt = _cluster(cloud, eps, mp, None, cuda)
        assert cnt == size and np.array_equal(got.astype(np.float64), want), (name, mp, cnt, size)
        if period is not None:
            pgot, pcnt = _cluster(cloud, eps, mp, period, cuda)
            assert pcnt == cnt and pc.same_bits(pgot, got), (name, mp, "periodic", pcnt, cnt)
    mp = min_points[-1]                                                          # total_pts below, equal to and not a multiple of the cluster size
    size = pc.cluster_want(name, mp)[1]
    for total in sorted({1, max(size - 1, 1), size, size + size // 2 + 1} if len(cloud) <= 300 else {size + 1}):
        if len(cloud) == 1024:                                                   # one oracle run per large cloud: np.tile's rows repeat
            want = pc.cluster_want(name, mp)[0][:size][np.arange(total) % size]
        else:
            want = pc.cluster_want(name, mp, total)[0]
        got, cnt = _cluster(cloud, eps, mp, period, cuda, total)
        assert cnt == size and np.array_equal(got.astype(np.float64), want), (name, mp, total)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["plain", "periodic"])
def test_hip_largest_cluster_all_noise_writes_count_zero_and_nothing_else(entry, cuda, hip_lib):
    """The library entry itself (the wrapper raises): objects 0 and 2 are all noise -> count 0, their output rows and the ints behind n_cluster untouched;
    object 1 between them is complete."""
    import seevcn_amd._lib as L
    clouds, eps, mp = pc.noise_batch()
    B, n, total = clouds.shape[0], clouds.shape[1], 16
    x = _dev(clouds, cuda)
    out = torch.full((B, total, 3), 7.0, dtype=torch.float32, device=cuda)
    cnt = torch.full((B + 4,), -7, dtype=torch.int32, device=cuda)
    if entry == "plain":
        rc = hip_lib.sv_vcn_largest_cluster(L.ptr(x), B, n, eps, mp, total, L.ptr(out), L.ptr(cnt), L.stream())
    else:
        period = torch.tensor([5, 10, 0], dtype=torch.int32, device=cuda)      # hints that do not hold
        rc = hip_lib.sv_vcn_largest_cluster_periodic(L.ptr(x), B, n, L.ptr(period), eps, mp, total, L.ptr(out), L.ptr(cnt), L.stream())
    L.check(rc, "sv_vcn_largest_cluster")
    assert cnt.cpu().tolist() == [0, n, 0, -7, -7, -7, -7]
    got = out.cpu().numpy()
    assert (got[0] == 7.0).all() and (got[2] == 7.0).all()
    assert np.array_equal(got[1].astype(np.float64), opp.largest_cluster(clouds[1], eps=eps, min_points=mp, total_pts=total)[0])
    for name in ("isolated", "n1", "n2_far", "lattice_pure_eps_exact"):       # the single all-noise clouds of the cases: min_points 2 on isolated rows
        cloud, eps, _, _ = pc.cluster_cases()[name]
        x = _dev(cloud[None], cuda)
        out.fill_(7.0), cnt.fill_(-7)
        if entry == "plain":
            rc = hip_lib.sv_vcn_largest_cluster(L.ptr(x), 1, len(cloud), eps, 2, total, L.ptr(out), L.ptr(cnt), L.stream())
        else:
            period = torch.tensor([max(len(cloud) // 2, 1)], dtype=torch.int32, device=cuda)
            rc = hip_lib.sv_vcn_largest_cluster_periodic(L.ptr(x), 1, len(cloud), L.ptr(period), eps, 2, total, L.ptr(out), L.ptr(cnt), L.stream())
        L.check(rc, "sv_vcn_largest_cluster")
        assert cnt.cpu().tolist() == [0] + [-7] * (B + 3) and bool((out == 7.0).all()), name


def _dedup(hip_lib, rows, cuda):
    """sv_dedup_rows in place on a device copy of `rows` -> the tensor."""
    import seevcn_amd._lib as L
    t = _dev(rows, cuda)
    n = t.shape[0]
    scratch = torch.empty((hip_lib.sv_dedup_rows_scratch_bytes(n),), dtype=torch.uint8, device=cuda)
    L.check(hip_lib.sv_dedup_rows(L.ptr(t), n, L.ptr(scratch), L.stream()), "sv_dedup_rows")
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("n", pc.DEDUP_SIZES)
@pytest.mark.parametrize("family", pc.DEDUP_FAMILIES)
def test_hip_dedup_rows_first_copy_survives(family, n, cuda, hip_lib):
    rows = pc.dedup_case(family, n)
    want, flag = pc.dedup_expect(rows)
    t = _dedup(hip_lib, rows, cuda)
    got = t.cpu().numpy()
    assert pc.same_bits(got[:, 1:], rows[:, 1:])                                  # x, y, z are never written
    assert pc.same_bits(got, want), (family, n, "flags differ at", np.nonzero((got[:, 0] == -1) != (want[:, 0] == -1))[0][:8].tolist(), int(flag.sum()))
    again = _dedup(hip_lib, got, cuda).cpu().numpy()                              # a second call on deduplicated rows changes nothing
    assert pc.same_bits(again, got)


def _near(hip_lib, entry, query, ref, thresh, cuda):
    """One of the two library entries on host arrays -> bool (n_query); the bytes behind the result must stay untouched."""
    import seevcn_amd._lib as L
    q, r = _dev(query, cuda), _dev(ref, cuda)
    nq, nr, D = q.shape[0], r.shape[0], q.shape[1]
    near = torch.full((nq + 64,), 7, dtype=torch.uint8, device=cuda)
    qp, rp = (L.ptr(q) if nq else None), (L.ptr(r) if nr else None)
    if entry == "boxed":
        scratch = torch.empty((hip_lib.sv_points_near_set_scratch_bytes(nr),), dtype=torch.uint8, device=cuda)
        rc = hip_lib.sv_points_near_set_boxed(qp, nq, rp, nr, D, float(thresh), L.ptr(scratch), L.ptr(near), L.stream())
    else:
        rc = hip_lib.sv_points_near_set(qp, nq, rp, nr, D, float(thresh), L.ptr(near), L.stream())
    L.check(rc, "sv_points_near_set" + ("_boxed" if entry == "boxed" else ""))
    got = near.cpu().numpy()
    assert (got[nq:] == 7).all() and (got[:nq] <= 1).all()
    return got[:nq].astype(bool)


def _assert_near(hip_lib, entry, row_dim, case, cuda, tag):
    q, r, thresh = pc.rows_of(case, row_dim)
    got, want = _near(hip_lib, entry, q, r, thresh, cuda), pc.near_want(q, r, thresh)
    assert np.array_equal(got, want), (tag, entry, row_dim, "queries that differ", np.nonzero(got != want)[0][:8].tolist())
    return got


NEAR_ENTRIES = pytest.mark.parametrize("entry,row_dim", [("boxed", 3), ("boxed", 4), ("tiled", 3), ("tiled", 4)])


@pytest.mark.gpu
@NEAR_ENTRIES
@pytest.mark.parametrize("name", ["pythagoras_5", "pythagoras_5_next", "tenth", "zero"])
def test_hip_near_set_threshold_is_strict(name, entry, row_dim, cuda, hip_lib):
    """(3, 4, 0) against 5.0 and the next double; the float32 neighbours of 0.1 against 0.1; thresh 0 with queries on reference rows."""
    got = _assert_near(hip_lib, entry, row_dim, pc.near_threshold_cases()[name], cuda, name)
    assert got.any() == (name != "zero")


@pytest.mark.gpu
@NEAR_ENTRIES
@pytest.mark.parametrize("n_ref", pc.NEAR_REF_SIZES)
def test_hip_near_set_sizes_around_the_tiles(n_ref, entry, row_dim, cuda, hip_lib):
    """No reference rows, one, and counts on either side of 128 and 256; no queries, one, 255 and 257.  The only near reference row is the last one:
    alone in the last tile (129, 257), its last row (128, 256) or the last of a partial tile."""
    for n_query in pc.NEAR_QUERY_SIZES:
        got = _assert_near(hip_lib, entry, row_dim, pc.near_size_case(n_ref, n_query), cuda, (n_ref, n_query))
        assert len(got) == n_query and (got.any() and not got.all()) == (n_ref > 0 and n_query > 1)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [pc.NB_TILE, pc.NS_TILE])
@pytest.mark.parametrize("entry", ["boxed", "tiled"])
def test_hip_near_set_dropped_reference_rows(entry, tile, cuda, hip_lib):
    """Reference rows as sv_dedup_rows leaves them: one tile dropped whole, one with its first row dropped, one with only its last row live (laid out
    for the tile of either kernel, each kernel on both).  Rows that arrived dropped lie where nothing is live: no query there is near, and neither is
    any query whose own scene id is -1."""
    before, q = pc.near_dropped_input(tile)
    ref = _dedup(hip_lib, before, cuda).cpu().numpy()
    assert pc.same_bits(ref, pc.dedup_expect(before)[0])
    _assert_near(hip_lib, entry, 4, (q, ref, 0.1), cuda, tile)


@pytest.mark.gpu
@NEAR_ENTRIES
@pytest.mark.parametrize("sort_rows", [True, False])
def test_hip_near_set_scene_seams(sort_rows, entry, row_dim, cuda, hip_lib):
    """A tile that spans three scenes, a query scene absent from a tile whose ids bracket it, queries of scenes without reference rows."""
    _assert_near(hip_lib, entry, row_dim, pc.near_seam_case(sort_rows), cuda, sort_rows)


@pytest.mark.gpu
@NEAR_ENTRIES
@pytest.mark.parametrize("offset", [0.0, 1.0e4])
@pytest.mark.parametrize("sort_rows", [True, False])
def test_hip_near_set_dense_sorted_unsorted_and_far_from_the_origin(sort_rows, offset, entry, row_dim, cuda, hip_lib):
    """1000 reference rows in row order (thin boxes) and shuffled (wide ones), at the origin and moved by 1.0e4, where the float pre-screen of the boxed
    kernel works at coarse float spacing; the two entries must agree with the restatement, hence with each other."""
    case = pc.near_dense_case(sort_rows, offset)
    got = _assert_near(hip_lib, entry, row_dim, case, cuda, (sort_rows, offset))
    q, r, thresh = pc.rows_of(case, row_dim)
    other = _near(hip_lib, "tiled" if entry == "boxed" else "boxed", q, r, thresh, cuda)
    assert np.array_equal(got, other)
