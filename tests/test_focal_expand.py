"""The sv_focal_* entries (selection, mark / count / emit, weigh and place, backward) against the restatement in tests/focal_reference.py, on a
grid whose scene boundary falls inside a 32-cell word and past a 1024-cell chunk of the coordinate index, with the rows that can go wrong
crafted in: candidates leaving through every face, coordinate 0, shared cells, ties and values exactly at the threshold."""
import itertools

import numpy as np
import pytest
import torch

import focal_reference as FR

GRID = (5, 9, 23)            # 1035 cells per scene
BATCH = 3                    # scene 1 is empty
T5, T3 = np.float32(0.5), np.float32(0.3)


def _below(v):
    return np.nextafter(np.float32(v), np.float32(0))


def _make_inputs(kind):
    """kind 'main': scenes 0 and 2 with 75 rows each; 'single': scene 2 has ONE voxel (k_b = 0 in top-k mode).  -> coords, s, info"""
    rng = np.random.RandomState(11 if kind == "main" else 12)
    Z, Y, X = GRID
    hi = lambda: np.full(27, 0.9, np.float32)
    crafted = {                                               # scene 0: cell -> (mv, kernel importances or None for random)
        (0, 0, 0): (0.990, hi()),                             # candidates leave through the three low faces or land on coordinate 0: only (1, 1, 1) stays
        (4, 8, 22): (0.989, hi()),                            # ... through the three high faces
        (1, 1, 1): (0.988, hi()),                             # candidates landing on coordinate 0 are dropped
        (2, 4, 10): (0.987, hi()),                            # P: foreground, hit by the three below (and hits them)
        (2, 4, 9): (0.986, hi()), (2, 3, 10): (0.985, hi()), (3, 4, 10): (0.984, hi()),
        (2, 4, 12): (0.010, hi()),                            # Q: background, hit by (2, 4, 11)
        (2, 4, 11): (0.983, hi()),
        (2, 7, 17): (0.982, None),                            # kernel importances exactly at and just below both thresholds (set below)
    }
    taken = set(crafted) | {(3, 3, 10)}                       # (3, 3, 10) stays free: a new cell hit by P, (2, 3, 10) and (3, 4, 10)
    rows, mv, ker = [], [], []
    for cell, (m, k) in crafted.items():
        rows.append((0,) + cell), mv.append(m), ker.append(k if k is not None else rng.uniform(0.05, 0.95, 27).astype(np.float32))
    ker[-1][:4] = [T5, _below(T5), T3, _below(T3)]
    free = [c for c in itertools.product(range(Z), range(Y), range(X)) if c not in taken]
    for b, n in ((0, 75 - len(crafted)), (2, 75 if kind == "main" else 1)):
        for i in rng.choice(len(free), n, replace=False):
            rows.append((b,) + free[i]), ker.append(rng.uniform(0.05, 0.95, 27).astype(np.float32))
        mv += list(rng.permutation(np.linspace(0.05, 0.95, n)))          # distinct
    coords, s = np.array(rows, np.int32), np.stack(ker).astype(np.float32)
    s[:, 26] = np.array(mv, np.float32)
    # values exactly at the thresholds among the random rows of scene 0, and equal values around both top-k boundaries of the last scene with >= 8 rows
    plain = np.arange(len(crafted), 75)
    s[plain[0], 26], s[plain[1], 26] = T5, T3
    tie_scene = 2 if kind == "main" else 0
    members = np.nonzero(coords[:, 0] == tie_scene)[0]
    order = members[np.argsort(-s[members, 26], kind="stable")]
    for thr in (0.5, 0.3):
        k = int(len(members) * thr)
        s[order[k - 2:k + 2], 26] = s[order[k - 2], 26]        # four equal values, two of them inside the top k
    perm = rng.permutation(len(coords))
    return coords[perm], s[perm]


@pytest.fixture(scope="module", params=["main", "single"])
def inputs(request):
    coords, s = _make_inputs(request.param)
    return request.param, coords, s


@pytest.fixture(scope="module")
def expected(inputs):
    """The restatement's structure, computed once per input set and mode and shared by the tests."""
    _, coords, s = inputs
    cache = {}

    def get(topk, thr):
        if (topk, thr) not in cache:
            cache[(topk, thr)] = FR.expand(s, coords, GRID, BATCH, topk, thr)
        return cache[(topk, thr)]
    return get


MODES = [(True, 0.5), (True, 0.3), (False, 0.5), (False, 0.3)]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def test_crafted_rows_are_what_they_claim(inputs, expected):
    """CPU: the crafted situations are present in the inputs (judged by the restatement)."""
    kind, coords, s = inputs
    row = {tuple(c): i for i, c in enumerate(coords.tolist())}
    for topk, thr in MODES:
        ex = expected(topk, thr)
        fore = ex["fore"]
        _, _, cnt = FR.features(np.zeros((len(coords), 1)), s, ex, False, False)
        J, O, cand = FR.candidates(s, coords, fore, GRID, thr)
        raw = [(j, o) for j in np.nonzero(fore)[0] for o in range(26) if s[j, o] >= np.float32(thr)]
        dropped = [coords[j, 1:] + FR.OFFSETS[o] for j, o in raw if (j, o) not in set(zip(J.tolist(), O.tolist()))]
        dropped = np.array(dropped)
        for axis, dim in enumerate(GRID):                      # a candidate leaves through each of the six faces, and one lands on coordinate 0
            assert (dropped[:, axis] == -1).any() and (dropped[:, axis] == dim).any() and (dropped[:, axis] == 0).any()
        assert fore[row[(0, 2, 4, 10)]] and cnt[row[(0, 2, 4, 10)]] >= 3
        q = row[(0, 2, 4, 12)]
        assert not fore[q] and (FR.linear_key(cand, GRID) == FR.linear_key(coords[q:q + 1], GRID)[0]).sum() >= 1
        assert (0, 3, 3, 10) not in row and (FR.linear_key(cand, GRID) == FR.linear_key(np.array([[0, 3, 3, 10]]), GRID)[0]).sum() >= 3
        e = row[(0, 2, 7, 17)]
        kept = set(O[J == e].tolist())
        assert fore[e] and kept & {0, 1, 2, 3} == ({0} if thr == 0.5 else {0, 1, 2})                          # >= at the threshold, not just below it
        if not topk:
            assert (s[:, 26] == np.float32(thr)).any() and not fore[s[:, 26] == np.float32(thr)].any()        # mv exactly at the threshold: strict >
        else:
            tie_scene = 2 if kind == "main" else 0
            members = np.nonzero(coords[:, 0] == tie_scene)[0]
            boundary = np.sort(s[members, 26])[::-1][int(len(members) * thr) - 1]
            tied = members[s[members, 26] == boundary]
            assert len(tied) == 4 and fore[tied].sum() == 2 and fore[tied[:2]].all()                            # lower row index first
            if kind == "single":
                assert (coords[:, 0] == 2).sum() == 1 and not fore[coords[:, 0] == 2].any()                     # k_b = int(1 * thr) = 0
        assert not (coords[:, 0] == 1).any()


def _device_inputs(coords, s, cuda):
    import seevcn_amd.spconv.functional as Fsp
    idx = torch.from_numpy(coords).to(cuda)
    rb = Fsp.build_subm_rulebook(idx, BATCH, list(GRID), [3, 3, 3])
    return idx, torch.from_numpy(s).to(cuda), rb.nbr_out


def _index_words_zero(cuda):
    """words and chunk counts of the grid's coordinate-index workspace (chunk_base is scan output, rewritten by every user)"""
    from seevcn_amd.spconv import focal
    ws, ncells = focal.index_workspace(BATCH, GRID, cuda)
    nchunks = (ncells + 1023) // 1024
    return not bool(ws[:nchunks * 32 * 8 + nchunks * 4].any())


@pytest.mark.gpu
@pytest.mark.parametrize("topk,thr", MODES)
def test_hip_focal_select_and_cells_bit_exact(inputs, expected, cuda, hip_lib, topk, thr):
    from seevcn_amd.spconv import focal
    _, coords, s = inputs
    ex = expected(topk, thr)
    idx, sd, _ = _device_inputs(coords, s, cuda)
    fore = focal.focal_select(sd, idx, BATCH, topk, thr)
    assert np.array_equal(fore.cpu().numpy().astype(bool), ex["fore"])
    out_coords, row_of_in, n_out = focal.focal_cells(idx, sd, fore, BATCH, GRID, thr)
    assert n_out == len(ex["out_coords"]) and out_coords.dtype == torch.int32
    assert np.array_equal(out_coords.cpu().numpy(), ex["out_coords"])
    assert np.array_equal(row_of_in.cpu().numpy(), ex["row_of_in"])
    assert _index_words_zero(cuda)
    # a capacity below the size of the set: an error, and nothing written past it
    cap = n_out - 7
    buf = torch.full((n_out + 5, 4), -77, dtype=torch.int32, device=cuda)
    with pytest.raises(Exception, match="capacity"):
        focal.focal_cells(idx, sd, fore, BATCH, GRID, thr, capacity=cap, out_coords=buf)
    got = buf.cpu().numpy()
    assert (got[cap:] == -77).all() and np.array_equal(got[:cap], ex["out_coords"][:cap])
    assert _index_words_zero(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [5, 16, 64])
def test_hip_focal_expand_features_and_gradients(inputs, expected, cuda, hip_lib, channels):
    """Features within 32 * 2^-24 * |value| of the float64 restatement (at most 26 fp32 adds, a divide and two multiplies).  Gradients against autograd
    on the torch-double restatement within (C + 32) * 2^-24 * sum|terms| per element: an fp32 sum of C products has error <= C * 2^-24 * sum|terms|
    whatever its order, the factors mv, w and 1 / (1 + c) add a few ulp each; sum|terms| is the same gradient taken with |f| and |g| (every other factor
    is positive).  Two runs are bit-identical, forward and backward."""
    from seevcn_amd.spconv import focal
    import seevcn_amd.spconv as spconv
    _, coords, s = inputs
    rng = np.random.RandomState(channels)
    f = rng.randn(len(coords), channels).astype(np.float32)
    idx, sd, nbr = _device_inputs(coords, s, cuda)
    for (topk, thr), (mask_multi, skip) in itertools.product(MODES, FLAGS):
        ex = expected(topk, thr)
        want, _, _ = FR.features(f, s, ex, mask_multi, skip)
        g = rng.randn(*want.shape).astype(np.float32)
        runs = []
        for _ in range(2):
            fd, sdd = torch.from_numpy(f).to(cuda).requires_grad_(True), sd.clone().requires_grad_(True)
            x = spconv.SparseConvTensor(fd, idx, list(GRID), BATCH)
            out, fore, row_of_in = focal.focal_expand(x, sdd, nbr, topk=topk, threshold=thr, mask_multi=mask_multi, skip_mask_kernel=skip)
            out.features.backward(torch.from_numpy(g).to(cuda))
            runs.append([t.detach().cpu().numpy() for t in (out.features, out.indices, fd.grad, sdd.grad)])
        for a, b in zip(*runs):
            assert np.array_equal(a, b)
        feats, out_idx, grad_f, grad_s = runs[0]
        assert out.indices.dtype == torch.int32 and out.spatial_shape == list(GRID) and out.indice_dict is x.indice_dict
        assert np.array_equal(out_idx, ex["out_coords"]) and np.array_equal(fore.cpu().numpy().astype(bool), ex["fore"])
        tag = (topk, thr, mask_multi, skip, channels)
        err = np.abs(feats - want)
        assert (err <= 32 * 2.0 ** -24 * np.abs(want)).all(), (tag, err.max())
        grads = []
        for ff, gg in ((f, g), (np.abs(f), np.abs(g))):
            ft, st = torch.from_numpy(ff).double().requires_grad_(True), torch.from_numpy(s).double().requires_grad_(True)
            FR.torch_features(ft, st, ex, mask_multi, skip).backward(torch.from_numpy(gg).double())
            grads.append((ft.grad.numpy(), st.grad.numpy() if st.grad is not None else np.zeros_like(s, np.float64)))      # None: s plays no part
        (want_f, want_s), (mag_f, mag_s) = grads
        bound = (channels + 32) * 2.0 ** -24
        assert (np.abs(grad_f - want_f) <= bound * mag_f).all(), (tag, "grad_f", np.abs(grad_f - want_f).max())
        assert (np.abs(grad_s[:, :26] - want_s[:, :26]) <= bound * mag_s[:, :26]).all(), (tag, "grad_s", np.abs(grad_s - want_s).max())
        assert (np.abs(grad_s[:, 26] - want_s[:, 26]) <= bound * mag_s[:, 26]).all(), (tag, "grad_mv", np.abs(grad_s[:, 26] - want_s[:, 26]).max())
        if not skip:
            assert np.abs(want_s[:, :26]).sum() > 0
        assert (np.abs(want_s[:, 26]).sum() > 0) == mask_multi
    assert _index_words_zero(cuda)


@pytest.mark.gpu
def test_hip_focal_refuses_cpu_tensors(inputs, hip_lib):
    import seevcn_amd._lib as L
    from seevcn_amd.spconv import focal
    import seevcn_amd.spconv as spconv
    _, coords, s = inputs
    idx, sd = torch.from_numpy(coords), torch.from_numpy(s)
    with pytest.raises(L.SeevcnHipError):
        focal.focal_select(sd, idx, BATCH, True, 0.5)
    with pytest.raises(L.SeevcnHipError):
        focal.focal_cells(idx, sd, torch.zeros(len(idx), dtype=torch.uint8), BATCH, GRID, 0.5)
    x = spconv.SparseConvTensor(torch.zeros(len(idx), 4), idx, list(GRID), BATCH)
    with pytest.raises(L.SeevcnHipError):
        focal.focal_expand(x, sd, torch.zeros((27, len(idx)), dtype=torch.int32), topk=True)
