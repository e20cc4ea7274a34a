"""The restatement of the focal sparse conv expansion (tests/focal_reference.py) against the golden the reference's own split_voxels / check_repeat
/ FocalLoss produced (tests/golden/make_focal_golden.py), and its behaviour where the reference's cell key stops being injective."""
import os

import numpy as np
import pytest
import torch

import focal_inputs as I
import focal_reference as FR


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "focal_split.npz"))


def _sigmoid(imps):
    return torch.from_numpy(imps).sigmoid().numpy()           # torch's fp32 sigmoid: the numbers the reference thresholds


@pytest.mark.parametrize("case", I.CASES, ids=[c["name"] for c in I.CASES])
def test_restatement_matches_reference_golden(golden, case):
    """Coordinates and order equal; every feature within 64 * 2^-24 of the float64 restatement's magnitude of that element: at most 27 fp32 adds, one
    divide and two multiplies on the reference's side stay under about 30 ulp (measured on these inputs: <= 1.8e-7 absolute on N(0, 1) features, 0.05 of the bound)."""
    inp = I.make_inputs()
    for k in ("coords", "features", "imps"):
        assert np.array_equal(inp[k], golden[k]), k
    s = _sigmoid(inp["imps"])
    ex = FR.expand(s, inp["coords"], I.GRID, I.BATCH, case["topk"], case["threshold"])
    want_coords, want = golden[case["name"] + "_coords"], golden[case["name"] + "_features"]
    assert np.array_equal(ex["out_coords"], want_coords)
    out, _, _ = FR.features(inp["features"], s, ex, case["mask_multi"], case["skip_mask_kernel"])
    err = np.abs(out - want.astype(np.float64))
    print(case["name"], "rows", len(want), "max abs err", err.max(), "max err / bound", (err / np.maximum(64 * 2.0 ** -24 * np.abs(out), 1e-300)).max())
    assert (err <= 64 * 2.0 ** -24 * np.abs(out)).all()
    # the fp32 mode of the restatement holds the same bound
    out32, _, _ = FR.features(inp["features"], s, ex, case["mask_multi"], case["skip_mask_kernel"], dtype=np.float32)
    assert (np.abs(out32 - out) <= 64 * 2.0 ** -24 * np.abs(out)).all()


def test_restatement_selection_counts(golden):
    """int(n_b * threshold) per scene, and the strict / non-strict compares, on the golden's inputs."""
    inp = I.make_inputs()
    s = _sigmoid(inp["imps"])
    for thr in (0.5, 0.3):
        fore = FR.select(s, inp["coords"], I.BATCH, True, thr)
        for b, n in enumerate(I.ROWS):
            assert fore[inp["coords"][:, 0] == b].sum() == int(n * thr)
        assert np.array_equal(FR.select(s, inp["coords"], I.BATCH, False, thr), s[:, 26] > np.float32(thr))
    assert int(0.29 * 100) == 28 and FR.select(np.tile(np.linspace(0.1, 0.9, 100, dtype=np.float32)[:, None], (1, 27)),
                                                   np.zeros((100, 4), np.int32) + np.arange(100, dtype=np.int32)[:, None] * [0, 0, 0, 1], 1, True, 0.29).sum() == 28


def test_focal_loss_matches_reference_golden(golden):
    inp = I.make_inputs()
    mv = _sigmoid(inp["imps"])[:, 26].astype(np.float64)
    mine = FR.focal_loss(np.stack([1 - mv, mv], axis=1), inp["loss_target"])
    want = float(golden["focal_loss"])
    print("loss", mine, want)
    assert abs(mine - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("topk", [True, False])
def test_restatement_keeps_every_voxel_at_coordinate_zero(topk):
    """Input voxels at y = 0 and x = 0, where the reference's key merges distinct voxels: every input coordinate appears exactly once in the output and
    no candidate has a coordinate 0."""
    rng = np.random.RandomState(3)
    Z, Y, X = 5, 9, 8
    cells = [(b, z, y, x) for b in range(2) for z in range(Z) for y in range(Y) for x in range(X)]
    coords = np.array([cells[i] for i in rng.choice(len(cells), 120, replace=False)], np.int32)
    assert (coords[:, 2] == 0).any() and (coords[:, 3] == 0).any() and (coords[:, 1] == 0).any()
    s = _sigmoid((1.5 * rng.randn(len(coords), 27)).astype(np.float32))
    ex = FR.expand(s, coords, (Z, Y, X), 2, topk, 0.5)
    out_keys, in_keys = FR.linear_key(ex["out_coords"], (Z, Y, X)), FR.linear_key(coords, (Z, Y, X))
    assert (np.diff(out_keys) > 0).all()                                        # canonical order, each cell once
    assert np.array_equal(out_keys[ex["row_of_in"]], in_keys)                   # every input voxel is there, at the row row_of_in names
    new = np.setdiff1d(out_keys, in_keys)
    assert len(new) > 0 and len(out_keys) == len(in_keys) + len(new)
    new_coords = ex["out_coords"][np.isin(out_keys, new)]
    assert (new_coords[:, 1:] > 0).all()
    _, _, cand = FR.candidates(s, coords, ex["fore"], (Z, Y, X), 0.5)
    assert len(cand) and (cand[:, 1:] > 0).all()
    f = rng.randn(len(coords), 4)
    out, w, cnt = FR.features(f, s, ex, False, False)
    assert np.array_equal(out[ex["row_of_in"]], f * w[:, None]) and not out[np.isin(out_keys, new)].any()
    assert (cnt[~ex["fore"]] == 0).all() and cnt.max() >= 2
