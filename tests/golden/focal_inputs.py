"""Seeded inputs and the case list of the focal sparse conv golden (make_focal_golden.py, tests/test_focal_reference.py)."""
import numpy as np

GRID = (5, 9, 8)            # Z, Y, X
BATCH = 2
CHANNELS = 16
ROWS = (30, 31)             # voxels per scene: 31 * 0.5 = 15.5 -> 15, 31 * 0.3 = 9.3 -> 9
SEED = 20


def _case(topk, mask_multi, skip_mask_kernel, threshold):
    name = f"{'topk' if topk else 'thr'}{int(round(threshold * 10)):02d}_mm{int(mask_multi)}_sk{int(skip_mask_kernel)}"
    return dict(name=name, topk=topk, mask_multi=mask_multi, skip_mask_kernel=skip_mask_kernel, threshold=threshold)


CASES = [_case(t, m, k, 0.5) for t in (True, False) for m in (False, True) for k in (False, True)] + [_case(True, True, False, 0.3),
                                                                                                     _case(False, True, False, 0.3)]


def make_inputs(seed=SEED):
    """coords (n, 4) int32 [b, z, y, x] with y, x >= 1 (where the reference's cell key is injective), rows shuffled across scenes; features (n, C)
    N(0, 1); imps (n, 27) logits (column 26: the voxel importance), distinct within a scene; loss_target (n) 0 / 1."""
    rng = np.random.RandomState(seed)
    Z, Y, X = GRID
    rows = []
    for b, n in enumerate(ROWS):
        cells = [(z, y, x) for z in range(Z) for y in range(1, Y) for x in range(1, X)]
        pick = rng.choice(len(cells), n, replace=False)
        rows += [(b,) + cells[i] for i in pick]
    coords = np.array(rows, np.int32)[rng.permutation(len(rows))]
    feats = rng.randn(len(rows), CHANNELS).astype(np.float32)
    imps = (1.5 * rng.randn(len(rows), 27)).astype(np.float32)
    for b in range(BATCH):
        mv = imps[coords[:, 0] == b, 26]
        assert len(np.unique(mv)) == len(mv)
    target = (rng.rand(len(rows)) < 0.3).astype(np.int64)
    return dict(coords=coords, features=feats, imps=imps, loss_target=target)
