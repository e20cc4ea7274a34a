"""Makes tests/golden/pyramid_augment.npz: the reference's own local_pyramid_dropout / local_pyramid_sparsify / local_pyramid_swap
(detector3d/pcdet/datasets/augmentor/augmentor_utils.py:573-762, imported through _refimport; scipy's Delaunay behind in_hull) under
np.random.seed, on the cases of tests/pyramid_augment_reference.py.  Data only: per case the inputs as the entry sees them (the box rows that
exist, the points that are alive), the seed and the five settings, the reference's pyramids, its Delaunay membership of every point in every
pyramid (bit-packed), the points after each of the three functions, and the next uniform() of the stream.  Dropout and sparsify only select and repeat input
rows, so their outputs are kept as row numbers of the input (checked here to reproduce the reference's arrays bit for bit); the swap's output
is kept whole.  For the C = 3 swap case: that the
reference raises.

    python tests/golden/make_pyramid_augment_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refimport  # noqa: E402
import pyramid_augment_reference as PR  # noqa: E402


def _rows(points, out):
    """The input row each output row is a copy of (the inputs' rows are distinct)."""
    key = {r.tobytes(): i for i, r in enumerate(points)}
    assert len(key) == len(points)
    idx = np.array([key[r.tobytes()] for r in out], np.int32).reshape(-1)
    assert np.array_equal(points[idx].view(np.uint32), out.view(np.uint32))
    return idx


def main():
    _refimport.import_pcdet()
    from pcdet.datasets.augmentor import augmentor_utils as ref
    cases = PR.cases()
    out = {"names": np.array(PR.GOLDEN_CASES), "discarded": np.array([PR.TALLY.discarded, PR.TALLY.drawn], np.int64)}
    for name in PR.GOLDEN_CASES:
        c = cases[name]
        boxes = c["boxes"][c["cls"] != -2][:, :7].copy()
        points = c["points"][~c["dead"]].copy()
        cfg = c["cfg"]
        pyramids = ref.get_pyramids(boxes)
        assert pyramids.dtype == np.float32
        masks = ref.points_in_pyramids_mask(points, pyramids) if len(boxes) else np.zeros((len(points), 0), bool)
        np.random.seed(c["seed"])
        _, p1, pyr = ref.local_pyramid_dropout(boxes.copy(), points.copy(), cfg["DROP_PROB"])
        _, p2, pyr = ref.local_pyramid_sparsify(boxes.copy(), p1, cfg["SPARSIFY_PROB"], cfg["SPARSIFY_MAX_NUM"], pyr)
        _, p3 = ref.local_pyramid_swap(boxes.copy(), p2, cfg["SWAP_PROB"], cfg["SWAP_MAX_NUM"], pyr)
        nxt = np.random.uniform()
        for arr in (p1, p2, p3):
            assert arr.dtype == np.float32
        out.update({f"{name}/boxes": boxes, f"{name}/points": points, f"{name}/seed": np.int64(c["seed"]),
                    f"{name}/cfg": np.array([cfg[k] for k in ("DROP_PROB", "SPARSIFY_PROB", "SPARSIFY_MAX_NUM", "SWAP_PROB", "SWAP_MAX_NUM")], np.float64),
                    f"{name}/pyramids": pyramids.reshape(-1, 6, 15), f"{name}/masks": np.packbits(masks, axis=1),
                    f"{name}/after_dropout_rows": _rows(points, p1), f"{name}/after_sparsify_rows": _rows(points, p2), f"{name}/after_swap": p3, f"{name}/next_uniform": np.float64(nxt)})
        print(f"{name}: {len(points)} points, {len(boxes)} boxes -> {len(p1)} / {len(p2)} / {len(p3)}")
    c = cases["columns3_swap"]
    np.random.seed(c["seed"])
    try:
        ref.local_pyramid_swap(c["boxes"].copy(), c["points"].copy(), c["cfg"]["SWAP_PROB"], c["cfg"]["SWAP_MAX_NUM"])
        raised = ""
    except ValueError as e:
        raised = type(e).__name__
    out["columns3_swap/raised"] = np.array(raised)
    path = os.path.join(HERE, "pyramid_augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; band discards", PR.TALLY.discarded, "of", PR.TALLY.drawn)


if __name__ == "__main__":
    main()
