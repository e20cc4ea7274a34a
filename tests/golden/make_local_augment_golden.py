"""Writes tests/golden/local_augment.npz: the reference's own local / frustum augmentors (detector3d/pcdet/datasets/augmentor/augmentor_utils.py
:257-570, imported through _refimport) run on the cases of tests/local_augment_reference.golden_cases() under np.random.seed(case's draw seed),
on the CPU and under the installed NumPy.  The file holds inputs, seeds, ranges and outputs: data only.

    python tests/golden/make_local_augment_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refimport  # noqa: E402
import local_augment_reference as LR  # noqa: E402


def ref_name(name):
    if name.startswith("local_translation_"):
        return "random_local_translation_along_" + name[-1]
    if name.startswith("local_dropout_"):
        return "local_frustum_dropout_" + name.split("_")[-1]
    if name.startswith("world_dropout_"):
        return "global_frustum_dropout_" + name.split("_")[-1]
    return name


def main():
    _refimport.import_pcdet()
    from pcdet.datasets.augmentor import augmentor_utils as ref
    out = {"numpy_version": np.array(np.__version__)}
    for key, case in LR.golden_cases().items():
        if key.endswith("_one_box"):
            continue
        np.random.seed(case["draw_seed"])
        gt, pts = case["boxes"].copy(), case["points"].copy()
        for name, lo, hi in case["specs"]:
            gt, pts = getattr(ref, ref_name(name))(gt, pts, [lo, hi])
        out[key + "/next_uniform"] = np.array(np.random.uniform())   # where the stream stands afterwards
        out[key + "/in_boxes"], out[key + "/in_points"] = case["boxes"], case["points"]
        out[key + "/seed"] = np.array(case["draw_seed"])
        out[key + "/ranges"] = np.array([[lo, hi] for _, lo, hi in case["specs"]])
        out[key + "/out_boxes"], out[key + "/out_points"] = np.asarray(gt), np.asarray(pts)
        assert out[key + "/out_points"].dtype == np.float32 and out[key + "/out_boxes"].dtype == np.float32
    path = os.path.join(HERE, "local_augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
