"""Generate tests/golden/focal_split.npz by running the REFERENCE's own split_voxels -> mask multiply -> combine_out's check_repeat sequence
(backbones_3d/focal_sparse_conv/focal_sparse_utils.py, in the order of focal_sparse_conv.py:145-215) and its FocalLoss on the CPU, on the seeded
inputs and cases of focal_inputs.py.  focal_sparse_utils.py imports torch alone, so it is loaded by its path under _refimport's reference root
(importing the package around it would pull in the image branch's torchvision models).  The generator asserts that the
reference's cell key is injective on every set it dedupes: the key merges distinct voxels otherwise, which is where the library deliberately differs.

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_focal_golden.py
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refimport as R  # noqa: E402
import focal_inputs as I  # noqa: E402

path = os.path.join(R.REF, "detector3d", "pcdet", "models", "backbones_3d", "focal_sparse_conv", "focal_sparse_utils.py")
spec = importlib.util.spec_from_file_location("ref_focal_sparse_utils", path)
fsu = importlib.util.module_from_spec(spec)
spec.loader.exec_module(fsu)

_check_repeat = fsu.check_repeat
deduped = [0]


def check_repeat_injective(features, indices, *args, **kwargs):
    idx = indices[:, 1:].long()
    key = idx[:, 0] * idx[:, 1].max() * idx[:, 2].max() + idx[:, 1] * idx[:, 2].max() + idx[:, 2]
    assert len(torch.unique(key)) == len(torch.unique(idx, dim=0)), "the reference's cell key is not injective on this set"
    deduped[0] += 1
    return _check_repeat(features, indices, *args, **kwargs)


fsu.check_repeat = check_repeat_injective          # split_voxels looks the name up in its module

offsets = [[i, j, k] for i in range(-1, 2) for j in range(-1, 2) for k in range(-1, 2)]
offsets.remove([0, 0, 0])
kernel_offsets = torch.Tensor(offsets)

inp = I.make_inputs()
out = dict(inp)
for case in I.CASES:
    x = SimpleNamespace(indices=torch.from_numpy(inp["coords"]), features=torch.from_numpy(inp["features"]).clone(), spatial_shape=list(I.GRID),
                        batch_size=I.BATCH)
    imps = torch.from_numpy(inp["imps"])
    fore_f, fore_i, back_f, back_i, mask_kernel = [], [], [], [], []
    for b in range(I.BATCH):
        ff, fi, bf, bi, mk = fsu.split_voxels(x, b, imps, None, kernel_offsets, mask_multi=case["mask_multi"], topk=case["topk"],
                                              threshold=case["threshold"])
        fore_f.append(ff), fore_i.append(fi), back_f.append(bf), back_i.append(bi), mask_kernel.append(mk)
    fore_f, fore_i, back_f, back_i, mask_kernel = (torch.cat(v, dim=0) for v in (fore_f, fore_i, back_f, back_i, mask_kernel))
    if not case["skip_mask_kernel"]:
        fore_f = fore_f * mask_kernel.unsqueeze(-1)
    feats, idx = torch.cat([fore_f, back_f], dim=0), torch.cat([fore_i.to(back_i.dtype), back_i], dim=0)
    feats_out, idx_out = [], []
    for b in range(I.BATCH):
        sel = idx[:, 0] == b
        fo, io, _ = fsu.check_repeat(feats[sel], idx[sel], flip_first=False)
        feats_out.append(fo), idx_out.append(io)
    out[case["name"] + "_coords"] = torch.cat(idx_out, dim=0).int().numpy()
    out[case["name"] + "_features"] = torch.cat(feats_out, dim=0).float().numpy()
    print(case["name"], "rows", len(out[case["name"] + "_coords"]), "of", len(inp["coords"]), "inputs")

mv = torch.from_numpy(inp["imps"])[:, -1].sigmoid()
two = torch.cat([1 - mv.unsqueeze(-1), mv.unsqueeze(-1)], dim=1)
out["focal_loss"] = np.float64(fsu.FocalLoss()(two, torch.from_numpy(inp["loss_target"])).double().item())
print("sets deduped", deduped[0], "loss", out["focal_loss"])
path = os.path.join(HERE, "focal_split.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
