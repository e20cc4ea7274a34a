"""FocalSparseConv against the composition of the existing SubMConv3d / BatchNorm1d modules, the host restatement of the expansion
(tests/focal_reference.py) and the restated FocalLoss (held to the reference's golden in tests/test_focal_reference.py)."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

import focal_reference as FR
from seeding import seeded_state_dict

GRID = (5, 9, 23)
BATCH = 2
C = 16
# one ground-truth box per scene over the default z-first range / voxel size of the module (x = 0.05 ix, y = 0.05 iy - 40, z = 0.1 iz - 3), heading 0,
# its faces at least 0.01 from every voxel position
GT = np.array([[[0.5, -39.8, -2.8, 0.52, 0.23, 0.25, 0.0, 1.0]], [[0.8, -39.7, -2.9, 0.32, 0.13, 0.25, 0.0, 1.0]]], np.float32)


def _inputs():
    rng = np.random.RandomState(5)
    cells = [(b, z, y, x) for b in range(BATCH) for z in range(GRID[0]) for y in range(GRID[1]) for x in range(GRID[2])]
    coords = np.array([cells[i] for i in rng.choice(len(cells), 150, replace=False)], np.int32)
    return coords, rng.randn(len(coords), C).astype(np.float32)


def _inside_boxes(coords):
    xyz = np.stack([coords[:, 3] * 0.05, coords[:, 2] * 0.05 - 40, coords[:, 1] * 0.1 - 3], axis=1)
    box = GT[coords[:, 0], 0]
    return (np.abs(xyz - box[:, :3]) <= box[:, 3:6] / 2).all(axis=1)


def _expected_keys(enlarge):
    keys = {"conv.weight": (C, 3, 3, 3, C), "bn1.weight": (C,), "bn1.bias": (C,), "bn1.running_mean": (C,), "bn1.running_var": (C,),
            "bn1.num_batches_tracked": (), "conv_imp.weight": (27, 3, 3, 3, enlarge if enlarge > 0 else C)}
    if enlarge > 0:
        keys.update({"conv_enlarge.0.weight": (enlarge, 3, 3, 3, C), "conv_enlarge.1.weight": (enlarge,), "conv_enlarge.1.bias": (enlarge,),
                     "conv_enlarge.1.running_mean": (enlarge,), "conv_enlarge.1.running_var": (enlarge,), "conv_enlarge.1.num_batches_tracked": ()})
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("enlarge", [-1, 32], ids=["plain", "enlarge32"])
def test_hip_focal_sparse_conv_matches_composition(cuda, hip_lib, enlarge, train):
    import seevcn_amd.spconv as spconv
    from oracle.tolerances import assert_close_per_channel
    from seevcn_amd.pcdet.models.backbones_3d.focal_sparse_conv import FocalSparseConv
    norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    topk, thr, mask_multi = True, 0.5, True
    m = FocalSparseConv(C, C, voxel_stride=1, norm_fn=norm_fn, indice_key="focal1", topk=topk, threshold=thr, mask_multi=mask_multi,
                        enlarge_voxel_channels=enlarge)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == _expected_keys(enlarge)
    assert m.conv.indice_key == "focal1" and m.conv_imp.indice_key == "focal1_imp" and (enlarge < 0 or m.conv_enlarge[0].indice_key == "focal1_enlarge")
    sd = seeded_state_dict(m, seed=31)
    m.load_state_dict(sd)
    m = m.to(cuda).train(train)
    coords, f = _inputs()
    idx = torch.from_numpy(coords).to(cuda)
    batch_dict = {"batch_size": BATCH, "gt_boxes": torch.from_numpy(GT).to(cuda)}

    # ---- ours
    fd = torch.from_numpy(f).to(cuda).requires_grad_(True)
    out, bd, loss = m(spconv.SparseConvTensor(fd, idx, list(GRID), BATCH), batch_dict)
    assert bd is batch_dict and out.indices.dtype == torch.int32
    rng = np.random.RandomState(9)
    g = torch.from_numpy(rng.randn(*out.features.shape).astype(np.float32)).to(cuda)
    total = (out.features * g).sum() + loss
    total.backward()
    mine = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}
    assert set(mine) == {k for k in _expected_keys(enlarge) if "running" not in k and "tracked" not in k}

    # ---- the composition: existing modules with the same weights, the expansion restated on the host in float64
    parts = {"conv": spconv.SubMConv3d(C, C, 3, bias=False, indice_key="a"), "bn1": norm_fn(C),
             "conv_imp": spconv.SubMConv3d(enlarge if enlarge > 0 else C, 27, 3, padding=1, bias=False, indice_key="b")}
    if enlarge > 0:
        parts["conv_enlarge"] = spconv.SparseSequential(spconv.SubMConv3d(C, enlarge, 3, padding=1, bias=False, indice_key="c"), norm_fn(enlarge), nn.ReLU())
    ref = nn.ModuleDict(parts)
    ref.load_state_dict(sd)
    ref = ref.to(cuda).train(train)
    fr = torch.from_numpy(f).to(cuda).requires_grad_(True)
    x = spconv.SparseConvTensor(fr, idx, list(GRID), BATCH)
    xp = ref["conv_enlarge"](x) if enlarge > 0 else x
    s = ref["conv_imp"](xp).features.sigmoid()
    s_host = s.double().cpu()
    ex = FR.expand(s.detach().cpu().numpy(), coords, GRID, BATCH, topk, thr)
    expanded = FR.torch_features(fr.double().cpu(), s_host, ex, mask_multi, False).float().to(cuda)
    y = ref["conv"](spconv.SparseConvTensor(expanded, torch.from_numpy(ex["out_coords"]).to(cuda), list(GRID), BATCH))
    want_feats = torch.relu(ref["bn1"](y.features))
    want_loss = 0
    if train:
        mv = s_host[:, 26]
        want_loss = FR.torch_focal_loss(torch.stack([1 - mv, mv], dim=1), torch.from_numpy(_inside_boxes(coords)))
        assert abs(float(want_loss.detach()) - FR.focal_loss(torch.stack([1 - mv, mv], dim=1).detach().numpy(), _inside_boxes(coords))) < 1e-12
        assert 0 < _inside_boxes(coords).sum() < len(coords)
    ((want_feats * g).sum() + (want_loss.float().to(cuda) if train else 0)).backward()

    assert len(ex["out_coords"]) > len(coords) and np.array_equal(out.indices.cpu().numpy(), ex["out_coords"])
    assert_close_per_channel(out.features.detach().cpu().numpy(), want_feats.detach().cpu().numpy(), rtol=1e-3, atol_frac=1e-4, name="features")
    if train:
        assert abs(float(loss) - float(want_loss)) <= 1e-5 * abs(float(want_loss)), (float(loss), float(want_loss))
    else:
        assert loss == 0
    assert_close_per_channel(fd.grad.cpu().numpy(), fr.grad.cpu().numpy(), rtol=2e-3, atol_frac=2e-4, name="input gradient")
    for k, p in ref.named_parameters():
        assert_close_per_channel(mine[k], p.grad.cpu().numpy(), rtol=2e-3, atol_frac=2e-3, name="grad " + k)
        assert np.abs(mine[k]).sum() > 0, k
    for k, b in ref.named_buffers():                                   # running statistics moved the same way (or not at all in eval mode)
        np.testing.assert_allclose(m.state_dict()[k].cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


def test_focal_sparse_conv_refuses_what_is_not_built():
    from seevcn_amd.pcdet.models.backbones_3d.focal_sparse_conv import FocalSparseConv
    norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    with pytest.raises(NotImplementedError, match="DeepLabV3"):
        FocalSparseConv(16, 16, voxel_stride=1, norm_fn=norm_fn, indice_key="f", use_img=True)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        FocalSparseConv(16, 16, voxel_stride=1, norm_fn=norm_fn, indice_key="f", kernel_size=5, padding=2)
