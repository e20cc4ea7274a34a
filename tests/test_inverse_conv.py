"""spconv.SparseInverseConv3d against the float64 restatement of tests/unet_reference.py over the oracle's rulebook of the paired strided layer:
values, both gradients, output sites, the conv + BatchNorm fusion, the parameter's name and shape, the error for a key without a strided
rulebook, and that the mirrored rulebook shares the paired rulebook's tables and plan objects."""
import functools

import numpy as np
import pytest
import torch

import unet_reference as UR
from oracle import spconv as osp
from oracle.tolerances import assert_close_per_channel

GRID = [9, 10, 11]
# kernel, stride, padding of the paired strided layer
GEOMS = {"k3s2p1": (3, 2, 1), "unet_pad011": (3, 2, (0, 1, 1)), "k311s211": ((3, 1, 1), (2, 1, 1), 0)}
# (C_in, C_out) of the inverse layer: the first three run on the planned kernel, 8 -> 24 on the plain one
CHANNELS = [(64, 32), (32, 16), (64, 64), (8, 24)]


@functools.lru_cache(maxsize=None)
def _sites():
    """Two scenes, about 200 active sites on GRID, rows in a seeded random order."""
    rng = np.random.default_rng(5)
    rows = []
    for b in range(2):
        occ = np.argwhere(rng.uniform(size=GRID) < 0.1)
        occ = occ[rng.permutation(len(occ))]
        rows.append(np.concatenate([np.full((len(occ), 1), b), occ], 1))
    return np.concatenate(rows).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _want(geom, cin, cout, bias):
    """Seeded inputs and the float64 forward / gradients of the inverse layer alone."""
    k, s, p = GEOMS[geom]
    coords = _sites()
    out_coords, nbr_out, nbr_in, oshape = osp.rulebook_sparse(coords, GRID, k, s, p)
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    kk = osp._triple(k)
    weight = (torch.randn((cout, *kk, cin), generator=g) / np.sqrt(cin * 4)).float()
    b = torch.randn((cout,), generator=g).float() if bias else None
    u = torch.randn((len(out_coords), cin), generator=g).float()
    gz = torch.randn((len(coords), cout), generator=g).float()
    u64, w64 = u.double().requires_grad_(True), weight.double().requires_grad_(True)
    z = UR.inverse_conv(u64, nbr_out, len(coords), w64, b)
    z.backward(gz.double())
    return dict(coords=coords, out_coords=out_coords, weight=weight, bias=b, u=u, gz=gz, z=z.detach().numpy(), gu=u64.grad.numpy(), gw=w64.grad.numpy())


def _layers(cuda, geom, cin, cout, bias, w):
    import seevcn_amd.spconv as spconv
    k, s, p = GEOMS[geom]
    down = spconv.SparseConv3d(cout, cin, k, stride=s, padding=p, bias=False, indice_key="sp").to(cuda)
    inv = spconv.SparseInverseConv3d(cin, cout, k, indice_key="sp", bias=bias).to(cuda)
    with torch.no_grad():
        inv.weight.copy_(w["weight"].to(cuda))
        if bias:
            inv.bias.copy_(w["bias"].to(cuda))
    return down, inv


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_parameter_name_and_shape():
    import seevcn_amd.spconv as spconv
    inv = spconv.SparseInverseConv3d(64, 32, 3, indice_key="spconv3", bias=False)
    assert isinstance(inv, spconv.SparseConvolution) and inv.inverse and not inv.subm
    assert {k: tuple(v.shape) for k, v in inv.state_dict().items()} == {"weight": (32, 3, 3, 3, 64)}
    biased = spconv.SparseInverseConv3d(8, 24, (3, 1, 1), indice_key="k")
    assert {k: tuple(v.shape) for k, v in biased.state_dict().items()} == {"weight": (24, 3, 1, 1, 8), "bias": (24,)}
    with pytest.raises(AssertionError):
        spconv.SparseInverseConv3d(8, 8, 3)                                   # no indice_key: nothing to undo


def test_missing_rulebook_names_the_key():
    import seevcn_amd.spconv as spconv
    inv = spconv.SparseInverseConv3d(8, 8, 3, indice_key="spconv_nowhere", bias=False)
    x = spconv.SparseConvTensor(torch.zeros(4, 8), torch.zeros(4, 4, dtype=torch.int32), GRID, 1)
    with pytest.raises(ValueError, match="spconv_nowhere"):
        inv(x)


def test_restatement_inverse_is_the_transpose():
    """<inverse(u), v> = <u, conv(v)> for the same table and the weight with its channel axes swapped: the inverse layer is the strided layer's adjoint."""
    coords = _sites()
    _, nbr_out, _, _ = osp.rulebook_sparse(coords, GRID, 3, 2, 1)
    g = torch.Generator().manual_seed(1)
    w = torch.randn((5, 3, 3, 3, 7), generator=g).double()                     # inverse: 7 -> 5
    u, v = torch.randn((nbr_out.shape[1], 7), generator=g).double(), torch.randn((len(coords), 5), generator=g).double()
    lhs = (UR.inverse_conv(u, nbr_out, len(coords), w) * v).sum()
    rhs = (u * UR.conv(v, nbr_out, w.permute(4, 1, 2, 3, 0))).sum()
    assert abs(float(lhs - rhs)) <= 1e-9 * abs(float(lhs))


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("use_plan", [True, False])
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_inverse_conv_against_float64(cuda, monkeypatch, geom, cin, cout, use_plan):
    import seevcn_amd.spconv as spconv
    from seevcn_amd.spconv import functional as Fsp
    monkeypatch.setattr(Fsp, "USE_PLAN", use_plan)
    bias = (cin, cout) == (8, 24)
    w = _want(geom, cin, cout, bias)
    down, inv = _layers(cuda, geom, cin, cout, bias, w)
    x = spconv.SparseConvTensor(torch.zeros((len(w["coords"]), cout), device=cuda), torch.from_numpy(w["coords"]).to(cuda), GRID, 2)
    y = down(x)
    assert np.array_equal(y.indices.cpu().numpy(), w["out_coords"])
    u = w["u"].to(cuda).requires_grad_(True)
    z = inv(y.replace_feature(u))
    assert z.indices is x.indices and z.spatial_shape == GRID                  # the paired layer's input sites
    assert_close_per_channel(z.features.detach().cpu().numpy(), w["z"], name="inverse conv forward")
    z.features.backward(w["gz"].to(cuda))
    assert_close_per_channel(u.grad.cpu().numpy(), w["gu"], name="inverse conv data gradient")
    assert_close_per_channel(osp.weight_to_kio(inv.weight.grad.cpu().numpy()), osp.weight_to_kio(w["gw"]), name="inverse conv weight gradient")
    paired, mirror = x.indice_dict["sp"], x.indice_dict[("sp", "inverse")]
    assert mirror.paired is paired and (mirror.n_in, mirror.n_out) == (paired.n_out, paired.n_in)
    assert mirror.nbr_out.data_ptr() == paired.nbr_in.data_ptr() and mirror.nbr_in.data_ptr() == paired.nbr_out.data_ptr()
    planned = use_plan and cin != 8
    assert (mirror.plan("fwd", cin, cout) is not None) == planned
    if planned:                                                               # the plan OBJECTS are the paired rulebook's: identity, not equality
        assert mirror.plan("fwd", cin, cout)[0] is paired._plans["bwd"]
        assert mirror.plan("bwd", cout, cin)[0] is paired._plans["fwd"]
        assert not mirror._plans


@pytest.mark.gpu
def test_tables_built_without_backward_plans(cuda):
    """The encoder's tables from prebuild_rulebooks(with_backward=False), as an eval forward builds them: the inverse layer makes the input-major
    plan on demand."""
    import seevcn_amd.spconv as spconv
    w = _want("k3s2p1", 64, 32, False)
    down, inv = _layers(cuda, "k3s2p1", 64, 32, False, w)
    x = spconv.SparseConvTensor(torch.zeros((len(w["coords"]), 32), device=cuda), torch.from_numpy(w["coords"]).to(cuda), GRID, 2)
    spconv.prebuild_rulebooks([down, inv], x, with_backward=False)
    assert "bwd" not in x.indice_dict["sp"]._plans and ("sp", "inverse") not in x.indice_dict
    with torch.no_grad():
        z = inv(down(x).replace_feature(w["u"].to(cuda)))
    assert_close_per_channel(z.features.cpu().numpy(), w["z"], name="inverse conv on eval tables")
    assert np.array_equal(z.indices.cpu().numpy(), w["coords"])


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", [(64, 32), (8, 24)])
def test_conv_bn_fusion_agrees(cuda, monkeypatch, cin, cout):
    """SparseSequential(inverse conv, BatchNorm1d, ReLU) in training mode with and without the conv + BN fusion, and both against float64."""
    import seevcn_amd.spconv as spconv
    from seevcn_amd.spconv import modules as M
    w = _want("unet_pad011", cin, cout, False)
    g = torch.Generator().manual_seed(9)
    gamma, beta = torch.rand((cout,), generator=g) + 0.5, torch.randn((cout,), generator=g)
    got = {}
    for fuse in (True, False):
        monkeypatch.setattr(M, "FUSE_CONV_BN", fuse)
        down, inv = _layers(cuda, "unet_pad011", cin, cout, False, w)
        bn = torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01).to(cuda)
        with torch.no_grad():
            bn.weight.copy_(gamma.to(cuda))
            bn.bias.copy_(beta.to(cuda))
        seq = spconv.SparseSequential(inv, bn, torch.nn.ReLU()).train()
        x = spconv.SparseConvTensor(torch.zeros((len(w["coords"]), cout), device=cuda), torch.from_numpy(w["coords"]).to(cuda), GRID, 2)
        u = w["u"].to(cuda).requires_grad_(True)
        z = seq(down(x).replace_feature(u))
        z.features.backward(w["gz"].to(cuda))
        got[fuse] = (z.features.detach().cpu().numpy(), u.grad.cpu().numpy(), osp.weight_to_kio(inv.weight.grad.cpu().numpy()))
    u64, w64 = w["u"].double().requires_grad_(True), w["weight"].double().requires_grad_(True)
    _, nbr_out, _, _ = osp.rulebook_sparse(w["coords"], GRID, *GEOMS["unet_pad011"])
    sd = {"bn.weight": gamma, "bn.bias": beta}
    z64 = torch.relu(UR.bn(UR.inverse_conv(u64, nbr_out, len(w["coords"]), w64), sd, "bn", True))
    z64.backward(w["gz"].double())
    want = (z64.detach().numpy(), u64.grad.numpy(), osp.weight_to_kio(w64.grad.numpy()))
    for i, what in enumerate(("forward", "data gradient", "weight gradient")):
        assert_close_per_channel(got[True][i], want[i], name=f"fused {what}")
        assert_close_per_channel(got[False][i], want[i], name=f"unfused {what}")
        assert_close_per_channel(got[True][i], got[False][i], name=f"fused vs unfused {what}")
