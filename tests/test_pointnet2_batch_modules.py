"""PointnetSAModuleMSG / PointnetSAModule / PointnetFPModule of pointnet2_batch/pointnet2_modules.py on the GPU against the float64 restatement in
tests/pointnet2_batch_reference.py: eval-mode values, train-mode values and the gradients of every parameter and of the inputs.  B = 2, N = 64,
C = 4.  The ball-query inputs keep every (query, point) pair at least 1e-3 away from each radius in float64, so no group membership hangs on
fp32 rounding."""
import functools

import numpy as np
import pytest
import torch

import pointnet2_batch_reference as R
from oracle.tolerances import assert_close_per_channel

B, N, C = 2, 64, 4
RADII = (0.4, 0.8)


@functools.lru_cache(maxsize=None)
def _inputs():
    """xyz (B, N, 3) fp32 in a 2 m cube with every pairwise distance 1e-3 clear of both radii (any point may become a query), features (B, C, N)."""
    rng = np.random.default_rng(20)
    xyz = np.zeros((B, N, 3), np.float32)
    for b in range(B):
        for i in range(N):
            for _ in range(1000):
                p = rng.uniform(-1, 1, 3).astype(np.float32)
                d = np.linalg.norm(xyz[b, :i].astype(np.float64) - p.astype(np.float64), axis=1)
                if all((np.abs(d - r) > 1e-3).all() for r in RADII) and (d > 1e-2).all():
                    xyz[b, i] = p
                    break
            else:
                raise AssertionError("no point found")
    feat = rng.standard_normal((B, C, N)).astype(np.float32)
    return xyz, feat


def _seed_module(m, seed):
    """Parameters and BatchNorm statistics away from their initial values, the same on every run."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in list(m.named_parameters()) + list(m.named_buffers()):
            if not t.is_floating_point():
                continue
            if name.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif name.endswith("weight") and t.dim() == 1:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif t.dim() == 1:
                t.copy_(torch.randn(t.shape, generator=g) * 0.3)
            else:
                t.copy_(torch.randn(t.shape, generator=g) / (t.shape[1] ** 0.5))
    return m


def _compare(cuda, module, run_dev, run_ref, inputs, out_channel_axis=1):
    """Eval values, then train values and gradients.  run_dev(module, *device inputs) and run_ref(params64, *float64 inputs, training) return the
    feature tensor; inputs: name -> fp32 numpy array (None allowed)."""
    ref_inputs = {k: (None if v is None else torch.from_numpy(v).to(R.D)) for k, v in inputs.items()}
    dev_inputs = {k: (None if v is None else torch.from_numpy(v).to(cuda)) for k, v in inputs.items()}
    p = R.params64(module)
    module = module.to(cuda).eval()
    with torch.no_grad():
        got = run_dev(module, **dev_inputs)
        want = run_ref(p, training=False, **ref_inputs)
    assert_close_per_channel(got.cpu().numpy(), want.numpy(), name="eval output", channel_axis=out_channel_axis)
    module.train()
    for d in (ref_inputs, dev_inputs):
        for v in d.values():
            if v is not None:
                v.requires_grad_(True)
    got = run_dev(module, **dev_inputs)
    want = run_ref(p, training=True, **ref_inputs)
    assert_close_per_channel(got.detach().cpu().numpy(), want.detach().numpy(), name="train output", channel_axis=out_channel_axis)
    w = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(want.shape)))
    (want * w).sum().backward()
    (got * w.to(cuda).float()).sum().backward()
    for name, param in module.named_parameters():
        g, gw = param.grad.cpu().numpy(), p[name].grad.numpy()
        if g.ndim == 4:
            g, gw = g[:, :, 0, 0], gw[:, :, 0, 0]
        assert_close_per_channel(g, gw, name="grad of " + name)
    for k in inputs:
        if ref_inputs[k] is not None and ref_inputs[k].grad is not None:
            axis = 1 if k.endswith("feats") or k == "features" else -1
            assert_close_per_channel(dev_inputs[k].grad.cpu().numpy(), ref_inputs[k].grad.numpy(), name="grad of " + k, channel_axis=axis)
    return got


def test_constructors_leave_their_config_alone():
    """Two modules from one config list have equal shapes, and the list is what it was (the reference adds 3 to its first entry in place)."""
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as M
    mlps = [[C, 8, 16], [C, 8, 12]]
    kw = dict(npoint=16, radii=list(RADII), nsamples=[8, 16], mlps=mlps)
    a, b = M.PointnetSAModuleMSG(**kw), M.PointnetSAModuleMSG(**kw)
    assert mlps == [[C, 8, 16], [C, 8, 12]]
    assert [tuple(v.shape) for v in a.state_dict().values()] == [tuple(v.shape) for v in b.state_dict().values()]
    assert a.state_dict()["mlps.0.0.weight"].shape == (8, C + 3, 1, 1) and list(a.state_dict())[0] == "mlps.0.0.weight"
    mlp = [C, 8]
    c, d = M.PointnetSAModule(mlp=mlp, npoint=None), M.PointnetSAModule(mlp=mlp, npoint=None, use_xyz=False)
    assert mlp == [C, 8] and c.mlps[0][0].weight.shape == (8, C + 3, 1, 1) and d.mlps[0][0].weight.shape == (8, C, 1, 1)
    f = M.PointnetFPModule(mlp=[12, 16, 8])
    assert list(f.state_dict())[:2] == ["mlp.0.weight", "mlp.1.weight"]


@pytest.mark.gpu
@pytest.mark.parametrize("pool_method", ["max_pool", "avg_pool"])
def test_sa_module_msg(cuda, pool_method):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as M
    xyz, feat = _inputs()
    m = _seed_module(M.PointnetSAModuleMSG(npoint=16, radii=list(RADII), nsamples=[8, 16], mlps=[[C, 8, 16], [C, 8, 12]], pool_method=pool_method), 1)
    new_xyz = {}

    def dev(mod, xyz, features):
        new_xyz["dev"], out = mod(xyz, features)
        return out

    def ref(p, xyz, features, training):
        new_xyz["ref"], out = R.sa_forward(p, xyz, features, 16, RADII, (8, 16), pool_method=pool_method, training=training)
        return out

    out = _compare(cuda, m, dev, ref, dict(xyz=xyz, features=feat))
    assert out.shape == (B, 28, 16)
    assert np.array_equal(new_xyz["dev"].detach().cpu().numpy(), new_xyz["ref"].detach().numpy().astype(np.float32))


@pytest.mark.gpu
def test_sa_module_group_all(cuda):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as M
    xyz, feat = _inputs()
    m = _seed_module(M.PointnetSAModule(mlp=[C, 8, 16], npoint=None, radius=None, nsample=None), 2)

    def dev(mod, xyz, features):
        new_xyz, out = mod(xyz, features)
        assert new_xyz is None
        return out

    out = _compare(cuda, m, dev, lambda p, xyz, features, training: R.sa_forward(p, xyz, features, None, None, None, training=training)[1],
                   dict(xyz=xyz, features=feat))
    assert out.shape == (B, 16, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [True, False])
def test_fp_module_three_nn(cuda, skip):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as M
    xyz, feat = _inputs()
    known = np.ascontiguousarray(xyz[:, 40:52])                                                    # 12 known points, 40 unknown ones
    known_feats = np.random.default_rng(3).standard_normal((B, 6, 12)).astype(np.float32)
    c_in = 6 + (C if skip else 0)
    m = _seed_module(M.PointnetFPModule(mlp=[c_in, 16, 8]), 3)
    inputs = dict(unknown=np.ascontiguousarray(xyz[:, :40]), known=known, unknow_feats=np.ascontiguousarray(feat[:, :, :40]) if skip else None,
                  known_feats=known_feats)
    out = _compare(cuda, m, lambda mod, **kw: mod(kw["unknown"], kw["known"], kw["unknow_feats"], kw["known_feats"]),
                   lambda p, training, **kw: R.fp_forward(p, kw["unknown"], kw["known"], kw["unknow_feats"], kw["known_feats"], training), inputs)
    assert out.shape == (B, 8, 40)


@pytest.mark.gpu
def test_fp_module_without_known_points(cuda):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as M
    xyz, feat = _inputs()
    known_feats = np.random.default_rng(4).standard_normal((B, 6, 1)).astype(np.float32)
    m = _seed_module(M.PointnetFPModule(mlp=[6 + C, 8]), 4)
    inputs = dict(unknown=xyz, unknow_feats=feat, known_feats=known_feats)
    out = _compare(cuda, m, lambda mod, **kw: mod(kw["unknown"], None, kw["unknow_feats"], kw["known_feats"]),
                   lambda p, training, **kw: R.fp_forward(p, kw["unknown"], None, kw["unknow_feats"], kw["known_feats"], training), inputs)
    assert out.shape == (B, 8, N)
