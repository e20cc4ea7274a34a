"""torch.nn.SyncBatchNorm on the fused sparse conv + BatchNorm routes (spconv/norm.py route(), the *_local / *_global kernels of csrc/norm.hip,
the cut launch lists of spconv/chain.py).  Two-rank tests: both ranks on cuda:0 over gloo, like tests/test_dist.py::_ddp_worker."""
import os
import re
import socket
import sys
from datetime import timedelta

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sv_batchnorm_stats_local", "sv_batchnorm_finalize_global", "sv_batchnorm_backward_sums_local", "sv_batchnorm_backward_apply_global")
PC_RANGE, VOXEL, GRID = [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1], [1408, 1600, 40]
EPS, MOM = 1e-3, 0.01


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---------------------------------------------------------------------------------------------------------------- 1. ABI (no GPU)
def test_sync_batchnorm_symbols_in_header_bindings_and_library(hip_lib):
    import seevcn_amd._lib as L
    header = open(L.HEADER_PATH).read()
    protos = L.parse_declarations(header)
    for name in SYMBOLS:
        assert name in protos and protos[name][0] == "int", f"{name} not declared in seevcn_hip.h"
        assert name in L.SIGNATURES, f"{name} has no prototype in _lib.py"
        assert hasattr(hip_lib, name), f"{name} not exported by the library"
    for code, name in ((11, "SV_OP_BN_STATS_LOCAL"), (12, "SV_OP_BN_FINALIZE_GLOBAL"), (13, "SV_OP_BN_BWD_SUMS_LOCAL"), (14, "SV_OP_BN_BWD_APPLY_GLOBAL")):
        assert re.search(r"#define\s+" + name + r"\s+" + str(code) + r"\b", header), name


def test_route_of_a_norm_module_without_a_process_group():
    """No torch.distributed: BatchNorm1d and a SyncBatchNorm (training or eval) are PLAIN, other norms are not taken."""
    import torch.nn as nn
    from seevcn_amd.spconv import norm
    assert norm.route(nn.BatchNorm1d(16)) == norm.PLAIN
    assert norm.route(nn.SyncBatchNorm(16)) == norm.PLAIN and norm.route(nn.SyncBatchNorm(16).eval()) == norm.PLAIN
    assert norm.route(nn.BatchNorm2d(16)) is None and norm.route(nn.LayerNorm(16)) is None

    class Mine(nn.BatchNorm1d):
        pass
    assert norm.route(Mine(16)) is None and norm.route(Mine(16), subclasses=True) == norm.PLAIN


# ---------------------------------------------------------------------------------------------------------------- 2. kernels, one process
class _K:
    """Thin callers of the BatchNorm entry points on raw tensors (one scratch per instance)."""

    def __init__(self, lib, c, dev):
        import seevcn_amd._lib as L
        self.L, self.lib, self.c, self.dev = L, lib, c, dev
        self.scratch = torch.zeros(lib.sv_batchnorm_scratch_bytes(c), dtype=torch.uint8, device=dev)

    def put_partials(self, part):
        """part (P, 2, C) float32 -> behind the 4 C coefficient floats of the scratch, where a producing kernel's epilogue leaves them"""
        raw = part.contiguous().view(torch.uint8).reshape(-1)
        self.scratch[16 * self.c:16 * self.c + raw.numel()] = raw

    def f32(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    def f64(self, *shape):
        return torch.empty(shape, dtype=torch.float64, device=self.dev)

    def stats_local(self, x, n, n_partials=0):
        sums = self.f64(2 * self.c + 1)
        p = self.L.ptr
        self.L.check(self.lib.sv_batchnorm_stats_local(p(x), n, self.c, p(self.scratch), n_partials, p(sums), self.L.stream()), "stats_local")
        return sums

    def finalize_global(self, gathered, gamma, beta, rm, rv, nbt):
        coef, mean, invstd, total = self.f32(2 * self.c), self.f32(self.c), self.f32(self.c), self.f64(1)
        p = self.L.ptr
        self.L.check(self.lib.sv_batchnorm_finalize_global(p(gathered), gathered.shape[0], self.c, p(gamma), p(beta), p(rm), p(rv), MOM, EPS, p(coef), p(mean),
                                                           p(invstd), p(nbt), p(total), self.L.stream()), "finalize_global")
        return coef, mean, invstd, total

    def finalize_forward(self, x, n, gamma, beta, rm, rv, nbt, n_partials=0):
        coef, mean, invstd = self.f32(2 * self.c), self.f32(self.c), self.f32(self.c)
        p = self.L.ptr
        self.L.check(self.lib.sv_batchnorm_finalize_forward(p(x), n, self.c, p(gamma), p(beta), p(rm), p(rv), MOM, EPS, p(self.scratch), n_partials, p(coef),
                                                            p(mean), p(invstd), p(nbt), self.L.stream()), "finalize_forward")
        return coef, mean, invstd

    def sums_local(self, x, dy, gamma, beta, mean, invstd, relu, n_partials=0):
        dg, db, sums = self.f32(self.c), self.f32(self.c), self.f64(2 * self.c)
        p = self.L.ptr
        self.L.check(self.lib.sv_batchnorm_backward_sums_local(p(x), p(dy), x.shape[0], self.c, p(gamma), p(beta), p(mean), p(invstd), int(relu), p(self.scratch),
                                                               n_partials, p(dg), p(db), p(sums), self.L.stream()), "sums_local")
        return dg, db, sums

    def apply_global(self, x, dy, gamma, beta, mean, invstd, relu, gathered, total):
        dx = torch.empty_like(x)
        p = self.L.ptr
        self.L.check(self.lib.sv_batchnorm_backward_apply_global(p(x), p(dy), x.shape[0], self.c, p(gamma), p(beta), p(mean), p(invstd), int(relu), p(gathered),
                                                                 gathered.shape[0], p(total), p(self.scratch), p(dx), self.L.stream()), "apply_global")
        return dx

    def backward(self, x, dy, gamma, beta, mean, invstd, relu, n_partials=0):
        dx, dg, db = torch.empty_like(x), self.f32(self.c), self.f32(self.c)
        p = self.L.ptr
        if n_partials:
            self.L.check(self.lib.sv_batchnorm_relu_backward_partial(p(x), p(dy), x.shape[0], self.c, p(gamma), p(beta), p(mean), p(invstd), int(relu),
                                                                     p(self.scratch), n_partials, p(dx), p(dg), p(db), self.L.stream()), "backward_partial")
        else:
            self.L.check(self.lib.sv_batchnorm_relu_backward(p(x), p(dy), x.shape[0], self.c, p(gamma), p(beta), p(mean), p(invstd), int(relu), p(self.scratch),
                                                             p(dx), p(dg), p(db), self.L.stream()), "backward")
        return dx, dg, db


def _inputs(c, n, dev):
    g = torch.Generator().manual_seed(1000 + c)
    x = (torch.randn(n, c, generator=g) * 1.7 + 0.6).to(dev)
    dy = torch.randn(n, c, generator=g).to(dev)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), (torch.randn(c, generator=g) * 0.3).to(dev)
    return x, dy, gamma, beta


def _running(c, dev):
    return torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.int64, device=dev)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [16, 64, 128])
def test_hip_sync_batchnorm_kernels_over_unequal_row_blocks_vs_float64(cuda, hip_lib, c):
    """An (N, C) matrix split into three row blocks of unequal size (one of a single row) stands for three ranks: stats_local per block, the buffers
    stacked by hand as the gathered buffer, finalize_global; sums_local / apply_global per block.  Against torch's batch_norm (+ ReLU) over the WHOLE
    matrix in float64 and its autograd."""
    from tolerances import assert_close_per_channel
    sizes = [1733, 1, 1266]
    n = sum(sizes)
    x, dy, gamma, beta = _inputs(c, n, cuda)
    k = _K(hip_lib, c, cuda)
    xs, dys = [t.contiguous() for t in x.split(sizes)], [t.contiguous() for t in dy.split(sizes)]
    gathered = torch.stack([k.stats_local(xb, xb.shape[0]) for xb in xs])
    assert gathered[:, 2 * c].tolist() == [float(s) for s in sizes]
    rm, rv, nbt = _running(c, cuda)
    coef, mean, invstd, total = k.finalize_global(gathered, gamma, beta, rm, rv, nbt)
    assert float(total) == float(n) and int(nbt) == 1

    x64 = x.double().cpu().requires_grad_(True)
    g64, b64 = gamma.double().cpu().requires_grad_(True), beta.double().cpu().requires_grad_(True)
    rm64, rv64 = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    y64 = torch.relu(torch.nn.functional.batch_norm(x64, rm64, rv64, g64, b64, True, MOM, EPS))
    m64 = x64.detach().mean(0)
    i64 = 1.0 / torch.sqrt(x64.detach().var(0, unbiased=False) + EPS)
    for got, want, name in ((mean, m64, "mean"), (invstd, i64, "invstd"), (rm, rm64, "running_mean"), (rv, rv64, "running_var"),
                            (coef[:c], g64.detach() * i64, "scale"), (coef[c:], b64.detach() - m64 * g64.detach() * i64, "shift")):
        assert_close_per_channel(got.cpu().numpy(), want.numpy(), name=f"{name} C={c}")
    y = torch.empty_like(x)
    import seevcn_amd._lib as L
    L.check(hip_lib.sv_batchnorm_apply(L.ptr(x), n, c, L.ptr(coef), 1, L.ptr(y), L.stream()), "apply")
    assert_close_per_channel(y.cpu().numpy(), y64.detach().numpy(), name=f"y C={c}")

    y64.backward(dy.double().cpu())
    local = [k.sums_local(xb, db, gamma, beta, mean, invstd, True) for xb, db in zip(xs, dys)]
    gathered_b = torch.stack([s for _, _, s in local])
    dx = torch.cat([k.apply_global(xb, db, gamma, beta, mean, invstd, True, gathered_b, total) for xb, db in zip(xs, dys)])
    assert_close_per_channel(dx.cpu().numpy(), x64.grad.numpy(), name=f"dx C={c}")
    # dgamma / dbeta stay local sums: their sum over the blocks is the gradient of the whole matrix
    assert_close_per_channel(sum(dg for dg, _, _ in local).cpu().numpy(), g64.grad.numpy(), name=f"dgamma C={c}")
    assert_close_per_channel(sum(db for _, db, _ in local).cpu().numpy(), b64.grad.numpy(), name=f"dbeta C={c}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", [16, 64, 128])
@pytest.mark.parametrize("from_partials", [False, True])
def test_hip_sync_batchnorm_kernels_world_one_bit_identical_to_the_plain_kernels(cuda, hip_lib, c, from_partials):
    """world == 1: stats_local + finalize_global give the bits of sv_batchnorm_finalize_forward (coef, batch statistics, running statistics), and
    sums_local + apply_global the bits of sv_batchnorm_relu_backward[_partial] (dx, dgamma, dbeta) -- from workgroup partials in the scratch and from x."""
    n, P = 2999, 37
    x, dy, gamma, beta = _inputs(c, n, cuda)
    k = _K(hip_lib, c, cuda)
    g = torch.Generator().manual_seed(7 + c)
    part_f = (torch.randn(P, 2, c, generator=g) * 40).abs().to(cuda)            # any (P, 2, C) floats serve as a producer's partial sums
    part_f[:, 1] = part_f[:, 1] * 3 + part_f[:, 0] ** 2 / (n / P)               # keeps sum x^2 / n >= mean^2
    part_b = (torch.randn(P, 2, c, generator=g) * 5).to(cuda)
    xarg, npart = (None, P) if from_partials else (x, 0)

    rm0, rv0, nbt0 = _running(c, cuda)
    if from_partials:
        k.put_partials(part_f)
    coef0, mean0, invstd0 = k.finalize_forward(xarg, n, gamma, beta, rm0, rv0, nbt0, npart)
    rm1, rv1, nbt1 = _running(c, cuda)
    if from_partials:
        k.put_partials(part_f)
    sums = k.stats_local(xarg, n, npart)
    coef1, mean1, invstd1, total = k.finalize_global(sums.view(1, -1), gamma, beta, rm1, rv1, nbt1)
    for a, b, name in ((coef0, coef1, "coef"), (mean0, mean1, "save_mean"), (invstd0, invstd1, "save_invstd"), (rm0, rm1, "running_mean"),
                       (rv0, rv1, "running_var"), (nbt0, nbt1, "num_batches_tracked")):
        assert torch.equal(a, b), f"{name} differs (C={c}, from_partials={from_partials})"
    assert float(total) == float(n)

    if from_partials:
        k.put_partials(part_b)
    dx0, dg0, db0 = k.backward(x, dy, gamma, beta, mean0, invstd0, True, npart)
    if from_partials:
        k.put_partials(part_b)
    dg1, db1, sums_b = k.sums_local(x, dy, gamma, beta, mean0, invstd0, True, npart)
    dx1 = k.apply_global(x, dy, gamma, beta, mean0, invstd0, True, sums_b.view(1, -1), total)
    for a, b, name in ((dx0, dx1, "dx"), (dg0, dg1, "dgamma"), (db0, db1, "dbeta")):
        assert torch.equal(a, b), f"{name} differs (C={c}, from_partials={from_partials})"


# ---------------------------------------------------------------------------------------------------------------- 3. two ranks, backbone vs the oracle
def _forbid_torch_sync_bn_on_matrices():
    """Route assertion: torch's own SyncBatchNorm.forward must never see an (N, C) voxel feature matrix -- the fused routes take those."""
    orig = torch.nn.SyncBatchNorm.forward

    def forward(self, input):
        if input.dim() == 2:
            raise AssertionError(f"torch.nn.SyncBatchNorm.forward reached with a 2-D input {tuple(input.shape)}: the fused route stood down")
        return orig(self, input)
    torch.nn.SyncBatchNorm.forward = forward


def _backbone_and_input(pts, batch_size, device, sync):
    from seevcn_amd.pcdet.models import backbones_3d
    from seevcn_amd.pcdet.models.backbones_3d import vfe
    from seevcn_amd.seeding import seeded_state_dict
    bd = {"batch_size": batch_size, "points": torch.from_numpy(pts).to(device)}
    bd = vfe.__all__["DynMeanVFE"](model_cfg={}, num_point_features=3, voxel_size=VOXEL, grid_size=GRID, point_cloud_range=PC_RANGE)(bd)
    m = backbones_3d.__all__["VoxelBackBone8x"]({}, 3, GRID)
    sd = seeded_state_dict(m, seed=1)
    m.load_state_dict(sd)
    if sync:
        m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
    return m.to(device).train(), sd, bd


def _train_pass(m, bd, G, input_grad):
    """One forward + backward of backbone -> HeightCompression with loss sum(dense * G).  -> dict of CPU tensors"""
    from seevcn_amd.pcdet.models.backbones_2d import map_to_bev
    m.zero_grad(set_to_none=True)
    bd = dict(bd)
    feats = bd["voxel_features"].detach().clone().requires_grad_(input_grad)
    bd["voxel_features"] = feats
    bd = map_to_bev.__all__["HeightCompression"]({"NUM_BEV_FEATURES": 256})(m(bd))
    dense = bd["spatial_features"]
    (dense * G.to(dense.device)).sum().backward()
    torch.cuda.synchronize()
    t = bd["encoded_spconv_tensor"]
    return {"out": t.features.detach().cpu(), "out_indices": t.indices.cpu(), "out_shape": list(t.spatial_shape),
            "dinput": None if feats.grad is None else feats.grad.cpu(), "grads": {k: p.grad.detach().cpu() for k, p in m.named_parameters()},
            "buffers": {k: b.detach().cpu().clone() for k, b in m.named_buffers()}}


def _g_for(rank, shape):
    return torch.from_numpy(np.random.default_rng(5 + rank).normal(size=tuple(shape)).astype(np.float32))


def _backbone_worker(rank, world, port, backend, outdir):
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import seevcn_amd.synth as synth
    from seevcn_amd.spconv import chain
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev_index = rank if backend == "nccl" else 0
    torch.cuda.set_device(dev_index)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=timedelta(seconds=120))
    device = torch.device("cuda", dev_index)
    _forbid_torch_sync_bn_on_matrices()
    chained = []
    run_chain = chain.run_chain
    chain.run_chain = lambda *a: chained.append(1) or run_chain(*a)
    pts, _ = synth.make_scene_batch(2, seed=2000 + 1000 * rank, n_az=90)
    m, _, bd = _backbone_and_input(pts, 2, device, sync=True)
    G = _g_for(rank, (2, 256, 200, 176))
    # the input wants a gradient: the module tree runs (conv + BatchNorm node per block); without: the launch-list chain.  Same arithmetic, two routes.
    res = {"module": _train_pass(m, bd, G, input_grad=True), "n_chain_module": len(chained)}
    res["chain"] = _train_pass(m, bd, G, input_grad=False)
    res["n_chain_chain"] = len(chained) - res["n_chain_module"]
    res["coords"], res["features"] = bd["voxel_coords"].cpu(), bd["voxel_features"].detach().cpu()
    torch.save(res, os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _check_two_rank_backbone(cuda, tmp_path, backend):
    import torch.multiprocessing as mp
    import seevcn_amd.synth as synth
    from oracle import spconv as osp
    from oracle import spconv_train as ost
    from tolerances import assert_close_per_channel
    mp.spawn(_backbone_worker, args=(2, _free_port(), backend, str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f"rank{k}.pt"), weights_only=False) for k in range(2)]
    assert [x["n_chain_module"] for x in r] == [0, 0] and [x["n_chain_chain"] for x in r] == [1, 1], "each pass must take the route it is meant to test"

    # the 4-scene union: rank 1's batch index + 2, rows appended (batch-major voxel order: this IS the sorted order)
    c1 = r[1]["coords"].clone()
    c1[:, 0] += 2
    coords = torch.cat([r[0]["coords"], c1]).numpy()
    feats = torch.cat([r[0]["features"], r[1]["features"]]).numpy()
    m_plain, sd, _ = _backbone_and_input(synth.make_scene_batch(2, seed=2000, n_az=90)[0], 2, cuda, sync=False)
    ref_dense, leaves, (ref_out, ref_coords, ref_shape) = ost.backbone8x_train_chain({k: v.numpy() for k, v in sd.items()}, feats, coords, 4, m_plain.sparse_shape)
    G = torch.cat([_g_for(0, (2, 256, 200, 176)), _g_for(1, (2, 256, 200, 176))])
    (ref_dense * G.double()).sum().backward()
    n_in, ref_rank = r[0]["features"].shape[0], ref_coords[:, 0] >= 2
    for route in ("module", "chain"):
        for k in range(2):
            got, sel = r[k][route], (ref_rank if k else ~ref_rank)
            want_idx = ref_coords[sel].copy()
            want_idx[:, 0] -= 2 * k
            assert np.array_equal(got["out_indices"].numpy(), want_idx) and got["out_shape"] == list(ref_shape), (route, k)
            assert_close_per_channel(got["out"].numpy(), ref_out.detach().numpy()[sel], name=f"conv_out features, rank {k}, {route} route")
        for k in range(2):
            want = leaves["input"].grad.numpy()[n_in * k:n_in * k + r[k]["features"].shape[0]]
            if route == "module":
                assert_close_per_channel(r[k][route]["dinput"].numpy(), want, rtol=2e-3, atol_frac=2e-4, name=f"d loss / d voxel_features, rank {k}")
        checked = 0
        for key in r[0][route]["grads"]:
            got = (r[0][route]["grads"][key] + r[1][route]["grads"][key]).numpy()
            if got.ndim == 5:
                got = osp.weight_to_kio(got)
            assert_close_per_channel(got, leaves[key].grad.numpy(), rtol=2e-3, atol_frac=2e-3, name=f"sum over ranks of grad {key}, {route} route")
            checked += 1
        assert checked == 12 + 24
    # running statistics (after the first pass): the same bits on both ranks ...
    b0, b1 = r[0]["module"]["buffers"], r[1]["module"]["buffers"]
    assert sorted(b0) == sorted(b1) and len(b0) == 3 * 12
    for key in b0:
        assert torch.equal(b0[key], b1[key]), f"{key} differs between the ranks"
    # ... and those of ONE process of this package running plain BatchNorm1d over the 4-scene batch
    p1 = synth.make_scene_batch(2, seed=3000, n_az=90)[0].copy()
    p1[:, 0] += 2
    pts4 = np.concatenate([synth.make_scene_batch(2, seed=2000, n_az=90)[0], p1])
    m4, _, bd4 = _backbone_and_input(pts4, 4, cuda, sync=False)
    assert np.array_equal(bd4["voxel_coords"].cpu().numpy(), coords)
    single = _train_pass(m4, bd4, G, input_grad=True)["buffers"]
    for key in b0:
        if key.endswith("num_batches_tracked"):
            assert int(b0[key]) == int(single[key]) == 1
        else:
            assert_close_per_channel(b0[key].numpy(), single[key].numpy(), name=key)


@pytest.mark.gpu
def test_hip_sync_batchnorm_backbone_two_ranks_vs_oracle_chain(cuda, hip_lib, tmp_path):
    """VoxelBackBone8x + HeightCompression converted with convert_sync_batchnorm, two ranks (no DDP wrapper) with 2 scenes each, against the float64
    oracle chain on the 4-scene union: SyncBatchNorm over two ranks IS BatchNorm over the union, and the convolutions are per scene.  Per rank the
    conv_out features and the input gradient; the sum over ranks of all 12 weight and 24 BatchNorm gradients; running statistics.  Both routes:
    module tree (conv + BatchNorm node) and launch-list chain.  torch's SyncBatchNorm.forward raises on a 2-D input inside the workers."""
    _check_two_rank_backbone(cuda, tmp_path, "gloo")


@pytest.mark.gpu
def test_hip_sync_batchnorm_backbone_two_ranks_rccl(cuda, hip_lib, tmp_path):
    """The same over RCCL, one rank per device."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _check_two_rank_backbone(cuda, tmp_path, "nccl")


# ---------------------------------------------------------------------------------------------------------------- 4. two ranks, whole detector under DDP
def _ddp_sync_worker(rank, world, port, out):
    """tests/test_dist.py::_ddp_worker with sync_bn and the 2-D-only patch; rank 0 trains on 1 scene, rank 1 on 2 (row counts differ by about 2x)."""
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.seeding import seeded_state_dict
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    _forbid_torch_sync_bn_on_matrices()
    device = torch.device("cuda", 0)
    net = detectors.build_detector(C.second_model_cfg(dynamic_vfe=True), num_class=3, dataset=C.SyntheticDatasetInfo())
    net.load_state_dict(seeded_state_dict(net, seed=5 + rank))
    net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
    net.to(device).train()
    ddp = torch.nn.parallel.DistributedDataParallel(net, device_ids=[0])
    params = [p for p in ddp.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9)
    scenes = 1 + rank
    pts, gt = synth.make_scene_batch(scenes, seed=2000 + 1000 * rank, n_az=96)
    batch = {"batch_size": scenes, "points": torch.from_numpy(pts).to(device), "gt_boxes": torch.from_numpy(gt).to(device)}
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        ret, _, _ = ddp(dict(batch))
        ret["loss"].backward()
        opt.step()
        losses.append(float(ret["loss"]))
    torch.cuda.synchronize()
    grads = torch.cat([p.grad.reshape(-1) for p in params]).cpu()
    weights = torch.cat([p.detach().reshape(-1) for p in params]).cpu()
    stats = torch.cat([b.detach().float().reshape(-1) for b in net.buffers()]).cpu()
    gathered = [None] * world
    dist.all_gather_object(gathered, (losses, grads, weights, stats))
    out[rank] = (all(torch.equal(gathered[0][1], g[1]) for g in gathered), all(torch.equal(gathered[0][2], g[2]) for g in gathered),
                 all(torch.equal(gathered[0][3], g[3]) for g in gathered), bool(torch.isfinite(grads).all() and np.isfinite(losses).all()),
                 gathered[0][0] != gathered[1][0])
    dist.destroy_process_group()


@pytest.mark.gpu
def test_hip_sync_batchnorm_ddp_second_net_two_ranks_unequal_batches(cuda, hip_lib):
    """The DDP-wrapped SECONDNet with --sync_bn for two steps: no hang, gradients / weights / buffers bit-identical on both ranks, losses finite and
    different; the sparse backbone's SyncBatchNorm modules never run their own forward (the BEV backbone's 4-D inputs still do)."""
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    mp.spawn(_ddp_sync_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert dict(out) == {0: (True,) * 5, 1: (True,) * 5}


# ---------------------------------------------------------------------------------------------------------------- 5. one process, no process group
@pytest.mark.gpu
def test_hip_converted_backbone_without_a_process_group_equals_the_unconverted_one(cuda, hip_lib):
    """convert_sync_batchnorm without torch.distributed: every norm takes the PLAIN route -- outputs and all gradients torch.equal to BatchNorm1d's."""
    import seevcn_amd.synth as synth
    pts, _ = synth.make_scene_batch(2, seed=2000, n_az=90)
    G = _g_for(0, (2, 256, 200, 176))
    for input_grad in (False, True):                                   # chain route, module route
        res = []
        for sync in (False, True):
            m, _, bd = _backbone_and_input(pts, 2, cuda, sync=sync)
            assert any(type(x) is torch.nn.SyncBatchNorm for x in m.modules()) == sync
            res.append(_train_pass(m, bd, G, input_grad=input_grad))
        a, b = res
        assert torch.equal(a["out"], b["out"]) and torch.equal(a["out_indices"], b["out_indices"])
        assert input_grad is False or torch.equal(a["dinput"], b["dinput"])
        assert sorted(a["grads"]) == sorted(b["grads"]) and len(a["grads"]) == 36
        for key in a["grads"]:
            assert torch.equal(a["grads"][key], b["grads"][key]), key
        for key in a["buffers"]:
            assert torch.equal(a["buffers"][key], b["buffers"][key]), key
