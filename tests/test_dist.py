"""World-size-2 gloo test of the data-parallel exchange step (the flat-bucket gradient all-reduce of bench.py)."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(7))]
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, float(rank + 1) * (i + 1))
    bench.allreduce_grads(params, world)
    ok = all(torch.allclose(p.grad, torch.full_like(p, 1.5 * (i + 1))) for i, p in enumerate(params))
    out[rank] = bool(ok)
    dist.destroy_process_group()


def test_flat_bucket_allreduce_world2():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert dict(out) == {0: True, 1: True}


def _gpu_worker(rank, world, port, out):
    """Two ranks on ONE GPU over gloo (RCCL refuses two ranks on a device): everything of bench.py's N > 1 path except the
    transport -- per-rank inputs, the step, the flat-bucket exchange on CUDA gradients, the optimiser."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    bench.SCENES_PER_GPU, bench.OBJECTS_PER_GPU = 2, 8                      # small per-rank batch: this is a plumbing test
    device = torch.device("cuda", 0)
    points, objects, scene, *_ = bench.make_inputs(rank, device)
    model = bench.build_model(device).train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, fused=True)
    for _ in range(2):
        loss = bench.run_step(model, opt, params, (points, objects, scene), world)
    torch.cuda.synchronize()
    grads = torch.cat([p.grad.reshape(-1) for p in params if p.grad is not None]).cpu()
    weights = torch.cat([p.detach().reshape(-1) for p in params]).cpu()
    gathered = [None] * world
    dist.all_gather_object(gathered, (float(loss), grads, weights))
    same_grads = all(torch.equal(gathered[0][1], g[1]) for g in gathered)
    same_weights = all(torch.equal(gathered[0][2], g[2]) for g in gathered)
    out[rank] = (bool(same_grads), bool(same_weights), bool(torch.isfinite(grads).all()), gathered[0][0] != gathered[1][0])
    dist.destroy_process_group()


import pytest  # noqa: E402


@pytest.mark.gpu
def test_two_rank_step_keeps_replicas_in_sync_on_one_gpu():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_gpu_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    # averaged gradients and updated weights identical on both ranks, finite, while the ranks saw different scenes (different loss)
    assert dict(out) == {0: (True, True, True, True), 1: (True, True, True, True)}


def _run_bench(argv, env_extra=None, timeout=600):
    import json
    import subprocess
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected, got {len(lines)}: {r.stdout[-500:]}"
    return json.loads(lines[0])


def test_bench_self_launches_its_ranks_world2_gloo():
    """`python bench.py --gpus 2` with no launcher: the parent starts the two ranks itself (dry run = the N > 1 control flow on gloo)."""
    out = _run_bench(["--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1"])
    assert out["n_gpus"] == 2 and out["exchange_ok"] is True
    # the record proves how many ranks answered and what each ran on (all-gathered identities; on a node: one device UUID per rank)
    assert out["ranks"]["world_size_seen"] == 2 and len(out["ranks"]["devices"]) == 2 and out["ranks"]["distinct_devices"] == 2


def test_bench_rank_under_an_external_launcher_world2_gloo():
    """The torchrun path: WORLD_SIZE already set -> the process is a rank, not a launcher."""
    import subprocess
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1"],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-500:] for o in outs]
    assert '"exchange_ok": true' in outs[0][0] and "{" not in outs[1][0]


@pytest.mark.gpu
def test_bench_main_two_ranks_end_to_end_on_one_gpu():
    """bench.py's whole N = 2 path (launcher, per-rank inputs, steps with the exchange, timing protocol, rank-0-only kernel timing,
    barrier, teardown) with both ranks on cuda:0 over gloo.  Round 1's main() hung here: rank 0 entered a collective alone."""
    out = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--scenes-per-gpu", "2", "--objects-per-gpu", "8", "--full", "--no-cpu-baseline"],
                     {"SEEVCN_BENCH_SHARE_GPU": "1", "SEEVCN_BENCH_BACKEND": "gloo"}, timeout=900)
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["roofline"]["achieved"] > 0
    assert out["config"]["scenes_per_gpu"] == 2
    # two ranks answered, and the record shows that they SHARED one device (this test mode) -- on a node it would list two UUIDs
    assert out["ranks"]["world_size_seen"] == 2 and out["ranks"]["distinct_devices"] == 1 and out["backend"] == "gloo"


def _dist_helper_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import seevcn_amd  # noqa: F401
    from seevcn_amd.pcdet.utils import common_utils
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    os.environ.pop("MASTER_PORT", None)
    assert common_utils.get_dist_info() == (0, 1)
    n_gpus, r = common_utils.init_dist_pytorch(port, rank, backend="gloo")
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    out[rank] = (r, common_utils.get_dist_info(), float(t), n_gpus == torch.cuda.device_count())
    dist.destroy_process_group()


def test_init_dist_pytorch_world2_gloo():
    """The reference's rendezvous helper (pcdet/utils/common_utils.py:164-182) with the same signature and return value."""
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_dist_helper_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert dict(out) == {0: (0, (0, 2), 3.0, True), 1: (1, (1, 2), 3.0, True)}


def _ddp_worker(rank, world, port, sync_bn, out):
    """tools/train.py:118-144 of the reference: build_network -> (convert_sync_batchnorm) -> .cuda() -> .train() -> DistributedDataParallel,
    then train steps on per-rank scenes.  Two ranks share cuda:0 over gloo (RCCL refuses two ranks per device)."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.pcdet.utils import common_utils
    from seevcn_amd.seeding import seeded_state_dict
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    common_utils.init_dist_pytorch(port, 0, backend="gloo")
    device = torch.device("cuda", 0)
    net = detectors.build_detector(C.second_model_cfg(dynamic_vfe=True), num_class=3, dataset=C.SyntheticDatasetInfo())
    net.load_state_dict(seeded_state_dict(net, seed=5 + rank))              # DDP broadcasts rank 0's parameters and buffers at wrap time
    if sync_bn:
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
    net.to(device).train()
    ddp = torch.nn.parallel.DistributedDataParallel(net, device_ids=[0])
    params = [p for p in ddp.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9)
    pts, gt = synth.make_scene_batch(2, seed=2000 + 1000 * rank, n_az=96)
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(device), "gt_boxes": torch.from_numpy(gt).to(device)}
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
                 bool(torch.isfinite(grads).all() and np.isfinite(losses).all()), gathered[0][0] != gathered[1][0],
                 (not sync_bn) or all(torch.equal(gathered[0][3], g[3]) for g in gathered))
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("sync_bn", [False, True])
def test_ddp_wrapped_second_net_two_ranks_on_one_gpu(sync_bn):
    """The reference's own multi-GPU wrapper: a registered detector (custom autograd nodes, prefetched rulebooks, per-stream workspaces)
    inside DistributedDataParallel for two steps -- no hang, averaged gradients and updated weights bit-identical on both ranks while
    each saw different scenes.  With --sync_bn (train.py:118-119) the BatchNorm layers become torch SyncBatchNorm: SparseSequential then
    runs conv and norm as separate nodes (the fused conv+BN node only takes a plain nn.BatchNorm1d) and the running statistics agree too."""
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_ddp_worker, args=(world, _free_port(), sync_bn, out), nprocs=world, join=True)
    assert dict(out) == {0: (True, True, True, True, True), 1: (True, True, True, True, True)}


def _nccl_helper_worker(rank, port, out):
    sys.path.insert(0, ROOT)
    import seevcn_amd  # noqa: F401
    from seevcn_amd.pcdet.utils import common_utils
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1")
    os.environ.pop("MASTER_PORT", None)
    os.environ.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)          # the helper itself must export it before the first HIP call
    n_gpus, r = common_utils.init_dist_pytorch(port, rank, backend="nccl")
    t = torch.full((4,), 3.0, device="cuda")
    dist.all_reduce(t)
    torch.cuda.synchronize()
    out[0] = (r, n_gpus >= 1, t.cpu().tolist(), os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), os.environ.get("MASTER_PORT") == str(port))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_init_dist_pytorch_nccl_one_rank():
    """The reference-compatible RCCL path of the helper (torchrun -> init_dist_pytorch(backend='nccl')): a fresh process whose FIRST GPU
    call happens inside the helper -- the dmabuf-IPC switch must be in the environment by then -- then one all-reduce on the device."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_nccl_helper_worker, args=(_free_port(), out), nprocs=1, join=True)
    assert dict(out) == {0: (0, True, [3.0] * 4, "0", True)}
