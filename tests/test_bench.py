"""bench.py's command line: the plain run prints the headline line only, --full adds the other measurements, --dump-outputs writes the last
timed step's results from seeded inputs."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--scenes-per-gpu", "2", "--objects-per-gpu", "8"]


def _bench(argv, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=timeout)


def _line(r):
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected, got {len(lines)}: {r.stdout[-500:]}"
    return json.loads(lines[0])


def test_bench_options_parse():
    r = _bench(["--help"], timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    assert _bench(["--steps", "0", "--dry-run"], timeout=120).returncode == 2
    assert _bench(["--dump-outputs", "x", "--config", "second"], timeout=120).returncode == 2


@pytest.mark.gpu
def test_bench_plain_line_and_dumped_outputs(tmp_path, cuda, hip_lib):
    """A plain run: one line with the headline fields and none of --full's blocks; --steps sets the timed steps.  --dump-outputs: float32
    arrays within 64 MB, one parameter and one gradient file per trained parameter.  A second run with the same arguments: the voxelised
    input bit for bit (integer coordinates, order-independent fixed-point sums), every other array within 1e-6 of its largest value (the
    run-to-run spread of fp32 atomic voxel sums was 1e-3 on the gradients).  The dump holds the LAST timed step: its loss and gradients and
    the weights after its optimiser step, as the same steps run in this process compute them."""
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = _line(_bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(d)] + SMALL))
        runs.append((out, d))
    out = runs[0][0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert not {"roofline", "roofline_vcn_gemm", "cpu_baseline", "side_modes"} & set(out)
    files = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(runs[0][1] / "*.npy"))}
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    for name in ("loss", "spatial_features_sample", "voxel_features", "voxel_coords"):
        assert name in files, name
    params = [n for n in files if n.startswith("param.")]
    assert params and all(f"grad.{n[len('param.'):]}" in files for n in params)
    assert np.isfinite(files["loss"]).all() and files["voxel_coords"].shape[0] == files["voxel_features"].shape[0] > 0
    again = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(runs[1][1] / "*.npy"))}
    assert set(again) == set(files)
    for n in files:
        if n in ("voxel_coords", "voxel_features"):
            np.testing.assert_array_equal(again[n], files[n], err_msg=n)
        else:
            assert np.abs(again[n].astype(np.float64) - files[n]).max() <= 1e-6 * np.abs(files[n]).max(), n
    # the same 1 + 3 steps in this process (bench's own prefetched step)
    import torch
    sys.path.insert(0, ROOT)
    import bench
    saved = bench.SCENES_PER_GPU, bench.OBJECTS_PER_GPU
    bench.SCENES_PER_GPU, bench.OBJECTS_PER_GPU = 2, 8
    try:
        points, objects, scene, *_ = bench.make_inputs(0, cuda)
        model = bench.build_model(cuda).train()
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        ps = [p for _, p in named]
        opt = torch.optim.SGD(ps, lr=1e-3, momentum=0.9, fused=True)
        pre = bench.Prefetch(model, (points, objects, scene))
        losses = []
        for i in range(4):
            if i == 3:
                before = torch.cat([p.detach().reshape(-1) for p in ps]).cpu().numpy()
            losses.append(float(bench.run_step_prefetched(model, opt, ps, pre, 1)))
        torch.cuda.synchronize()
        pre.close()
        after = torch.cat([p.detach().reshape(-1) for p in ps]).cpu().numpy()
        grads = {n: p.grad.detach().cpu().numpy() for n, p in named}
    finally:
        bench.SCENES_PER_GPU, bench.OBJECTS_PER_GPU = saved
    assert float(files["loss"]) == pytest.approx(losses[3], rel=1e-5) and losses[3] != losses[2]
    dumped = np.concatenate([files[f"param.{n}"].reshape(-1) for n, _ in named])
    step = np.abs(after - before).max()
    assert step > 0 and np.abs(dumped - after).max() < 0.1 * step          # after the last optimiser step, not before it
    for n, g in grads.items():
        assert np.abs(files[f"grad.{n}"] - g).max() <= 1e-5 * np.abs(g).max(), n
