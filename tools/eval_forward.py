#!/usr/bin/env python3
"""Eval-mode forward of the two 3-D backbones, launch-list chain against module tree.

VoxelBackBone8x on the bench's 16-scene KITTI-shaped batch and VoxelResBackBone8x on the one-scene CenterPoint batch, under torch.no_grad().  The
inputs are a COPY of what bench_configs.build makes for its `second` and `centerpoint` configs (seeds, sizes, n_az, voxeliser arguments, model seeds:
bench_configs hands out a step closure, not its inputs) -- when those change there, change them here.
SEEVCN_EVAL_CHAIN=1 and =0 run in alternating child processes (the switch is read at import), REPEATS times each; a child warms up, then times FORWARDS forwards between two HIP events.  Prints ms per forward
for every arm and repeat, then the spread of each arm.

    python tools/eval_forward.py                 # both backbones, 5 alternations
    REPEATS=7 FORWARDS=50 python tools/eval_forward.py second
    SPLIT=1 python tools/eval_forward.py --child second   # + medians of the host thread's time in the index build, its read and the fragment refresh
    python tools/eval_forward.py --child second  # one arm, in this process (what a profiler wraps: SEEVCN_EVAL_CHAIN from the environment)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _inputs(config, dev):
    """-> (backbone in eval mode with seeded weights, batch_dict in front of the backbone)"""
    import numpy as np
    import torch
    import bench
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.seeding import seeded_state_dict
    if config == "second":
        n = 16
        pts, _ = synth.make_scene_batch(n, seed=2000, n_az=bench.SCENE_N_AZ)
        net = detectors.build_detector(C.second_model_cfg(dynamic_vfe=True), num_class=3, dataset=C.SyntheticDatasetInfo())
        net.load_state_dict(seeded_state_dict(net, seed=5))
        batch = {"batch_size": n, "points": torch.from_numpy(pts).to(dev)}
    else:
        import seevcn_amd.config_inputs as ci
        from seevcn_amd.pcdet.ops import voxel_ops
        p, _ = ci.centerpoint_scene(seed=4000, n_az=1200)
        p = p[np.random.default_rng(0).permutation(len(p))]
        grid = np.round((np.array(ci.NUSC_RANGE[3:]) - np.array(ci.NUSC_RANGE[:3])) / np.array(ci.NUSC_VOXEL)).astype(np.int64)
        ds = C.SyntheticDatasetInfo(class_names=C.NUSC_CLASS_NAMES, point_cloud_range=ci.NUSC_RANGE, voxel_size=ci.NUSC_VOXEL, num_point_features=3)
        net = detectors.build_detector(C.centerpoint_model_cfg(), num_class=10, dataset=ds)
        net.load_state_dict(seeded_state_dict(net, seed=21))
        vox, crd, nmp, nv = voxel_ops.voxelize_hard(torch.from_numpy(p).to(dev), 0, 3, [len(p)], ci.NUSC_RANGE, ci.NUSC_VOXEL, grid, 10, 120000)
        k = int(nv[0])
        coords = torch.cat([torch.zeros((k, 1), dtype=torch.int32, device=dev), crd[0, :k]], dim=1)
        batch = {"batch_size": 1, "voxels": vox[0, :k].contiguous(), "voxel_coords": coords, "voxel_num_points": nmp[0, :k].contiguous()}
    net = net.to(dev).eval()
    with torch.no_grad():
        batch = net.module_list[0](batch)                          # the VFE: voxel_features / voxel_coords
    return net.backbone_3d, batch


def _host_split():
    """SPLIT=1: wall-clock stamps of the host thread around the pieces of a backbone forward, as tools/step_hosttime.py takes them for the training step:
    the index build (prebuild_rulebooks) with the blocked part of its device -> host read apart, the weight-fragment refresh, and the rest (the launch
    list, or the walk over the module tree) = host enqueue time minus these.  -> {piece: [seconds per call]}"""
    import time
    import seevcn_amd.spconv as spconv
    import seevcn_amd.spconv.functional as Fsp
    from seevcn_amd import _lib
    T = {}

    def timed(name, fn):
        def wrapper(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                T.setdefault(name, []).append(time.perf_counter() - t0)
        return wrapper

    read = timed("read: device -> host copy + wait (inside the index build)", _lib.host_ints)
    _lib.host_ints = read
    Fsp._lib.host_ints = read
    spconv.prebuild_rulebooks = timed("index build: prebuild_rulebooks (read included)", spconv.prebuild_rulebooks)
    spconv.refresh_weight_fragments = timed("refresh_weight_fragments", spconv.refresh_weight_fragments)
    return T


def child(config):
    import time
    import torch
    dev = torch.device("cuda:0")
    backbone, batch = _inputs(config, dev)
    warmup, forwards = int(os.environ.get("WARMUP", "10")), int(os.environ.get("FORWARDS", "30"))
    split = _host_split() if os.environ.get("SPLIT") == "1" else None
    with torch.no_grad():
        for _ in range(warmup):
            backbone(dict(batch))
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        s.record()
        for _ in range(forwards):
            backbone(dict(batch))
        e.record()
        host_ms = (time.perf_counter() - t0) * 1e3 / forwards      # time the host needs to enqueue one forward (it runs ahead of the GPU when it can)
        torch.cuda.synchronize()
    print(json.dumps({"config": config, "backbone": type(backbone).__name__, "voxels": int(batch["voxel_coords"].shape[0]),
                      "eval_chain": os.environ.get("SEEVCN_EVAL_CHAIN", "1") != "0", "ms_per_forward": round(s.elapsed_time(e) / forwards, 4),
                      "host_enqueue_ms_per_forward": round(host_ms, 4),
                      **({"host_split_median_ms": {k: round(sorted(v[-forwards:])[forwards // 2] * 1e3, 4) for k, v in split.items()}} if split else {})}))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1])
    configs = args or ["second", "centerpoint"]
    repeats = int(os.environ.get("REPEATS", "5"))
    for config in configs:
        arms = {"1": [], "0": []}
        for rep in range(repeats):
            for arm in ("1", "0"):
                env = dict(os.environ, SEEVCN_EVAL_CHAIN=arm)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config], env=env, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:                             # nothing more is started on the GPU after a failed child
                    sys.stderr.write(out.stdout + out.stderr)
                    return out.returncode
                r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
                arms[arm].append(r)
                print(f"{config:11s} {r['backbone']:18s} rep {rep} eval chain {'on ' if arm == '1' else 'off'}: {r['ms_per_forward']:8.3f} ms / forward "
                      f"(host enqueue {r['host_enqueue_ms_per_forward']:.3f} ms, {r['voxels']} voxels)", flush=True)
        for arm, name in (("1", "chain"), ("0", "module tree")):
            ms = [r["ms_per_forward"] for r in arms[arm]]
            print(f"{config:11s} {name:11s}: min {min(ms):.3f}  median {sorted(ms)[len(ms) // 2]:.3f}  max {max(ms):.3f} ms / forward over {len(ms)} repeats")
    return 0


if __name__ == "__main__":
    sys.exit(main())
