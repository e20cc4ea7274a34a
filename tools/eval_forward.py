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
    python tools/eval_forward.py --dtype float16 # the half-precision list (set_eval_dtype) against the fp32 list instead: the two arms alternate in
                                                 # rotating order, the fp32 arm of the same run is the baseline
    python tools/eval_forward.py --child second --dtype float16          # one arm of that, in this process
    python tools/eval_forward.py --layers second # per-launch times of both lists' conv rows (sv_run_ops_timed), fp16 beside fp32, in one process
    python tools/eval_forward.py --deviation     # fp16 list against fp32 list on the last tap: 2-scene and 16-scene batches (reported, no bound exists)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _inputs(config, dev, n_scenes=16):
    """-> (backbone in eval mode with seeded weights, batch_dict in front of the backbone)"""
    import numpy as np
    import torch
    import bench
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.seeding import seeded_state_dict
    if config == "second":
        n = n_scenes
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


def layers(config):
    """Median time of every conv launch of the fp32 and the fp16 eval list, from sv_run_ops_timed on the lists the backbone itself builds."""
    import numpy as np
    import torch
    from seevcn_amd import _lib
    from seevcn_amd.spconv import chain
    dev = torch.device("cuda:0")
    backbone, batch = _inputs(config, dev)
    seen = []

    def timed(rows, what):
        arr = np.array(rows, dtype=np.int64)
        ms = np.zeros(len(rows), dtype=np.float32)
        _lib.check(_lib.load().sv_run_ops_timed(arr.ctypes.data, len(rows), _lib.stream(), ms.ctypes.data), what)
        seen.append((arr, ms))

    chain._run = timed
    forwards = int(os.environ.get("FORWARDS", "15"))
    table = {}
    for dtype in ("float32", "float16"):
        backbone.set_eval_dtype(dtype)
        with torch.no_grad():
            for _ in range(3 + forwards):
                del seen[:]
                backbone(dict(batch))
                arr, ms = seen[0]
                for pos, (r, t) in enumerate(zip(arr, ms)):
                    if r[0] in (chain.OP_CONV_PLANNED, chain.OP_CONV_PLANNED_H16):
                        kd, nc = (int(r[3]), int(r[4])) if r[0] == chain.OP_CONV_PLANNED else (int(r[2]), int(r[3]))
                        table.setdefault((pos - (2 if dtype == "float16" else 1), kd, nc, int(r[10])), {}).setdefault(dtype, []).append(float(t))
        print(f"{config} {dtype}: route {backbone.last_eval_route}")
    for (k, kd, nc, n_rows), arms in sorted(table.items()):
        med = {d: sorted(v[3:])[len(v[3:]) // 2] * 1e3 for d, v in arms.items()}
        print(f"{config:11s} entry {k:2d} {kd:3d} -> {nc:3d} {n_rows:7d} rows: fp32 {med.get('float32', float('nan')):8.1f} us   fp16 {med.get('float16', float('nan')):8.1f} us")


def deviation():
    """max and 99.9th percentile of |fp16 list - fp32 list| / max |fp32 list| on the last tap, 2 and 16 scenes of the synthetic KITTI-shaped batch."""
    import torch
    dev = torch.device("cuda:0")
    for n in (2, 16):
        backbone, batch = _inputs("second", dev, n_scenes=n)
        outs = {}
        for dtype in ("float32", "float16"):
            backbone.set_eval_dtype(dtype)
            with torch.no_grad():
                outs[dtype] = backbone(dict(batch))["encoded_spconv_tensor"].features
            assert backbone.last_eval_route == ("half" if dtype == "float16" else "chain"), backbone.last_eval_route
        d = (outs["float16"] - outs["float32"]).abs().flatten().double() / float(outs["float32"].abs().max())
        k = max(int(0.999 * d.numel()), 1)
        print(f"VoxelBackBone8x {n:2d} scenes, {batch['voxel_coords'].shape[0]} voxels, last tap {tuple(outs['float32'].shape)}: "
              f"max |diff| / max |out| = {float(d.max()):.3e}, 99.9th percentile = {float(d.kthvalue(k).values):.3e}")


def child(config, dtype=None):
    import time
    import torch
    dev = torch.device("cuda:0")
    backbone, batch = _inputs(config, dev)
    if dtype is not None:
        backbone.set_eval_dtype(dtype)
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
                      "eval_chain": os.environ.get("SEEVCN_EVAL_CHAIN", "1") != "0", "route": backbone.last_eval_route, "ms_per_forward": round(s.elapsed_time(e) / forwards, 4),
                      "host_enqueue_ms_per_forward": round(host_ms, 4),
                      **({"host_split_median_ms": {k: round(sorted(v[-forwards:])[forwards // 2] * 1e3, 4) for k, v in split.items()}} if split else {})}))


def main():
    args = sys.argv[1:]
    dtype = None
    if "--dtype" in args:
        q = args.index("--dtype")
        dtype = args[q + 1]
        del args[q:q + 2]
    if args and args[0] == "--child":
        return child(args[1], dtype)
    if args and args[0] == "--layers":
        return layers(args[1] if len(args) > 1 else "second")
    if args and args[0] == "--deviation":
        return deviation()
    configs = args or ["second", "centerpoint"]
    repeats = int(os.environ.get("REPEATS", "5"))
    if dtype == "float16":
        return dtype_arms(configs, repeats)
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


def dtype_arms(configs, repeats):
    """The fp16 list against the fp32 list, one child process per arm and repeat, the order of the two arms rotating from repeat to repeat."""
    for config in configs:
        arms = {"float16": [], "float32": []}
        for rep in range(repeats):
            order = ("float16", "float32") if rep % 2 == 0 else ("float32", "float16")
            for arm in order:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, "--dtype", arm], capture_output=True, text=True, timeout=600)
                if out.returncode != 0:                             # nothing more is started on the GPU after a failed child
                    sys.stderr.write(out.stdout + out.stderr)
                    return out.returncode
                r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
                arms[arm].append(r)
                print(f"{config:11s} {r['backbone']:18s} rep {rep} {arm} (route {r['route']}): {r['ms_per_forward']:8.3f} ms / forward "
                      f"(host enqueue {r['host_enqueue_ms_per_forward']:.3f} ms, {r['voxels']} voxels)", flush=True)
        for arm in ("float16", "float32"):
            ms = [r["ms_per_forward"] for r in arms[arm]]
            print(f"{config:11s} {arm:11s}: min {min(ms):.3f}  median {sorted(ms)[len(ms) // 2]:.3f}  max {max(ms):.3f} ms / forward over {len(ms)} repeats")
    return 0


if __name__ == "__main__":
    sys.exit(main())
