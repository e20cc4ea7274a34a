"""The mesh ray caster at the size of one frame of the reference's VC dataset builder: 20 ellipsoid cars of 20 480 triangles each (icosphere at
subdivision 5), six pole cylinders, and one 1280 x 640 pinhole image per car cast from the lidar origin (dataset_functions.py:310-342).

    python tools/raycast_micro.py [--cars 20] [--subdivision 5] [--height 640] [--reps 10] > profiles/raycast.txt

Build (keys + sort + tree), cast (all cameras, one launch) and compaction (hit points + in-box crop) are timed separately with device events,
medians over --reps after a warm-up.  Library calls and host reads per frame are the package's COUNTERS.  The reference's Embree path needs open3d
and the parent commit has no ray caster, so the comparison is a plain-torch brute-force statement of the same arithmetic on the device, one
camera of 128 x 64 rays against the whole scene, and the numpy restatement (tests/raycast_reference.py) on the host for a 128-ray sample of that
camera; both are also compared with the kernel's answer.  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_frame(args):
    import raycast_reference as R
    rng = np.random.RandomState(0)
    v, f = R.icosphere(args.subdivision, 1.0, (0, 0, 0), (2.2, 0.9, 0.7))
    cars = []
    for k in range(args.cars):
        ang, dist, yaw = 2 * np.pi * k / args.cars + rng.uniform(-0.1, 0.1), rng.uniform(8, 40), rng.uniform(-np.pi, np.pi)
        centre = np.array([dist * np.cos(ang), dist * np.sin(ang), rng.uniform(-1.6, -1.0)])
        rmat = np.array([[np.cos(yaw), np.sin(yaw), 0], [-np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        bbox = np.array([[sx * 2.2, sy * 0.9, sz * 0.7] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]) @ rmat + centre
        cars.append({"vertices": (v.astype(np.float64) @ rmat + centre).astype(np.float32), "triangles": f, "label": list(centre) + [4.4, 1.8, 1.4, yaw],
                     "bbox": bbox})
    return cars


def torch_brute_force(rays, tris, chunk=128):
    """The stated arithmetic as plain torch elementwise operations (one rounding each: separate kernels, nothing contracted)."""
    import torch
    v0, e1, e2 = tris[:, 0][None], (tris[:, 1] - tris[:, 0])[None], (tris[:, 2] - tris[:, 0])[None]

    def cross(a, b):
        return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                            a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)

    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    t_hit, index = [], []
    for a in range(0, rays.shape[0], chunk):
        o, d = rays[a:a + chunk, None, :3], rays[a:a + chunk, None, 3:]
        p = cross(d, e2)
        det = dot(e1, p)
        inv = 1.0 / det
        s = o - v0
        u = dot(s, p) * inv
        q = cross(s, e1)
        v = dot(d, q) * inv
        t = dot(e2, q) * inv
        hit = (det != 0) & (u >= 0) & (v >= 0) & ((u + v) <= 1) & (t >= 0)
        t = torch.where(hit, t, torch.full_like(t, float("inf")))
        best = t.min(1)
        first = torch.where(t == best.values[:, None], torch.arange(t.shape[1], device=t.device)[None], t.shape[1]).min(1).values
        t_hit.append(best.values)
        index.append(torch.where(torch.isfinite(best.values), first, torch.full_like(first, -1)))
    return torch.cat(t_hit), torch.cat(index)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cars", type=int, default=20)
    ap.add_argument("--subdivision", type=int, default=5)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("raycast_micro: needs a GPU")
    import raycast_reference as R
    from seevcn_amd.vcn.vc_shapenet import dataset_functions as DF, raycasting as rc
    dev = torch.device("cuda:0")
    H, W = args.height, 2 * args.height
    cars = make_frame(args)
    rng = np.random.RandomState(1)
    scene = DF.populate_scene(cars, {}, rng, random_poles_pct=0.3, device=dev)      # int(20 * 0.3) = 6 pole cylinders
    fovs = [rng.normal(60, 30) for _ in cars]
    cams = rc.cameras_to_device([rc.pinhole_camera(f, car["label"][:3], [0, 0, 0], [0, 0, 1], W, H) for f, car in zip(fovs, cars)], dev)
    boxes = torch.tensor(np.array([car["label"] for car in cars], np.float32), device=dev)
    C, T = len(cars), scene.num_triangles
    print(f"raycast_micro: {C} cars of {len(cars[0]['triangles'])} triangles, {len(scene._meshes) - C} cylinders, {T} triangles in all; {C} cameras x {W} x {H} = "
          f"{C * W * H} rays; {args.reps} reps; {torch.cuda.get_device_name(0)}")

    def timed(fn, reps):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    def build():
        scene._built = None
        scene._build()

    state = {}

    def cast():
        state["ans"] = scene.cast_pinhole(cams, W, H)

    def compact():
        state["out"] = rc.hit_points(state["ans"]["t_hit"], C, W, H, cams=cams, boxes=boxes)

    # one frame as a user runs it: calls and reads
    rc.reset_counters()
    scene._built = None
    frame = DF.raycast_frame(cars, scene, np.random.RandomState(2), aspect_ratio=2, height_px=H)
    counters = dict(rc.COUNTERS)
    print(f"raycast_frame: library calls {counters['library_calls']} (keys, build, cast, hit points), host reads {counters['host_reads']}; "
          f"{sum(r['num_ray_pts'] for r in frame)} hit points, {sum(r['num_obj_pts'] for r in frame)} inside their car's box")
    del frame
    for label, fn in (("build (keys + torch.sort + tree + refit)", build), ("cast (all cameras, one launch)", cast), ("hit points + in-box crop (3 kernels)", compact)):
        med, lo, hi = timed(fn, args.reps)
        extra = f"   {C * W * H / med / 1e6:8.2f} G rays/s" if fn is cast else ""
        print(f"device  {label:42s} median {med:9.3f} ms   min {lo:9.3f} ms   max {hi:9.3f} ms{extra}")
    L_status = scene.status.cpu().tolist()
    counts = state["out"][3].cpu().numpy()
    print(f"status words {L_status} (not finite, stack full); hit share {counts[0].sum() / (C * W * H):.4f}, in-box share of the hits {counts[1].sum() / max(counts[0].sum(), 1):.4f}")

    # ---- the comparison: one camera of 128 x 64 rays against the whole scene
    w, h = 128, 64
    cam1 = rc.cameras_to_device([rc.pinhole_camera(fovs[0], cars[0]["label"][:3], [0, 0, 0], [0, 0, 1], w, h)], dev)
    tris = torch.cat(scene._meshes)
    rays = rc.rays_pinhole(cam1, w, h).reshape(-1, 6)
    small = {}

    def cast_small():
        small["ans"] = scene.cast_pinhole(cam1, w, h)

    def brute_small():
        small["torch"] = torch_brute_force(rays, tris)

    med_k, lo_k, _ = timed(cast_small, args.reps)
    med_t, lo_t, _ = timed(brute_small, 3)
    same_t = int((small["ans"]["t_hit"].view(torch.int32) == small["torch"][0].view(torch.int32)).sum())
    sizes = np.cumsum([0] + [int(m.shape[0]) for m in scene._meshes])
    g = small["ans"]["geometry_ids"].long()
    index_kernel = torch.where(g >= 0, torch.tensor(sizes[:-1], device=dev)[g.clamp(min=0)] + small["ans"]["primitive_ids"].long(), torch.full_like(g, -1))
    same_i = int((index_kernel == small["torch"][1]).sum())
    print(f"one camera {w} x {h} = {w * h} rays against {T} triangles:")
    print(f"device  kernel (hierarchy)                         median {med_k:9.3f} ms   min {lo_k:9.3f} ms")
    print(f"device  plain torch brute force                    median {med_t:9.3f} ms   min {lo_t:9.3f} ms   ratio {med_t / med_k:9.1f} x"
          f"   equal t_hit bits {same_t} of {w * h}, equal triangle {same_i} of {w * h}")
    pick = np.arange(0, w * h, w * h // 128)[:128]
    rays_h = rays.cpu().numpy()[pick]
    tris_h, gid, pid = tris.cpu().numpy(), np.repeat(np.arange(len(scene._meshes)), np.diff(sizes)).astype(np.int32), np.concatenate([np.arange(n) for n in np.diff(sizes)]).astype(np.int32)
    t0 = time.perf_counter()
    want = R.brute_force(rays_h, tris_h, gid, pid, np.float32, chunk=8)
    dt = time.perf_counter() - t0
    got_t = small["ans"]["t_hit"].cpu().numpy()[pick]
    same = int((got_t.view(np.uint32) == want["t_hit"].view(np.uint32)).sum())
    same_ids = int(((small["ans"]["geometry_ids"].cpu().numpy()[pick] == want["geometry_ids"]) & (small["ans"]["primitive_ids"].cpu().numpy()[pick] == want["primitive_ids"])).sum())
    print(f"host    numpy restatement, {len(pick)} of those rays       {1e3 * dt:9.1f} ms = {1e3 * dt / len(pick):.2f} ms a ray (the kernel: {1e3 * med_k / (w * h):.5f} us a ray)"
          f"   equal t_hit bits {same} of {len(pick)}, equal ids {same_ids} of {len(pick)}")
    print("one run on one machine; event-timed; no pass mark is set on any ratio")


if __name__ == "__main__":
    main()
