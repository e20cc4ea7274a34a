"""The VC_cars train queue (LidarSimulation, ResamplePoints(1024)) on a batch of 32 ring-like objects of about 3000 points each.

    python tools/lidar_sim_micro.py [--batch 32] [--points 3000] [--reps 20] > profiles/lidar_sim.txt

Device: the three kernels timed one by one with device events (median over --reps after a warm-up), and the wall time of BatchCompose.forward with its
one host read, host draws and uploads.  Host: the numpy route the reference takes per sample (cart2sph, np.histogram(bins='sqrt'), digitize, in1d,
unique, two strided picks, the spherical round trip, tile + permutation), restated here, on the same machine, with the same seeds; its float32 cast
is compared with the device's output.  Also measured: the largest difference, in ulps, between the device's float64 elevations and numpy's, over the
batch and over the clouds of tests/golden/vc_transforms.npz.  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def host_queue(pts, rng, n_points=1024, min_in_pts=100, min_out_pts=30, max_sel=30):
    """One sample through Compose([LidarSimulation, ResamplePoints]) as the reference computes it: float64 numpy, rng in Compose's order."""
    def cart2sph(p):
        return np.stack([np.linalg.norm(p, axis=1), np.arctan2(p[:, 1], p[:, 0]), np.arctan2(np.linalg.norm(p[:, :2], axis=1), p[:, 2])], 1)

    def sph2cart(s):
        return np.stack([s[:, 0] * np.sin(s[:, 2]) * np.cos(s[:, 1]), s[:, 0] * np.sin(s[:, 2]) * np.sin(s[:, 1]), s[:, 0] * np.cos(s[:, 2])], 1)

    def lidar(pts):
        if len(pts) < min_in_pts:
            return pts
        sph = cart2sph(pts)
        hist = np.histogram(sph[:, 2], bins='sqrt')
        ring = np.digitize(sph[:, 2], hist[1][np.argwhere(hist[0] > 0).squeeze(1)])
        num_rings = max(ring)
        step = rng.randint(1, max(np.ceil(num_rings * 0.3), 2))
        chosen = np.unique(ring)[rng.randint(0, max(np.ceil(num_rings * 0.1), 1))::step]
        mask = np.in1d(ring, chosen)
        onetwo = rng.choice([False, True], replace=False, p=[0.8, 0.2]) and len(chosen) > 2
        if onetwo:
            onetwo_mask = np.in1d(ring, rng.choice(chosen, size=rng.randint(1, 3)))
        _, counts = np.unique(ring[mask], return_counts=True)
        hstep = rng.randint(1, max(np.ceil(min(counts) * 0.5), 2))
        out = sph2cart(sph[mask][rng.randint(0, min(counts))::hstep])
        if onetwo:
            few = sph2cart(sph[onetwo_mask][rng.randint(0, min(counts))::min(max_sel, hstep)])
            return out if len(few) < min_out_pts else few
        return out if len(out) > min_out_pts else pts

    rng.uniform(0, 1)
    pts = lidar(pts)
    rng.uniform(0, 1)
    tiled = np.tile(pts, (int(np.ceil(n_points / len(pts))), 1))
    return tiled[rng.permutation(tiled.shape[0])[:n_points]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lidar_sim_micro: needs a GPU")
    import vc_transforms_reference as V
    from seevcn_amd.vcn.datasets import data_transforms as T
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    clouds = [V.ring_cloud(100 + b, int(args.points + rng.randint(-300, 301)), int(rng.randint(16, 41))) for b in range(args.batch)]
    counts = np.array([len(c) for c in clouds])
    points = torch.from_numpy(np.concatenate(clouds)).to(dev)
    print(f"lidar_sim_micro: {args.batch} objects of {counts.min()}..{counts.max()} points ({counts.sum()} in all), VC_cars train queue "
          f"(LidarSimulation, ResamplePoints(1024)); {args.reps} reps; {torch.cuda.get_device_name(0)}")

    # ---- elevations: the device's float64 atan2 against numpy's
    for label, cl in (("this batch", clouds), ("the golden's 14 clouds", V.make_cases()[1])):
        st = T.StackedClouds(torch.from_numpy(np.concatenate(cl)).to(dev), [len(c) for c in cl])
        _, _, elev = T.vc_rings(st, 0, 0, with_elevation=True)
        want = V.elevation(np.concatenate(cl))
        ulps = np.abs(elev.cpu().numpy() - want) / np.spacing(want)
        print(f"elevation, device float64 atan2 against numpy, {label}: largest difference {ulps.max():.2f} ulps, {int((ulps > 0).sum())} of {len(want)} "
              f"differ (the tests allow 16; the golden's clouds keep 64 from every inner bin edge)")

    # ---- the queue as a user runs it
    compose = T.BatchCompose(V.VC_CARS_TRAIN)
    batch = {"partial": points, "partial_cnt": counts}
    walls = []
    for rep in range(args.reps + 2):
        rngs = [np.random.RandomState(1000 + b) for b in range(args.batch)]
        T.reset_counters()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = compose.forward(batch, rngs)
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    walls = walls[2:]
    print(f"device  BatchCompose.forward, wall (draws, uploads, 1 read)  median {np.median(walls):8.3f} ms   min {np.min(walls):8.3f} ms   = "
          f"{1e3 * np.median(walls) / args.batch:7.1f} us a sample; library calls {T.COUNTERS['library_calls']}, host reads {T.COUNTERS['host_reads']}")

    # ---- the kernels one by one
    st = T.StackedClouds(points, counts)
    ring, table, _ = T.vc_rings(st, 0, 100)
    num_rings, ring_cnt = T.read_ring_table(table, args.batch)
    plans = [T.plan_lidar_simulation(np.random.RandomState(1000 + b), int(n), int(r), c) for b, (n, r, c) in enumerate(zip(counts, num_rings, ring_cnt))]
    plan_table = torch.from_numpy(T.pack_plans([p for p, _ in plans], [m for _, m in plans])).to(dev)
    lengths = np.array([m for _, m in plans])
    sel = torch.empty(int(lengths.sum()), 3, device=dev)
    T.call("sv_vc_select", *st.args(), T.L.ptr(ring), None, T.L.ptr(plan_table), T.L.ptr(sel), T.L.stream())
    st2 = T.StackedClouds(sel, lengths)
    index = torch.from_numpy(np.stack([T.draw_resample(np.random.RandomState(b), int(n), 1024) for b, n in enumerate(lengths)]).astype(np.int32)).to(dev)
    res = torch.empty(args.batch, 1024, 3, device=dev)
    elev = torch.empty(int(counts.sum()), dtype=torch.float64, device=dev)

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(np.min(ms))

    kernels = (("sv_vc_rings (elevations computed twice)", lambda: T.call("sv_vc_rings", *st.args(), 0, 100, T.L.ptr(ring), T.L.ptr(table[:args.batch]), T.L.ptr(table[args.batch:]), None, T.L.stream())),
               ("sv_vc_rings (elevations stored)", lambda: T.call("sv_vc_rings", *st.args(), 0, 100, T.L.ptr(ring), T.L.ptr(table[:args.batch]), T.L.ptr(table[args.batch:]), T.L.ptr(elev), T.L.stream())),
               ("sv_vc_select", lambda: T.call("sv_vc_select", *st.args(), T.L.ptr(ring), None, T.L.ptr(plan_table), T.L.ptr(sel), T.L.stream())),
               ("sv_vc_resample", lambda: T.call("sv_vc_resample", *st2.args(), T.L.ptr(index), 1024, T.L.ptr(res), T.L.stream())))
    for label, fn in kernels:
        med, lo = timed(fn)
        print(f"device  {label:42s} median {1e3 * med:8.1f} us   min {1e3 * lo:8.1f} us")
    print(f"        rings per object {num_rings.min()}..{num_rings.max()}; rows kept {lengths.min()}..{lengths.max()}; exits "
          + ", ".join(f"{e} {[p['exit'] for p, _ in plans].count(e)}" for e in ("out", "onetwo", "onetwo_fallback", "original")))

    # ---- the host route on the same machine, same seeds
    t0 = time.perf_counter()
    host = [host_queue(c.astype(np.float64), np.random.RandomState(1000 + b)) for b, c in enumerate(clouds)]
    dt = 1e3 * (time.perf_counter() - t0)
    same = int((np.stack(host).astype(np.float32).view(np.uint32) == out["partial"].cpu().numpy().view(np.uint32)).all(axis=(1, 2)).sum())
    print(f"host    numpy route of the reference, per sample          total  {dt:8.3f} ms   = {1e3 * dt / args.batch:7.1f} us a sample   "
          f"(wall ratio host / device {dt / np.median(walls):.2f}); samples with every bit equal after the float32 cast: {same} of {args.batch}")
    print("one run on one machine; kernels event-timed, the rest wall time; reported, no pass mark is set on any number")


if __name__ == "__main__":
    main()
