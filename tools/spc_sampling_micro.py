"""SPC keypoint sampling at pv_rcnn_plusplus.yaml sizes (2 scenes, 4096 keypoints, 6 sectors, radius 1.6, the TEST NMS_POST_MAXSIZE = 100 RoIs) at two
scene sizes, the bench's ~21 k points and a Waymo-like 180 k: time per call of the three kernels (sv_spc_select, sv_spc_partition,
sv_stack_farthest_point_sampling_ragged) and of the whole VoxelSetAbstraction.get_sampled_points, with launches and host reads of one call.  Beside
them two baselines: (a) the same keypoints from the reference's Python statements (voxel_set_abstraction.py:45-121) run on the GPU scene by scene over
this library's ragged FPS, (b) today's FPS of 4096 keypoints from the full scenes.  Every kernel is compared element for element with a plain-torch
statement before anything is timed; a difference is written into the record and fails the run.

Device events around windows of calls behind a warm-up, medians with their range; kernel time and launch count of ONE call from torch.profiler.
Needs a GPU (--rehearse: small sizes on the CPU, the torch statements against the numpy restatement of tests/spc_reference.py, stop).

    python tools/spc_sampling_micro.py [--out profiles/spc_sampling.txt] [--windows 15] [--calls 10]
"""
import argparse
import math
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vector_pool_micro import kernels_of_one_call, timed  # noqa: E402

K, S, RADIUS, NUM_ROIS, BAND = 4096, 6, 1.6, 100, 1e-5


def make_inputs(n_per_scene, num_rois=NUM_ROIS, seed=7):
    """Two scenes around the sensor (+-75 m): a ground sheet plus clusters at the RoIs; 80 live RoIs and zero rows up to num_rois, like a padded NMS block."""
    rng = np.random.default_rng(seed)
    xyz, rois = [], []
    for b in range(2):
        live = num_rois * 4 // 5
        c = rng.uniform([-70, -70, -1.0], [70, 70, 1.0], (live, 3))
        r = np.concatenate([c, rng.uniform([1.5, 0.6, 1.2], [5, 2.2, 2], (live, 3)), rng.uniform(-3, 3, (live, 1))], 1)
        r = np.concatenate([r, np.zeros((num_rois - live, 7))])
        n = n_per_scene + (b * 37)                                                                 # ragged
        near = c[rng.integers(0, live, n // 3)] + rng.normal(0, 1.5, (n // 3, 3)) * np.array([1.0, 1.0, 0.3])
        far = rng.uniform([-75, -75, -2.0], [75, 75, 0.5], (n - len(near), 3))
        xyz.append(np.concatenate([near, far])[rng.permutation(n)].astype(np.float32))
        rois.append(r.astype(np.float32))
    cnt = np.array([len(p) for p in xyz], np.int32)
    return np.concatenate(xyz), cnt, np.stack(rois)


def torch_select(points, rois, radius):
    """sample_points_with_roi's mask for one scene, plain torch with the products summed left to right"""
    d = points[:, None, :] - rois[None, :, 0:3]
    dist = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    min_dis, j = dist.min(dim=-1)
    h = rois[:, 3:6] / 2
    max_dim = torch.sqrt(h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1] + h[:, 2] * h[:, 2])
    return min_dis < max_dim[j] + radius


def torch_sector(points, num_sectors):
    ang = torch.atan2(points[:, 1], points[:, 0]) + np.pi
    return (ang / (np.pi * 2 / num_sectors)).floor().clamp(min=0, max=num_sectors)


def torch_partition(sector, start, cnt, k, num_sectors):
    """order and tables from boolean masks, one nonzero per (scene, bucket) -- for scenes that take neither fallback"""
    order = torch.full_like(sector, -1)
    rows_t, tab = [], []
    for b, (s, n) in enumerate(zip(start, cnt)):
        sec = sector[s:s + n]
        n_sel = int((sec >= 0).sum())
        pos, out = s, b * (k + num_sectors)
        for q in range(num_sectors + 1):
            rows = torch.nonzero(sec == q)[:, 0] + s
            order[pos:pos + len(rows)] = rows.to(order.dtype)
            if q < num_sectors:
                m = min(len(rows), math.ceil(len(rows) / n_sel * k))
                tab.append((pos, len(rows), m, out))
                out += m
            pos += len(rows)
        rows_t.append(out - b * (k + num_sectors))
    return order, torch.tensor(tab, dtype=torch.int32).t().contiguous(), rows_t


def torch_fps(points, m):
    """plain farthest point sampling (first maximum wins; random data has no ties)"""
    temp = torch.full((len(points),), 1e10, device=points.device)
    out, old = [0], 0
    for _ in range(1, m):
        d = points - points[old]
        temp = torch.minimum(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], temp)
        old = int(torch.argmax(temp))
        out.append(old)
    return out


def reference_statements(xyz, start, cnt, rois, ops_utils):
    """baseline (a): voxel_set_abstraction.py:45-121 statement by statement on the GPU, scene by scene, over the library's ragged FPS"""
    keypoints = []
    for b, (s, n) in enumerate(zip(start, cnt)):
        points = xyz[s:s + n]
        mask = torch_select(points, rois[b], RADIUS)
        sampled = points[:1] if mask.sum() == 0 else points[mask, :]
        sector_idx = torch_sector(sampled, S)
        pts, bc, mc = [], [], []
        for q in range(S):
            sm = sector_idx == q
            c = sm.sum().item()
            if c > 0:
                pts.append(sampled[sm])
                bc.append(c)
                mc.append(min(c, math.ceil(c / sampled.shape[0] * K)))
        if not bc:
            pts, bc, mc = [sampled], [len(sampled)], [K]
        cat = torch.cat(pts, dim=0)
        idx = ops_utils.stack_farthest_point_sample(cat.contiguous(), torch.tensor(bc, device=xyz.device).int(), torch.tensor(mc, device=xyz.device).int())
        keypoints.append(cat[idx.long()])
    return torch.cat(keypoints)


def rehearse():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spc_reference as R
    xyz, cnt, rois = make_inputs(900, num_rois=20)
    start = np.cumsum(cnt) - cnt
    sector = R.select(xyz, start, cnt, rois, RADIUS, S)
    t = torch.from_numpy(xyz)
    got = torch.cat([torch_select(t[s:s + n], torch.from_numpy(rois[b]), RADIUS) for b, (s, n) in enumerate(zip(start, cnt))]).numpy()
    assert np.array_equal(got, sector >= 0), "torch statement of the selection differs"
    q = R.sector_quotient(xyz, S)
    clear = np.abs(q - np.round(q)) > BAND
    assert np.array_equal(torch_sector(t, S).numpy()[clear & got], sector[clear & got]), "torch statement of the sector differs"
    want = R.partition(sector, xyz, start, cnt, 64, S)
    order, tab, kp = torch_partition(torch.from_numpy(sector), start.tolist(), cnt.tolist(), 64, S)
    assert np.array_equal(order.numpy()[want["order"] >= 0], want["order"][want["order"] >= 0]) and kp == want["kp_cnt"].tolist()
    for i, k in enumerate(("seg_start", "seg_cnt", "seg_m", "seg_out_start")):
        assert np.array_equal(tab[i].numpy(), want[k]), k
    seg = xyz[want["order"][want["seg_start"][0]:want["seg_start"][0] + want["seg_cnt"][0]]]
    assert torch_fps(torch.from_numpy(seg), 16) == R.fps_segment(seg, 16).tolist()
    print(f"rehearsal: {len(xyz)} points, {int((sector >= 0).sum())} selected, keypoints {want['kp_cnt'].tolist()}: torch statements == restatement")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        return rehearse()
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models.backbones_3d.pfe.voxel_set_abstraction import VoxelSetAbstraction
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as ext, pointnet2_utils as ops_utils
    assert torch.cuda.is_available(), "spc_sampling_micro needs a GPU (--rehearse runs the statements on the CPU)"
    dev = torch.device("cuda:0")
    lines = [f"SPC keypoint sampling at pv_rcnn_plusplus.yaml sizes: 2 scenes, K {K}, S {S}, radius {RADIUS}, {NUM_ROIS} RoIs; per call: median of windows "
             "(min .. max), launches and kernel time of one call"]
    differ = []

    def agree(name, got, want):
        n = int((got != want).sum()) if got.shape == want.shape else -1
        if n:
            differ.append(f"{name}: kernel and torch statement differ in {n} of {got.numel()} elements")
            lines.append("!! " + differ[-1])

    def host_reads(fn):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return sum("synchroniz" in str(x.message).lower() for x in w)

    def report(name, fn, note="", slow=False, reads=False):
        windows, calls = (5, 2) if slow else (a.windows, a.calls)
        for _ in range(1 if slow else 3):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, windows, calls)
        launches, kernel_ms = kernels_of_one_call(fn)
        k = "profiler: not measured" if launches is None else f"{launches} launches, kernel time {kernel_ms:.3f} ms"
        if reads:
            k += f", {host_reads(fn)} host reads"
        lines.append(f"{name:<58s} median {ms[len(ms) // 2]:9.3f} ms   min {ms[0]:9.3f}   max {ms[-1]:9.3f}   ({len(ms)} x {calls} calls)   {k}   {note}")
        print(lines[-1], flush=True)

    pfe, _, _ = C.pvrcnnpp_cfg(features_source=('raw_points',))
    vsa = VoxelSetAbstraction(pfe, voxel_size=C.DA_VOXEL, point_cloud_range=C.DA_RANGE, num_bev_features=0, num_rawpoint_features=5).to(dev)
    with torch.no_grad():
        for n_scene in (21000, 180000):
            xyz, cnt, rois = make_inputs(n_scene)
            start = (np.cumsum(cnt) - cnt).tolist()
            d_xyz, d_cnt, d_rois = (torch.from_numpy(v).to(dev) for v in (xyz, cnt, rois))
            max_n = int(cnt.max())
            lines.append(f"-- scenes of {cnt.tolist()} points")
            # ---- each kernel against its torch statement
            sector = ext.spc_select(d_xyz, d_cnt, d_rois, RADIUS, S, max_n)
            t_mask = torch.cat([torch_select(d_xyz[s:s + n], d_rois[b], RADIUS) for b, (s, n) in enumerate(zip(start, cnt.tolist()))])
            agree("select mask", sector >= 0, t_mask)
            q = torch.atan2(d_xyz[:, 1].double(), d_xyz[:, 0].double()).add(np.pi).div(np.pi * 2 / S)
            clear = ((q - q.round()).abs() > BAND) & t_mask
            t_sec = torch_sector(d_xyz, S).to(torch.int32)
            agree("sector (rows further than 1e-5 from a sector edge)", sector[clear], t_sec[clear])
            order, tables = ext.spc_partition(sector, d_xyz, d_cnt, K, S)
            t_order, t_tab, t_kp = torch_partition(sector, start, cnt.tolist(), K, S)
            agree("partition tables", tables[:4].cpu(), t_tab)
            agree("partition order", order[t_order >= 0], t_order[t_order >= 0])
            assert tables[4][:2].tolist() == t_kp
            idx = torch.empty((2 * (K + S),), dtype=torch.int32, device=dev)
            ext.stack_farthest_point_sampling_ragged(d_xyz, order, tables[0], tables[1], tables[2], tables[3], idx, max_n)
            seg0 = order[int(tables[0][0]):int(tables[0][0]) + int(tables[1][0])].long()
            head = min(256, int(tables[2][0]))
            agree("ragged FPS (first picks of the first segment)", idx[:head].cpu(), seg0[torch_fps(d_xyz[seg0], head)].to(torch.int32).cpu())
            batch = {"batch_size": 2, "points": torch.cat([torch.repeat_interleave(torch.arange(2, device=dev), d_cnt.long()).float()[:, None], d_xyz,
                                                           torch.zeros((len(xyz), 2), device=dev)], 1), "rois": d_rois, "points_per_scene": cnt.tolist()}
            keypoints = vsa.get_sampled_points(dict(batch))
            agree("keypoints against the reference's statements", keypoints[:, 1:4], reference_statements(d_xyz, start, cnt.tolist(), d_rois, ops_utils))
            sel = (sector >= 0).sum().item()
            segs = tables[1].tolist()
            note = f"[{sel} of {len(xyz)} points selected; segments {segs}; quotas {tables[2].tolist()}]"
            # ---- times
            report("select    sv_spc_select", lambda: ext.spc_select(d_xyz, d_cnt, d_rois, RADIUS, S, max_n), note)
            report("partition sv_spc_partition", lambda: ext.spc_partition(sector, d_xyz, d_cnt, K, S))
            report("fps       sv_stack_farthest_point_sampling_ragged",
                   lambda: ext.stack_farthest_point_sampling_ragged(d_xyz, order, tables[0], tables[1], tables[2], tables[3], idx, max_n),
                   f"[{max(tables[2].tolist())} rounds in the longest segment]")
            report("whole     VoxelSetAbstraction.get_sampled_points (SPC)", lambda: vsa.get_sampled_points(dict(batch)), reads=True)
            report("(a)       the reference's statements, scene by scene", lambda: reference_statements(d_xyz, start, cnt.tolist(), d_rois, ops_utils), reads=True)
            report(f"(b)       FPS of {K} keypoints from the full scenes", lambda: ext.stack_farthest_point_sampling(d_xyz, d_cnt, K, max_n), slow=n_scene > 65536)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if differ:
        raise SystemExit("\n".join(differ))


if __name__ == "__main__":
    main()
