"""The VCN validation metrics at the validation shape (VC_cars.yaml: 1024 predicted rows against N_POINTS 16384), new route against the composed one.

    python tools/vc_metrics_micro.py [--batch 16] [--coarse 1024] [--complete 16384] [--reps 10] > profiles/vc_metrics.txt

new:      Metrics.get (sv_vc_metrics_objects + sv_vc_metrics_levels + one read): host-clock windows that end with the read, and device events around
          each of the two launches, with the module's COUNTERS.
composed: the same 30 values put together the reference's way from the entry points the library had before this route: ChamferDistanceL1/L2
          (ignore_zeros=True) on the masked subsets with one .item() each, boxes_iou3d_gpu on the masked boxes (a B x B matrix whose diagonal is
          used), get_bbox_from_keypoints, rotm_to_heading's torch ops, and get_oob_error as a host loop over the objects (numpy membership test, a
          set difference of row tuples, np.unique) in place of the reference's open3d crop.
The two routes alternate rep by rep on the same inputs; median / min / max over --reps after a warm-up.  The values of both are printed side by side
(they differ in the last digits: the composed route sums in torch's order).  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--coarse", type=int, default=1024)
    ap.add_argument("--complete", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vc_metrics_micro: needs a GPU")
    import vc_metrics_reference as R
    from seevcn_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils
    from seevcn_amd.vcn.extensions.chamfer_dist import ChamferDistanceL1, ChamferDistanceL2
    from seevcn_amd.vcn.utils import metrics as M
    from seevcn_amd.vcn.utils.bbox_utils import get_bbox_from_keypoints
    dev = torch.device("cuda:0")
    B = args.batch
    num_pts = [(4, 12, 40, 150, 400)[b % 5] for b in range(B)]
    case = R.make_case("micro", B, args.coarse, args.complete, num_pts, seed=99, zero_rows=(0,))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pred = {"coarse": t(case["coarse"]), "reg_rot": t(case["reg_rot"]), "reg_centre": t(case["reg_centre"])}
    gt = {"complete": t(case["complete"]), "gt_boxes": t(case["gt_boxes"]), "num_pts": np.array(num_pts)}
    print(f"vc_metrics_micro: {B} objects, {args.coarse} predicted rows against {args.complete} complete rows, {args.reps} reps, "
          f"{torch.cuda.get_device_name(0)}")

    cd1, cd2 = ChamferDistanceL1(ignore_zeros=True), ChamferDistanceL2(ignore_zeros=True)
    masks = [np.ones(B, bool)] + [(np.array(num_pts) >= lo) & (np.array(num_pts) <= hi) for _, lo, hi in R.LEVELS]

    def host_oob(pc, boxes):
        out = []
        for p, b in zip(pc.cpu().numpy(), boxes.cpu().numpy()):
            out.append(float(R.oob_ratio32(p, b)))
        return torch.from_numpy(np.array(out)).to(dev).float()

    def composed():
        ret = dict(pred)
        ret["pred_box"] = get_bbox_from_keypoints(ret["coarse"], gt["gt_boxes"])
        values = []
        for module in (cd1, cd2):
            for m in masks:
                mk = torch.from_numpy(m).to(dev)
                values.append(module(ret["coarse"][mk], gt["complete"][mk]).item() * 1000 if m.any() else -1)
        for m in masks:
            mk = torch.from_numpy(m).to(dev)
            values.append(host_oob(ret["coarse"][mk], gt["gt_boxes"][mk]).mean().item() if m.any() else -1)
        for m in masks:
            mk = torch.from_numpy(m).to(dev)
            values.append(iou3d_nms_utils.boxes_iou3d_gpu(ret["pred_box"][mk], gt["gt_boxes"][mk]).diag().mean().item() if m.any() else -1)
        for m in masks:
            mk = torch.from_numpy(m).to(dev)
            if not m.any():
                values.append(-1)
                continue
            v = ret["reg_rot"][mk][:, 0, :]
            nrm = torch.linalg.norm(v, dim=1)
            values.append(torch.abs(torch.atan2(v[:, 1] / nrm, v[:, 0] / nrm) - gt["gt_boxes"][:, -1][mk]).median().item())
        for m in masks:
            mk = torch.from_numpy(m).to(dev)
            values.append(torch.abs(ret["reg_centre"][mk] - gt["gt_boxes"][:, :3][mk]).mean().item() if m.any() else -1)
        return values

    M.reset_counters()
    new_values = M.Metrics.get(pred, gt)
    counters = dict(M.COUNTERS)
    old_values = composed()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        M.Metrics.get(pred, gt)
        t_new.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        composed()
        t_old.append(1e3 * (time.perf_counter() - t0))
    stat = lambda ts: f"median {np.median(ts):9.3f} ms   min {np.min(ts):9.3f}   max {np.max(ts):9.3f}"
    print(f"new      Metrics.get, wall to the read      {stat(t_new)}   library calls {counters['library_calls']}, host reads {counters['host_reads']}")
    print(f"composed the same 30 values, wall           {stat(t_old)}   30 .item() reads, {B} objects through the host loop x 2 groups each")
    print(f"ratio of the medians (composed / new): {np.median(t_old) / np.median(t_new):.1f}")

    num = M._num_pts_device(gt["num_pts"], dev)
    out = torch.empty(30, dtype=torch.float32, device=dev)
    table = M.objects_table(pred["coarse"], gt["complete"], gt["gt_boxes"], pred["reg_rot"], pred["reg_centre"])

    def event_time(fn):
        ts = []
        for i in range(args.reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ts.append(a.elapsed_time(b))
        return ts

    objs = event_time(lambda: M.objects_table(pred["coarse"], gt["complete"], gt["gt_boxes"], pred["reg_rot"], pred["reg_centre"]))
    from seevcn_amd import _lib as L
    lev = event_time(lambda: M.call("sv_vc_metrics_levels", L.ptr(table), L.ptr(num), B, L.ptr(out), L.stream()))
    evals = 2.0 * B * args.coarse * args.complete
    print(f"kernel   sv_vc_metrics_objects (device events) {stat(objs)}   {evals / 1e6:.0f} M distance evaluations, "
          f"{evals / (np.median(objs) * 1e-3) / 1e9:.1f} G evaluations/s on {B} workgroups")
    print(f"kernel   sv_vc_metrics_levels  (device events) {stat(lev)}")
    print("values   name                    new             composed")
    for name, a, b in zip(M.Metrics.names(), new_values, old_values):
        print(f"         {name:22s} {a:15.7g} {b:15.7g}")


if __name__ == "__main__":
    main()
