"""The four anchor entries of csrc/head.hip, event-timed on the inputs of two goldens:

  plain   sv_assign_targets_axis_aligned / sv_anchor_decode at the shape of tests/golden/second_head.npz: SECOND's single head, 2 scenes,
          211 200 anchors in 3 sets, 24 ground-truth boxes per scene, 2 direction bins
  coded   sv_assign_targets_axis_aligned_coded / sv_anchor_decode_coded on the coded case of tests/golden/multihead_inputs.py: 2 scenes,
          144 head-major anchors of 9 numbers, sin/cos heading, 6 boxes per scene (launch-bound: it times the entry, not the kernel)
  wide    the coded entries in the old layout (E = 0, sincos = 0, set_major = 0) on the plain inputs: the wide instantiation at the large shape

The plain and wide rows are compared bit for bit before anything is timed.  Device events around windows of calls behind a warm-up; median,
min and max of the windows in microseconds per call, and the summed kernel time of a call from torch.profiler (mean of 50 calls; the memset of
the assignment counts as a launch).  SEEVCN_LIB selects the library.  Needs a GPU.

    python tools/anchor_micro.py [--out FILE] [--windows 15] [--calls 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from vector_pool_micro import kernels_of_one_call, timed  # noqa: E402


def plain_inputs(dev):
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import dense_heads
    g = np.load(os.path.join(ROOT, "tests", "golden", "second_head.npz"))
    head = dense_heads.__all__["AnchorHeadSingle"](model_cfg=C.SECOND_DENSE_HEAD, input_channels=16, num_class=3, class_names=C.CLASS_NAMES,
                                                   grid_size=np.array([1408, 1600, 40]), point_cloud_range=np.array(C.KITTI_RANGE, np.float32)).to(dev)
    return head, torch.from_numpy(g["gt_boxes"]).to(dev), 0, 0, 0, 2, C.SECOND_DENSE_HEAD


def coded_inputs(dev):
    import multihead_inputs as I
    head = I.build_head("coded").to(dev)
    car = head.anchors[0].reshape(-1, head.anchors[0].shape[-1])[0, :7].cpu().numpy()
    return head, torch.from_numpy(I.gt_boxes(car)).to(dev), 2, 1, 1, 0, I.HEAD_CODED


def entries(lib, L, head, gt, E, sincos, set_major, bins, cfg, coded, seed):
    """(assign, decode, outputs): closures over preallocated tensors, one call of the entry each"""
    dev = gt.device
    anchors = head._anchors_on(dev)                                # moves head.anchors to the device first
    t = head.target_assigner._device_tables(head.anchors)
    B, G, A = gt.shape[0], gt.shape[1], t["anchors"].shape[0]
    gt = gt.contiguous().float()
    labels = torch.empty((B, A), dtype=torch.int32, device=dev)
    targets = torch.empty((B, A, 7 + sincos + E), device=dev)
    weights = torch.empty((B, A), device=dev)
    scratch = torch.empty((B * G,), device=dev)
    rng = np.random.default_rng(seed)
    enc = torch.from_numpy((rng.normal(size=(B, A, 7 + sincos + E)) * 0.5).astype(np.float32)).to(dev)
    dirs = torch.from_numpy(rng.normal(size=(B, A, bins)).astype(np.float32)).to(dev) if bins else None
    out = torch.empty((B, A, 7 + E), device=dev)
    tail = (t["per_loc"], len(head.anchors), L.ptr(t["offs"]), L.ptr(t["cls"]), L.ptr(t["mthr"]), L.ptr(t["uthr"]), L.ptr(gt), B, G, L.ptr(scratch),
            L.ptr(labels), L.ptr(targets), L.ptr(weights))
    dtail = (L.ptr(enc), L.ptr(dirs) if bins else None, B, bins, float(cfg.get("DIR_OFFSET", 0.0)), float(cfg.get("DIR_LIMIT_OFFSET", 0.0)), L.ptr(out))
    # every argument converted once: a call below is one foreign call, so that the small shape times the entry and not the conversions
    code = (E, sincos, set_major) if coded else ()
    aargs = (L.ptr(t["anchors"]), A, *code, *tail, L.stream())
    dargs = (L.ptr(anchors), A, *code[:2], *dtail, L.stream())
    fa = lib.sv_assign_targets_axis_aligned_coded if coded else lib.sv_assign_targets_axis_aligned
    fd = lib.sv_anchor_decode_coded if coded else lib.sv_anchor_decode

    def assign():
        L.check(fa(*aargs), "assign")

    def decode():
        L.check(fd(*dargs), "decode")
    keep = (gt, enc, dirs, scratch)                                # the raw pointers above do not hold their tensors
    return assign, decode, (labels, targets, weights, out), f"{B} x {A} anchors, {G} boxes a scene", keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import seevcn_amd._lib as L
    assert torch.cuda.is_available(), "anchor_micro needs a GPU"
    dev = torch.device("cuda:0")
    lib = L.load()
    plain, coded = plain_inputs(dev), coded_inputs(dev)
    rows = [("plain", entries(lib, L, *plain, coded=False, seed=1)), ("wide", entries(lib, L, *plain, coded=True, seed=1)),
            ("coded", entries(lib, L, *coded, coded=True, seed=2))]
    for _, (assign, decode, _, _, _) in rows:
        assign(), decode()
    torch.cuda.synchronize()
    same = all(torch.equal(p.view(torch.int32), w.view(torch.int32)) for p, w in zip(rows[0][1][2], rows[1][1][2]))
    lines = [f"anchor entries, library {L.LIB_PATH}", f"wide entries in the old layout == plain entries bit for bit: {same}",
             f"positives: plain {int((rows[0][1][2][0] > 0).sum())}, coded {int((rows[2][1][2][0] > 0).sum())}"]
    print("\n".join(lines), flush=True)
    for name, (assign, decode, _, shape, _) in rows:
        for what, fn in (("assign", assign), ("decode", decode)):
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            us = [1e3 * m for m in timed(fn, a.windows, a.calls)]
            launches, kernel_ms = kernels_of_one_call(lambda: [fn() for _ in range(50)])
            k = "profiler: not measured" if launches is None else f"{launches / 50:g} launches, kernel time {1e3 * kernel_ms / 50:7.2f} us a call"
            lines.append(f"{name + ' ' + what:<14s} median {us[len(us) // 2]:8.2f} us   min {us[0]:8.2f}   max {us[-1]:8.2f}   ({len(us)} x {a.calls} calls; {shape})   {k}")
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not same:
        raise SystemExit("the wide entries differ from the plain ones")


if __name__ == "__main__":
    main()
