"""Class-wise post-processing of AnchorHeadMulti at cbgs_second_multihead.yaml sizes: 4 scenes, feature map 128 x 128, 10 classes in 6 heads
(2 rotations: 32 768 anchors per class), SCORE_THRESH 0.1, NMS_PRE_MAXSIZE 1000, NMS_POST_MAXSIZE 83, NMS_THRESH 0.2.  Seeded logits shaped so
that several hundred boxes per class and scene pass the threshold.  Two paths over the same input, compared element for element before anything
is timed:

  batched   model_nms_utils.multi_classes_nms_batch: one top-k per head, one sv_nms_segments launch pair for all 40 box sets, one host read
  loop      the reference's statement on this library: per scene, head and class a mask, a top-k and nms_gpu (sv_nms_prefix, one host read each)

Device events around windows of calls behind a warm-up, medians with their range; launches and kernel time of ONE call from torch.profiler, host
reads of one call from torch's sync debug mode.  Needs a GPU (--rehearse: a small size on the CPU-built inputs only, prints the counts, stop).

    python tools/multihead_post_micro.py [--out profiles/multihead_post.txt] [--windows 15] [--calls 5]
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vector_pool_micro import kernels_of_one_call, timed  # noqa: E402

SCENES, FM, ROTS = 4, 128, 2
HEADS = [1, 2, 2, 1, 2, 2]                                      # classes per head
NMS = dict(MULTI_CLASSES_NMS=True, NMS_TYPE='nms_gpu', NMS_THRESH=0.2, NMS_PRE_MAXSIZE=1000, NMS_POST_MAXSIZE=83)
SCORE_THRESH = 0.1
PASS_PER_CLASS = 600                                            # boxes of one class and scene above the threshold, about


def make_inputs(fm=FM, seed=3, pass_per_class=PASS_PER_CLASS):
    """logits [(B, A_h, C_h)] and boxes (B, A, 9): anchors on the map (102.4 m square) with jitter; pass_per_class anchors of every class and
    scene, within 3 m of 60 object centres so that NMS has work, get distinct logits above SCORE_THRESH, all others -8"""
    rng = np.random.default_rng(seed)
    per_class = ROTS * fm * fm
    ys, xs = np.meshgrid(np.linspace(-51.2, 51.2, fm), np.linspace(-51.2, 51.2, fm), indexing="ij")
    logits, boxes = [], []
    for classes in HEADS:
        lg = np.full((SCENES, classes * per_class, classes), -8.0, np.float32)
        for c in range(classes):
            a = np.zeros((SCENES, per_class, 9), np.float32)
            a[..., 0] = np.tile(xs.reshape(-1), ROTS) + rng.normal(size=(SCENES, per_class)) * 0.3
            a[..., 1] = np.tile(ys.reshape(-1), ROTS) + rng.normal(size=(SCENES, per_class)) * 0.3
            a[..., 2] = -1.0
            a[..., 3:6] = np.array([4.6, 1.9, 1.7], np.float32) * np.exp(rng.normal(size=(SCENES, per_class, 3)) * 0.1)
            a[..., 6] = np.repeat(np.array([0.0, 1.57], np.float32), fm * fm) + rng.normal(size=(SCENES, per_class)) * 0.2
            a[..., 7:9] = rng.normal(size=(SCENES, per_class, 2))
            boxes.append(a)
            for b in range(SCENES):
                centres = rng.uniform(-45, 45, size=(60, 2))
                d = np.sqrt(((a[b, :, None, 0:2] - centres[None]) ** 2).sum(-1)).min(1)
                near = np.nonzero(d < 3.0)[0]
                pick = rng.choice(near, size=min(pass_per_class, len(near)), replace=False)
                lg[b, c * per_class + pick, c] = rng.permutation(np.linspace(-2.0, 3.0, len(pick))).astype(np.float32)   # distinct; sigmoid(-2.0) = 0.12 > 0.1
        logits.append(lg)
    return logits, np.concatenate(boxes, axis=1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        logits, boxes = make_inputs(fm=32, pass_per_class=100)
        passing = [int((1 / (1 + np.exp(-lg[0, :, 0])) >= SCORE_THRESH).sum()) for lg in logits]
        print("rehearsal: boxes", boxes.shape, "logits", [lg.shape for lg in logits], "passing in scene 0, first class of each head", passing)
        return
    from seevcn_amd.pcdet.models.model_utils import model_nms_utils
    assert torch.cuda.is_available(), "multihead_post_micro needs a GPU"
    dev = torch.device("cuda:0")
    logits_np, boxes_np = make_inputs()
    logits = [torch.from_numpy(x).to(dev) for x in logits_np]
    boxes = torch.from_numpy(boxes_np).to(dev)
    labels, at = [], 1
    for classes in HEADS:
        labels.append(torch.arange(at, at + classes, device=dev))
        at += classes
    passing = torch.stack([(torch.sigmoid(lg) >= SCORE_THRESH).sum(1).float().mean(0) for lg in logits if lg.shape[2] == 2]).mean().item()

    def batched():
        return model_nms_utils.multi_classes_nms_batch(logits, boxes, labels, NMS, score_thresh=SCORE_THRESH, normalized=False)

    def loop():
        out = []
        for b in range(SCENES):
            start, sc, lb, bx = 0, [], [], []
            for lg, mapping in zip(logits, labels):
                s, l, x = model_nms_utils.multi_classes_nms(torch.sigmoid(lg[b]), boxes[b, start:start + lg.shape[1]], NMS, SCORE_THRESH)
                sc.append(s), lb.append(mapping[l]), bx.append(x)
                start += lg.shape[1]
            out.append({'pred_boxes': torch.cat(bx), 'pred_scores': torch.cat(sc), 'pred_labels': torch.cat(lb)})
        return out

    lines = [f"class-wise post-processing at cbgs_second_multihead.yaml sizes: {SCENES} scenes, map {FM} x {FM}, {sum(HEADS)} classes in {len(HEADS)} heads, "
             f"{boxes.shape[1]} anchors a scene, threshold {SCORE_THRESH}, pre {NMS['NMS_PRE_MAXSIZE']}, post {NMS['NMS_POST_MAXSIZE']}, "
             f"NMS threshold {NMS['NMS_THRESH']}; {passing:.0f} boxes of a class pass the threshold on average"]
    got, want = batched(), loop()
    kept = [len(d['pred_labels']) for d in want]
    same = all(torch.equal(g[k], w[k]) for g, w in zip(got, want) for k in ('pred_boxes', 'pred_scores', 'pred_labels'))
    lines.append(f"survivors per scene {kept}; batched path == per-class loop element for element: {same}")
    print("\n".join(lines), flush=True)
    for name, fn in (("batched (sv_nms_segments)", batched), ("per-class loop (nms_gpu)", loop)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, a.windows, a.calls)
        launches, kernel_ms = kernels_of_one_call(fn)
        k = "profiler: not measured" if launches is None else f"{launches} launches, kernel time {kernel_ms:.3f} ms"
        lines.append(f"{name:<28s} median {ms[len(ms) // 2]:8.3f} ms   min {ms[0]:8.3f}   max {ms[-1]:8.3f}   ({len(ms)} x {a.calls} calls)   {k}, "
                     f"{host_reads(fn)} host reads")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not same:
        raise SystemExit("the two paths differ")


if __name__ == "__main__":
    main()
