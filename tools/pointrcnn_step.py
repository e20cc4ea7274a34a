"""One PointRCNN train step and one eval forward at pointrcnn.yaml sizes (2 scenes x 16 384 points, the full model of model_cfgs.pointrcnn_model_cfg),
with the device time split per module: forward hooks record events in front of and behind every entry of the detector's module_list and every
set-abstraction / feature-propagation module under it; the backward pass is one span.  Median over the timed steps behind a warm-up.  The record
is there to show where the time goes (the SA MLPs run as torch Conv2d + BatchNorm2d on MIOpen), not to meet a target.  Needs a GPU (--rehearse:
build the inputs and the model on the CPU, print the module list, stop).  --ordered: the same steps with seevcn_amd.set_ordered_gradients(True),
i.e. the grouping and interpolation gradients of every SA / FP module on the order-fixed entries; the calls they took are printed.

    python tools/pointrcnn_step.py [--out profiles/pointrcnn_step.txt] [--steps 5] [--warmup 2] [--ordered]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seevcn_amd.pcdet import model_cfgs as C  # noqa: E402
from seevcn_amd.seeding import seeded_state_dict  # noqa: E402

SCENES, POINTS = 2, 16384


def make_inputs():
    """A synthetic scene batch resampled to exactly POINTS points a scene (with repetition where a scene has fewer), an intensity column added."""
    import seevcn_amd.synth as synth
    rng = np.random.default_rng(9)
    pts, gt = synth.make_scene_batch(SCENES, seed=2000, n_az=900)
    rows = []
    for b in range(SCENES):
        p = pts[pts[:, 0] == b]
        rows.append(p[rng.choice(len(p), POINTS, replace=len(p) < POINTS)])
    pts = np.concatenate(rows)
    return np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1)).astype(np.float32)], 1).astype(np.float32), gt.astype(np.float32)


class Spans:
    """Device events around named modules."""

    def __init__(self):
        self.open, self.done = {}, []

    def watch(self, name, module):
        def pre(_m, _inp):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.open[name] = e

        def post(_m, _inp, _out):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.done.append((name, self.open.pop(name), e))
        module.register_forward_pre_hook(pre)
        module.register_forward_hook(post)

    def span(self, name):
        spans = self

        class _Ctx:
            def __enter__(self):
                self.a = torch.cuda.Event(enable_timing=True)
                self.a.record()

            def __exit__(self, *exc):
                b = torch.cuda.Event(enable_timing=True)
                b.record()
                spans.done.append((name, self.a, b))
                return False
        return _Ctx()

    def take(self):
        torch.cuda.synchronize()
        out = [(n, a.elapsed_time(b)) for n, a, b in self.done]
        self.done = []
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--ordered", action="store_true", help="take the order-fixed gradient route (set_ordered_gradients(True))")
    a = ap.parse_args()
    import seevcn_amd
    seevcn_amd.set_ordered_gradients(a.ordered)
    from seevcn_amd.pcdet.models import detectors
    pts, gt = make_inputs()
    net = detectors.build_detector(C.pointrcnn_model_cfg(), num_class=3, dataset=C.SyntheticDatasetInfo(num_point_features=4))
    net.load_state_dict(seeded_state_dict(net, seed=6))
    lines = [f"PointRCNN (pointrcnn.yaml), {SCENES} scenes x {POINTS} points, {sum(p.numel() for p in net.parameters())} parameters; "
             f"modules {[type(m).__name__ for m in net.module_list]}; gradients: {'order-fixed (--ordered)' if a.ordered else 'default (float atomics)'}"]
    if a.rehearse or not torch.cuda.is_available():
        print("\n".join(lines))
        if not a.rehearse:
            raise SystemExit("pointrcnn_step: no GPU visible; timings are not produced anywhere else")
        return
    dev = torch.device("cuda:0")
    net = net.to(dev)
    spans = Spans()
    for top in ("backbone_3d", "point_head", "roi_head"):
        mod = getattr(net, top)
        spans.watch(top, mod)
        for group in ("SA_modules", "FP_modules"):
            for k, sub in enumerate(getattr(mod, group, [])):
                spans.watch(f"{top}.{group}.{k}", sub)
    pool = net.roi_head.roipoint_pool3d_layer
    spans.watch("roi_head.roipoint_pool3d_layer", pool)
    batch = {"batch_size": SCENES, "points": torch.from_numpy(pts).to(dev), "gt_boxes": torch.from_numpy(gt).to(dev), "points_per_scene": [POINTS] * SCENES}
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    results = {"train": [], "eval": []}
    np.random.seed(0)
    torch.manual_seed(0)
    for mode in ("train", "eval"):
        net.train(mode == "train")
        for step in range(a.warmup + a.steps):
            with spans.span("whole step"):
                if mode == "train":
                    opt.zero_grad(set_to_none=True)
                    ret, tb, _ = net(dict(batch))
                    with spans.span("backward"):
                        ret["loss"].backward()
                    with spans.span("optimizer"):
                        opt.step()
                else:
                    with torch.no_grad(), spans.span("forward + post_processing"):
                        net(dict(batch))
            got = spans.take()
            if step >= a.warmup:
                results[mode].append(got)
        if mode == "train":
            lines.append("train step losses: " + ", ".join(f"{k} {float(v):.4f}" for k, v in tb.items()))
            calls = {k: v for k, v in seevcn_amd.ordered_gradient_calls().items() if v}
            lines.append(f"order-fixed gradient calls over the {a.warmup + a.steps} train steps: {calls if calls else 'none'}")
    for mode, runs in results.items():
        lines.append(f"--- {mode}: median of {len(runs)} steps behind {a.warmup} warm-up steps (ms: median, min .. max)")
        names = []
        for n, _ in runs[0]:
            if n not in names:
                names.append(n)
        order = sorted(names, key=lambda n: (n != "whole step", n))
        for n in order:
            per_step = sorted(sum(ms for m, ms in run if m == n) for run in runs)
            lines.append(f"{n:<40s} {per_step[len(per_step) // 2]:9.3f}   {per_step[0]:9.3f} .. {per_step[-1]:9.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
