"""Optimizer-step microbenchmark on the parameter list of the SECOND model of bench_configs (seeded values, static gradients).

Three routes, each timed over --steps steps after --warmup (GPU time by events around the whole loop, host time = wall time of enqueueing it):
  (a) fused      OptimWrapper over seevcn_amd.optim.FusedAdam as build_optimizer makes it (clip + true_wd + Adam in <= 3 launches)
  (b) reference  the reference's route in plain torch: clip_grad_norm_, one p.data.mul_(1 - wd*lr) per parameter, torch.optim.Adam
  (c) torch      clip_grad_norm_ + torch.optim.AdamW(fused=True)
and the fused kernels' share of the attainable HBM rate (MI355X: 6.29 TB/s measured float4 copy), taken on 16 copies of the list so that the GPU and
not the host bounds the loop: the norm reads 4 bytes an element, the update reads 16 and writes 12.  Writes profiles/optim_step.txt (or --out).

    python tools/optim_micro.py --steps 200 --warmup 20 --runs 3
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ATTAINABLE = 6.29e12
COPIES = 16


class Counting:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    host = (time.perf_counter() - t0) / steps
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / steps, host


def launches(step):
    """Kernels of one step as the profiler sees them; None where this build's profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.txt"))
    args = ap.parse_args()
    import seevcn_amd  # noqa: F401
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.seeding import seeded_state_dict
    from seevcn_amd.tools.train_utils import optimization as O
    dev = torch.device("cuda:0")
    cfg = dict(OPTIMIZER="adam_onecycle", LR=0.003, WEIGHT_DECAY=0.01, MOMS=[0.95, 0.85], PCT_START=0.4, DIV_FACTOR=10, DECAY_STEP_LIST=[35, 45],
               LR_DECAY=0.1, LR_CLIP=1e-7, LR_WARMUP=False, GRAD_NORM_CLIP=10)

    def model():
        net = detectors.build_detector(C.second_model_cfg(dynamic_vfe=True), num_class=3, dataset=C.SyntheticDatasetInfo())
        net.load_state_dict(seeded_state_dict(net, seed=5))
        net = net.to(dev)
        g = torch.Generator(device=dev).manual_seed(1)
        for p in net.parameters():
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 0.1
        return net

    lr, mom, wd, clip = 3e-4, 0.95, 0.01, 10.0
    rows = []
    # (a)
    net = model()
    n_elem = sum(p.numel() for p in net.parameters())
    n_tens = len(list(net.parameters()))
    opt = O.build_optimizer(net, cfg)
    O.build_scheduler(opt, 100, 1, -1, cfg)[0].step(0)
    calls = Counting(opt.opt._lib)
    for name in ("sv_optim_grad_sqnorm", "sv_optim_adam_step"):                    # on the library object: the step reaches it through _lib.launch
        setattr(opt.opt._lib, name, getattr(calls, name))
    opt.step()
    del calls.calls[:]
    opt.step()
    per_step = list(calls.calls)
    fused = [timed(opt.step, args.steps, args.warmup) for _ in range(args.runs)]
    rows.append(("(a) fused", fused, len(per_step), launches(opt.step), "sv_optim_grad_sqnorm (1 launch) + sv_optim_adam_step (2 launches)"))
    # the kernels' share of the memory rate: the steps above are as long on the host as on the GPU, so the rate is taken on COPIES copies of the same
    # shapes (a working set far beyond the 256 MB MALL, GPU time well above the host's), with and without the norm launch
    from seevcn_amd.optim import FusedAdam
    big = [torch.nn.Parameter(p.detach().clone()) for _ in range(COPIES) for p in net.parameters()]
    for p in big:
        p.grad = torch.full_like(p, 0.01)
    big_opt = FusedAdam(big, lr=lr, betas=(mom, 0.99), weight_decay=wd, decoupled_weight_decay=True, max_grad_norm=clip)
    whole = [timed(big_opt.step, 50, 5) for _ in range(args.runs)]
    big_opt.max_grad_norm = None
    upd = [timed(big_opt.step, 50, 5) for _ in range(args.runs)]
    del big, big_opt
    # (b)
    net = model()
    params = [p for p in net.parameters()]
    adam = torch.optim.Adam(params, lr=lr, betas=(mom, 0.99))

    def ref_step():
        torch.nn.utils.clip_grad_norm_(params, clip)
        for p in params:
            p.data.mul_(1 - wd * lr)
        adam.step()
    rows.append(("(b) reference route, plain torch", [timed(ref_step, args.steps, args.warmup) for _ in range(args.runs)], None, launches(ref_step),
                 "clip_grad_norm_, one mul_ per parameter, torch.optim.Adam (torch's default implementation on this device)"))
    # (c)
    net = model()
    params_c = [p for p in net.parameters()]
    adamw = torch.optim.AdamW(params_c, lr=lr, betas=(mom, 0.99), weight_decay=wd, fused=True)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(params_c, clip)
        adamw.step()
    rows.append(("(c) clip_grad_norm_ + AdamW(fused=True)", [timed(torch_step, args.steps, args.warmup) for _ in range(args.runs)], None,
                 launches(torch_step), ""))

    lines = [f"Optimizer step on the SECOND model's parameter list: {n_tens} tensors, {n_elem} fp32 elements ({n_elem * 4 / 1e6:.1f} MB), static gradients.",
             f"{args.runs} runs of {args.steps} steps after {args.warmup} warm-up steps, one process on one MI355X ({torch.cuda.get_device_name(0)}), "
             f"torch {torch.__version__}.",
             "GPU time: events around the loop / steps.  Host time: wall time of enqueueing the loop / steps.  Best and worst run.", ""]
    for name, runs, ncalls, nlaunch, note in rows:
        gpu, host = [r[0] for r in runs], [r[1] for r in runs]
        lines.append(f"{name:42s} GPU {min(gpu) * 1e6:8.1f} .. {max(gpu) * 1e6:8.1f} us   host {min(host) * 1e6:8.1f} .. {max(host) * 1e6:8.1f} us   "
                     f"library calls {ncalls if ncalls is not None else '-':>3}   launches {nlaunch if nlaunch is not None else 'n/a':>4}   {note}")
    lines.append("")
    n_big = COPIES * n_elem
    for name, runs, nbytes in (("update alone (max_grad_norm=None: finalize + update launches)", upd, 28), ("whole step (norm + finalize + update)", whole, 32)):
        gpu, host = min(r[0] for r in runs), min(r[1] for r in runs)
        lines.append(f"rate, {COPIES} copies of the list ({n_big} elements, {16 * n_big / 1e6:.0f} MB of parameter, gradient and moments), {name}: "
                     f"GPU {gpu * 1e6:.1f} .. {max(r[0] for r in runs) * 1e6:.1f} us (host {host * 1e6:.1f} us) = {nbytes * n_big / gpu / 1e12:.2f} TB/s of "
                     f"{nbytes} bytes an element = {nbytes * n_big / gpu / HBM_ATTAINABLE * 100:.0f} % of the attainable {HBM_ATTAINABLE / 1e12:.2f} TB/s")
    lines += ["", f"library calls of a fused step: {per_step}"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
