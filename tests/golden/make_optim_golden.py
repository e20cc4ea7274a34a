"""Generate tests/golden/optim.npz by running the REFERENCE's own build_optimizer / build_scheduler (detector3d/tools/train_utils/optimization) and
torch.nn.utils.clip_grad_norm_ on CPU torch, in its train loop's order (train_utils.py:34-56: scheduler.step(it), zero_grad, gradients, clip, step),
over the seeded cases of tests/optim_reference.py.  The VCN case uses torch.optim.AdamW and the LambdaLR factor of the reference's
build_lambda_sche, as its builder.build_opti_sche does.

Per case <c>: <c>/lr, <c>/mom (K, groups) as set before each step, <c>/total_norm (K) as clip_grad_norm_ returned it (0 where the case does not
clip), <c>/p<k>/<i> parameter i after step k (k = 0: the seeded start), <c>/sd3/... the optimizer's state_dict after step 3 (step, exp_avg,
exp_avg_sq per parameter index; groups as index lists), <c>/weight_decay3 the groups' weight_decay keys then.

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_optim_golden.py
"""
import os
import sys

import numpy as np
import torch
from torch.nn.utils import clip_grad_norm_

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refimport as R  # noqa: E402
import optim_reference as OR  # noqa: E402

sys.path.insert(0, os.path.join(R.REF, "detector3d", "tools"))
from train_utils.optimization import build_optimizer, build_scheduler  # noqa: E402

out = {}
for ci, (name, case) in enumerate(OR.CASES.items()):
    model = OR.make_model()
    init, grads = OR.seeded_arrays(model, seed=100 + ci)
    OR.load_params(model, init)
    cfg = case["cfg"]
    if case["kind"] == "pcdet":
        opt = build_optimizer(model, cfg)
        sched, _ = build_scheduler(opt, total_iters_each_epoch=case["iters"], total_epochs=case["epochs"], last_epoch=-1, optim_cfg=cfg)
        max_norm = cfg.GRAD_NORM_CLIP
    else:
        opt = torch.optim.AdamW(model.parameters(), **cfg.optimizer.kwargs)
        kw = cfg.scheduler.kwargs
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: max(kw.lr_decay ** (e / kw.decay_step), kw.lowest_decay))
        max_norm = None
    for i, a in enumerate(init):
        out[f"{name}/p0/{i}"] = a
    lrs, moms, norms = [], [], []
    for k in range(OR.K):
        if case["kind"] == "pcdet" and cfg.OPTIMIZER == "adam_onecycle":
            sched.step(k)
        opt.zero_grad()
        OR.set_grads(model, grads[k])
        groups = opt.param_groups
        lrs.append([g["lr"] for g in groups])
        moms.append([g["betas"][0] for g in groups])
        norms.append(float(clip_grad_norm_(model.parameters(), max_norm)) if max_norm else 0.0)
        opt.step()
        if not (case["kind"] == "pcdet" and cfg.OPTIMIZER == "adam_onecycle"):
            sched.step()
        for i, p in enumerate(model.parameters()):
            out[f"{name}/p{k + 1}/{i}"] = p.detach().numpy().copy()
        if k == 2:
            sd = opt.state_dict()
            for idx, s in sd["state"].items():
                out[f"{name}/sd3/state/{idx}/step"] = np.float32(float(s["step"]))
                out[f"{name}/sd3/state/{idx}/exp_avg"] = s["exp_avg"].numpy().copy()
                out[f"{name}/sd3/state/{idx}/exp_avg_sq"] = s["exp_avg_sq"].numpy().copy()
            for gi, g in enumerate(sd["param_groups"]):
                out[f"{name}/sd3/group/{gi}"] = np.asarray(g["params"], np.int64)
            out[f"{name}/weight_decay3"] = np.asarray([g["weight_decay"] for g in sd["param_groups"]], np.float64)
    out[f"{name}/lr"] = np.asarray(lrs, np.float64)
    out[f"{name}/mom"] = np.asarray(moms, np.float64)
    out[f"{name}/total_norm"] = np.asarray(norms, np.float32)

path = os.path.join(HERE, "optim.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
