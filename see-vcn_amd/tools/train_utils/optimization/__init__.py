"""build_optimizer / build_scheduler for a reference OPTIMIZATION: block (detector3d/tools/train_utils/optimization/__init__.py), over FusedAdam.

    OPTIMIZER: adam_onecycle   WEIGHT_DECAY: 0.01   MOMS: [0.95, 0.85]   GRAD_NORM_CLIP: 10

The reference's train loop clips with clip_grad_norm_ before optimizer.step() (train_utils.py:53); with fuse_grad_clip the clip is part of the fused
step, and that line is redundant (harmless if kept: a second clip's coefficient clamps to 1).
"""
from functools import partial

import torch.nn as nn
import torch.optim as optim
import torch.optim.lr_scheduler as lr_sched

from ....optim import FusedAdam
from .fastai_optim import FastAIMixedOptim, OptimWrapper, listify, split_bn_bias  # noqa: F401
from .learning_schedules_fastai import CosineWarmupLR, LRSchedulerStep, OneCycle, annealing_cos  # noqa: F401


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _leaves(m):
    """The modules without children, in definition order: the reference's one flat layer group (parameters held directly by a module that also
    has children are not in it, there as here)."""
    kids = list(m.children())
    return [m] if not kids else [leaf for k in kids for leaf in _leaves(k)]


def build_optimizer(model, optim_cfg, fuse_grad_clip=True):
    name = _get(optim_cfg, "OPTIMIZER")
    clip = _get(optim_cfg, "GRAD_NORM_CLIP") if fuse_grad_clip else None
    names = {id(p): n for n, p in model.named_parameters()}
    if name == "adam":
        return FusedAdam(model.parameters(), lr=_get(optim_cfg, "LR"), weight_decay=_get(optim_cfg, "WEIGHT_DECAY"), max_grad_norm=clip, names=names)
    if name == "sgd":
        return optim.SGD(model.parameters(), lr=_get(optim_cfg, "LR"), weight_decay=_get(optim_cfg, "WEIGHT_DECAY"),
                         momentum=_get(optim_cfg, "MOMENTUM"))
    if name == "adam_onecycle":
        opt_func = partial(FusedAdam, betas=(0.9, 0.99), max_grad_norm=clip, names=names)
        return OptimWrapper.create(opt_func, 3e-3, [nn.Sequential(*_leaves(model))], wd=_get(optim_cfg, "WEIGHT_DECAY"), true_wd=True, bn_wd=True)
    raise NotImplementedError(f"OPTIMIZER: {name!r} (adam, adam_onecycle and sgd are built)")


def build_scheduler(optimizer, total_iters_each_epoch, total_epochs, last_epoch, optim_cfg):
    decay_steps = [x * total_iters_each_epoch for x in _get(optim_cfg, "DECAY_STEP_LIST")]

    def lr_lbmd(cur_epoch):
        """LR_DECAY once per decay step reached (multiplied up one at a time, as the reference does), floored at LR_CLIP / LR."""
        factor = 1
        for _ in range(sum(1 for s in decay_steps if cur_epoch >= s)):
            factor = factor * _get(optim_cfg, "LR_DECAY")
        return max(factor, _get(optim_cfg, "LR_CLIP") / _get(optim_cfg, "LR"))

    lr_warmup_scheduler = None
    total_steps = total_iters_each_epoch * total_epochs
    if _get(optim_cfg, "OPTIMIZER") == "adam_onecycle":
        lr_scheduler = OneCycle(optimizer, total_steps, _get(optim_cfg, "LR"), list(_get(optim_cfg, "MOMS")), _get(optim_cfg, "DIV_FACTOR"),
                                _get(optim_cfg, "PCT_START"))
    else:
        lr_scheduler = lr_sched.LambdaLR(optimizer, lr_lbmd, last_epoch=last_epoch)
        if _get(optim_cfg, "LR_WARMUP"):
            # the reference takes len() of total_iters_each_epoch here, an int, and cannot run; the count itself is what it means
            lr_warmup_scheduler = CosineWarmupLR(optimizer, T_max=_get(optim_cfg, "WARMUP_EPOCH") * total_iters_each_epoch,
                                                 eta_min=_get(optim_cfg, "LR") / _get(optim_cfg, "DIV_FACTOR"))
    return lr_scheduler, lr_warmup_scheduler
