"""The schedules of detector3d/tools/train_utils/optimization/learning_schedules_fastai.py: plain host float64, the lr and mom they set equal the
reference's bit for bit (tests/test_optim_reference.py holds them to the recorded sequences with ==)."""
import math
from functools import partial

import numpy as np
import torch.optim.lr_scheduler as lr_sched


def _phases(total_step, phases):
    """((start fraction, f), ...) -> [(first step, end step, f)]; a phase ends where the next begins, the last at total_step; int() truncates."""
    out = []
    for i, (start, fn) in enumerate(phases):
        assert not out or phases[i - 1][0] < start
        if isinstance(fn, str):
            fn = eval(fn)
        end = int(phases[i + 1][0] * total_step) if i + 1 < len(phases) else total_step
        out.append((int(start * total_step), end, fn))
    assert out[0][0] == 0
    return out


class LRSchedulerStep:
    """Piecewise schedules of lr and mom over [0, total_step); step(k) applies every phase that has begun, in order, so the last one begun wins."""

    def __init__(self, fai_optimizer, total_step, lr_phases, mom_phases):
        self.optimizer = fai_optimizer
        self.total_step = total_step
        self.lr_phases = _phases(total_step, lr_phases)
        self.mom_phases = _phases(total_step, mom_phases)

    def step(self, step):
        for start, end, fn in self.lr_phases:
            if step >= start:
                self.optimizer.lr = fn((step - start) / (end - start))
        for start, end, fn in self.mom_phases:
            if step >= start:
                self.optimizer.mom = fn((step - start) / (end - start))


def annealing_cos(start, end, pct):
    """Cosine from start (pct 0) to end (pct 1); numpy's cos, in this order of operations."""
    cos_out = np.cos(np.pi * pct) + 1
    return end + (start - end) / 2 * cos_out


class OneCycle(LRSchedulerStep):
    """lr: lr_max / div_factor up to lr_max over the first pct_start of the steps, then down to lr_max / div_factor / 1e4; mom: moms[0] down to
    moms[1] and back."""

    def __init__(self, fai_optimizer, total_step, lr_max, moms, div_factor, pct_start):
        self.lr_max, self.moms, self.div_factor, self.pct_start = lr_max, moms, div_factor, pct_start
        low_lr = lr_max / div_factor
        lr_phases = ((0, partial(annealing_cos, low_lr, lr_max)), (pct_start, partial(annealing_cos, lr_max, low_lr / 1e4)))
        mom_phases = ((0, partial(annealing_cos, *moms)), (pct_start, partial(annealing_cos, *moms[::-1])))
        fai_optimizer.lr, fai_optimizer.mom = low_lr, moms[0]
        super().__init__(fai_optimizer, total_step, lr_phases, mom_phases)


class CosineWarmupLR(lr_sched._LRScheduler):
    def __init__(self, optimizer, T_max, eta_min=0, last_epoch=-1):
        self.T_max = T_max
        self.eta_min = eta_min
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return [self.eta_min + (base_lr - self.eta_min) * (1 - math.cos(math.pi * self.last_epoch / self.T_max)) / 2 for base_lr in self.base_lrs]
