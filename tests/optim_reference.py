"""The optimizer step of include/seevcn_hip.h ("optimizer step") restated in numpy, in float64 and in fp32 in the header's order; the per-element
allowance between the two; the bound on total_norm; the seeded cases shared by tests/golden/make_optim_golden.py and the tests.

Allowance (u = 2^-24, the unit roundoff of fp32; every fp32 operation, and every float64 scalar rounded to fp32, contributes at most u relative).
All quantities on the right are the float64 restatement's own intermediates, so the allowance is an array computed once per case:
  clip   = max_norm / (total_norm + 1e-6), clamped: the sum, the quotient, max_norm rounded, and the norm's own rounding      e_c = 4u
  g      = grad * clip [+ wd * p]: |dg| <= 6u G,  G = |grad * clip| + |wd * p|   (clip 4u, product u; wd rounded u, product u; the sum u)
  p'     = p * decay: |dp'| <= 2u |p|                                              (decay rounded, the product)
  m      = b1 m + omb1 g: |dm| <= 9u M,  M = |b1 m| + (1 - b1) G                   (two roundings of a scalar, two products, the sum: 3u M; and
                                                                                    (1 - b1) |dg| <= 6u M.  torch's lerp form m + w (g - m) costs
                                                                                    3u w (|g| + |m|) + u |m| <= 4u M for b1 >= 1/2)
  v      = b2 v + (omb2 g) g: |dv| <= 16u V,  V = b2 v + (1 - b2) G^2              (3u on each term and the sum; d(g^2) <= 2 G |dg| = 12u G^2)
  s      = sqrt(v): |ds| <= min(|dv| / (2 s), sqrt(|dv|)) + u s
  D      = s / rbc2 + eps: |dD| <= |ds| / rbc2 + 4u D                              (rbc2 rounded, the quotient, eps rounded, the sum)
  q      = (step m) / D: |dq| <= (step / D) (|dm| + |m| (4u + |dD| / D))           (step rounded u, beta^t from another pow u, product, quotient)
  p      = p' - q: |dp| <= |dp'| + |dq| + u |p|                                    (half an ulp of the result)
The allowance is SAFETY = 2 times that sum: first-order terms only were kept.

total_norm: the squares are exact in float64, their sum of n terms in the header's order has relative error <= n 2^-53, the square root halves it and
adds 2^-53, the rounding to fp32 adds u:  |total_norm - exact| <= exact (u + n 2^-53).
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
NO_DECAY, L2, DECOUPLED = 0, 1, 2
F = np.float32


def total_norm64(grads):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads)))


def total_norm_bound(exact, n):
    return exact * (U + n * 2.0 ** -53) + 1e-45


def clip64(total_norm, max_norm):
    if max_norm is None or max_norm <= 0:
        return 1.0
    c = max_norm / (total_norm + 1e-6)
    return 1.0 if c > 1.0 else c


def clip32(total_norm, max_norm):
    """From the fp32 total_norm, in fp32: the finalize launch's arithmetic (and clip_grad_norm_'s)."""
    if max_norm is None or max_norm <= 0:
        return F(1.0)
    with np.errstate(all="ignore"):
        c = F(max_norm) / (F(total_norm) + F(1e-6))
    return F(1.0) if c > F(1.0) else c


def adam_step64(p, g, m, v, t, lr, b1, b2, eps, wd, mode, clip, with_allowance=False):
    """One step in float64 from fp32 inputs; t is the step count AFTER this step.  Returns (p, m, v) and, when asked, the allowance on p."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step, rbc2 = lr / bc1, np.sqrt(bc2)
    gc = g * clip
    G = np.abs(gc)
    if mode == L2:
        G = G + np.abs(wd * p)
        gc = gc + wd * p
    p1 = p * (1.0 - lr * wd) if mode == DECOUPLED else p
    m1 = b1 * m + (1.0 - b1) * gc
    v1 = b2 * v + ((1.0 - b2) * gc) * gc
    s = np.sqrt(v1)
    D = s / rbc2 + eps
    q = (step * m1) / D
    pn = p1 - q
    if not with_allowance:
        return pn, m1, v1
    dp1 = 2 * U * np.abs(p) if mode == DECOUPLED else 0.0
    dm = 9 * U * (np.abs(b1 * m) + (1.0 - b1) * G)
    dv = 16 * U * (b2 * v + (1.0 - b2) * G * G)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(s > 0, np.minimum(dv / (2 * np.where(s > 0, s, 1.0)), np.sqrt(dv)), np.sqrt(dv)) + U * s
    dD = ds / rbc2 + 4 * U * D
    dq = (step / D) * (dm + np.abs(m1) * (4 * U + dD / D))
    allow = SAFETY * (dp1 + dq + U * np.abs(pn))
    if with_allowance == "all":                                     # also the allowances on exp_avg and exp_avg_sq
        return pn, m1, v1, allow, SAFETY * dm, SAFETY * dv
    return pn, m1, v1, allow


def adam_step32(p, g, m, v, t, lr, b1, b2, eps, wd, mode, clip):
    """The same step in fp32 in the header's order, every operation rounded once.  clip is the fp32 coefficient."""
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step, rbc2 = F(lr / bc1), F(np.sqrt(bc2))
    fb1, omb1, fb2, omb2, feps, fwd, decay = F(b1), F(1.0 - b1), F(b2), F(1.0 - b2), F(eps), F(wd), F(1.0 - lr * wd)
    with np.errstate(all="ignore"):
        gc = g * F(clip)
        if mode == L2:
            gc = gc + fwd * p
        if mode == DECOUPLED:
            p = p * decay
        m1 = fb1 * m + omb1 * gc
        v1 = fb2 * v + (omb2 * gc) * gc
        D = np.sqrt(v1) / rbc2 + feps
        pn = p - (step * m1) / D
    assert pn.dtype == F and m1.dtype == F and v1.dtype == F
    return pn, m1, v1


# ---- the schedules, restated (host float64; must equal the reference's sequences bit for bit) -----------------------------------------------------
def annealing_cos(start, end, pct):
    cos_out = np.cos(np.pi * pct) + 1
    return end + (start - end) / 2 * cos_out


def one_cycle(step, total_step, lr_max, moms, div_factor, pct_start):
    """(lr, mom) the OneCycle schedule sets at `step`."""
    a1 = int(total_step * pct_start)
    low = lr_max / div_factor
    if step >= a1:
        pct = (step - a1) / (total_step - a1)
        return annealing_cos(lr_max, low / 1e4, pct), annealing_cos(moms[1], moms[0], pct)
    pct = (step - 0) / (a1 - 0)
    return annealing_cos(low, lr_max, pct), annealing_cos(moms[0], moms[1], pct)


def step_decay_lambda(epoch, decay_steps, lr_decay, lr_clip, lr):
    """build_scheduler's LambdaLR factor."""
    f = 1
    for s in decay_steps:
        if epoch >= s:
            f = f * lr_decay
    return max(f, lr_clip / lr)


# ---- the seeded cases --------------------------------------------------------------------------------------------------------------------------
K = 6                                                 # steps per trajectory
GRAD_SCALES = [3.0, 0.1, 1.0, 0.02, 2.0, 0.3]         # gradient norms from far above GRAD_NORM_CLIP to far below it


class Cfg(dict):
    """Attribute access over a dict, as the reference's EasyDict configs give."""
    __getattr__ = dict.__getitem__


CASES = {
    # every detector config: adam_onecycle, true_wd.  total steps 7 = 7 x 1 and 10 = 5 x 2: int(total * 0.4) truncates (2.8 -> 2) or is exact (4)
    "onecycle7": dict(kind="pcdet", iters=7, epochs=1, cfg=Cfg(OPTIMIZER="adam_onecycle", LR=0.003, WEIGHT_DECAY=0.01, MOMENTUM=0.9, MOMS=[0.95, 0.85],
                                                               PCT_START=0.4, DIV_FACTOR=10, DECAY_STEP_LIST=[35, 45], LR_DECAY=0.1, LR_CLIP=1e-7,
                                                               LR_WARMUP=False, WARMUP_EPOCH=1, GRAD_NORM_CLIP=10)),
    "onecycle10": dict(kind="pcdet", iters=5, epochs=2, cfg=Cfg(OPTIMIZER="adam_onecycle", LR=0.003, WEIGHT_DECAY=0.01, MOMENTUM=0.9, MOMS=[0.95, 0.85],
                                                                PCT_START=0.4, DIV_FACTOR=10, DECAY_STEP_LIST=[35, 45], LR_DECAY=0.1, LR_CLIP=1e-7,
                                                                LR_WARMUP=False, WARMUP_EPOCH=1, GRAD_NORM_CLIP=10)),
    # OPTIMIZER: adam, L2 decay, step decay at iterations 2 and 4
    "adam_l2": dict(kind="pcdet", iters=2, epochs=3, cfg=Cfg(OPTIMIZER="adam", LR=0.003, WEIGHT_DECAY=0.01, MOMENTUM=0.9, MOMS=[0.95, 0.85],
                                                             PCT_START=0.4, DIV_FACTOR=10, DECAY_STEP_LIST=[1, 2], LR_DECAY=0.1, LR_CLIP=1e-7,
                                                             LR_WARMUP=False, WARMUP_EPOCH=1, GRAD_NORM_CLIP=10)),
    # the VCN YAML: AdamW, weight_decay 0, LambdaLR, no clipping
    "adamw0": dict(kind="vcn", iters=3, epochs=2, cfg=Cfg(optimizer=Cfg(type="AdamW", kwargs=Cfg(lr=0.0001, weight_decay=0)),
                                                          scheduler=Cfg(type="LambdaLR", kwargs=Cfg(decay_step=2, lr_decay=0.9, lowest_decay=0.02)))),
}


def make_model():
    """A few thousand parameters in 13 tensors: Linear and BatchNorm leaves at two depths, so that the flat layer group has both kinds."""
    import torch.nn as nn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1 = nn.Linear(7, 13)
            self.bn1 = nn.BatchNorm1d(13)
            self.block = nn.Sequential(nn.Linear(13, 33, bias=False), nn.BatchNorm1d(33), nn.ReLU(), nn.Conv1d(33, 33, 3), nn.BatchNorm1d(33))
            self.head = nn.Linear(33, 5)

    return Net()


def seeded_arrays(model, seed):
    """Initial parameters and K gradients per parameter from numpy's generator (the same on every machine), in model.parameters() order."""
    rng = np.random.RandomState(seed)
    shapes = [tuple(p.shape) for p in model.parameters()]
    init = [rng.standard_normal(s).astype(F) * F(0.5) for s in shapes]
    grads = [[(rng.standard_normal(s) * GRAD_SCALES[k]).astype(F) for s in shapes] for k in range(K)]
    return init, grads


def load_params(model, arrays):
    import torch
    with torch.no_grad():
        for p, a in zip(model.parameters(), arrays):
            p.copy_(torch.from_numpy(a).to(p.device))


def set_grads(model, arrays):
    import torch
    for p, a in zip(model.parameters(), arrays):
        p.grad = torch.from_numpy(a.copy()).to(p.device)


def group_layout(model):
    """For model.parameters() order: the index of each parameter inside the reference wrapper's even (non-BatchNorm) / odd (BatchNorm) groups,
    as (group, position) -- the flat layer group of build_optimizer keeps definition order inside each."""
    import torch.nn as nn
    bn = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)
    where, count = {}, [0, 0]
    for mod in model.modules():
        if list(mod.children()):
            continue
        gi = 1 if isinstance(mod, bn) else 0
        for p in mod.parameters():
            where[id(p)] = (gi, count[gi])
            count[gi] += 1
    return [where[id(p)] for p in model.parameters()]


def optimizer_index(model, split):
    """For model.parameters() order: each parameter's index in the optimizer's state_dict -- its own position, or with the wrapper's split the
    non-BatchNorm parameters first and the BatchNorm parameters after them."""
    n = len(list(model.parameters()))
    if not split:
        return list(range(n))
    layout = group_layout(model)
    n_even = sum(1 for g, _ in layout if g == 0)
    return [j + (n_even if g else 0) for g, j in layout]
