"""CPU: the restated optimizer step and schedules (tests/optim_reference.py, seevcn_amd.tools.train_utils.optimization) against what the
reference's own build_optimizer / build_scheduler / clip_grad_norm_ recorded in tests/golden/optim.npz."""
import os

import numpy as np
import pytest
import torch

import optim_reference as OR
from oracle.tolerances import assert_close_per_channel
from seevcn_amd.tools.train_utils import optimization as O

PCDET = [c for c, v in OR.CASES.items() if v["kind"] == "pcdet"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "optim.npz"))


def case_data(name):
    ci = list(OR.CASES).index(name)
    model = OR.make_model()
    init, grads = OR.seeded_arrays(model, seed=100 + ci)
    return model, init, grads


def hyper(name, golden, k):
    """(lr, b1, b2, eps, wd, mode, max_norm) of step k as the reference ran it."""
    case = OR.CASES[name]
    lr, b1 = float(golden[f"{name}/lr"][k, 0]), float(golden[f"{name}/mom"][k, 0])
    if case["kind"] == "vcn":
        return lr, b1, 0.999, 1e-8, 0.0, OR.NO_DECAY, None
    cfg = case["cfg"]
    if cfg.OPTIMIZER == "adam_onecycle":
        return lr, b1, 0.99, 1e-8, cfg.WEIGHT_DECAY, OR.DECOUPLED, cfg.GRAD_NORM_CLIP
    return lr, b1, 0.999, 1e-8, cfg.WEIGHT_DECAY, OR.L2, cfg.GRAD_NORM_CLIP


class _Knobs:
    lr = mom = None


@pytest.mark.parametrize("name", ["onecycle7", "onecycle10"])
def test_one_cycle_equals_reference(golden, name):
    """int(total_step * 0.4) truncates for 7 (2.8) and not for 10; steps 2 and 4 sit exactly on the phase boundary."""
    case = OR.CASES[name]
    cfg, total = case["cfg"], case["iters"] * case["epochs"]
    knobs = _Knobs()
    sched, warm = O.build_scheduler(knobs, case["iters"], case["epochs"], -1, cfg)
    assert isinstance(sched, O.OneCycle) and warm is None
    assert int(total * cfg.PCT_START) in range(OR.K)
    for k in range(OR.K):
        sched.step(k)
        assert knobs.lr == golden[f"{name}/lr"][k, 0] and knobs.mom == golden[f"{name}/mom"][k, 0], (k, knobs.lr, knobs.mom)
        lr, mom = OR.one_cycle(k, total, cfg.LR, cfg.MOMS, cfg.DIV_FACTOR, cfg.PCT_START)
        assert lr == golden[f"{name}/lr"][k, 0] and mom == golden[f"{name}/mom"][k, 0]
    assert (golden[f"{name}/lr"] == golden[f"{name}/lr"][:, :1]).all() and golden[f"{name}/lr"].shape[1] == 2


def test_annealing_cos_ends():
    assert O.annealing_cos(0.95, 0.85, 0.0) == OR.annealing_cos(0.95, 0.85, 0.0) == 0.95
    assert O.annealing_cos(0.95, 0.85, 1.0) == OR.annealing_cos(0.95, 0.85, 1.0)
    assert O.annealing_cos(3e-4, 3e-3, 0.5) == OR.annealing_cos(3e-4, 3e-3, 0.5)


def test_step_decay_lambda_equals_reference(golden):
    case = OR.CASES["adam_l2"]
    cfg = case["cfg"]
    w = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([w], lr=cfg.LR)
    sched, warm = O.build_scheduler(opt, case["iters"], case["epochs"], -1, cfg)
    assert warm is None
    steps = [s * case["iters"] for s in cfg.DECAY_STEP_LIST]
    for k in range(OR.K):
        assert opt.param_groups[0]["lr"] == golden["adam_l2/lr"][k, 0]
        assert cfg.LR * OR.step_decay_lambda(k, steps, cfg.LR_DECAY, cfg.LR_CLIP, cfg.LR) == golden["adam_l2/lr"][k, 0]
        opt.step()
        sched.step()


def test_warmup_branch_runs():
    """The reference's LR_WARMUP branch takes len() of an int; ours uses the int."""
    cfg = OR.Cfg(OR.CASES["adam_l2"]["cfg"], LR_WARMUP=True, WARMUP_EPOCH=2)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=cfg.LR)
    _, warm = O.build_scheduler(opt, 5, 3, -1, cfg)
    assert isinstance(warm, O.CosineWarmupLR) and warm.T_max == 10 and warm.eta_min == cfg.LR / cfg.DIV_FACTOR


def test_mixed_optim_is_not_built():
    with pytest.raises(NotImplementedError, match="FastAIMixedOptim"):
        O.FastAIMixedOptim.create(None, 1e-3, [])


def run32(name, golden, grads, init, steps):
    """The fp32 restatement for `steps` steps with the reference's lr / mom; returns per step (params, m, v, total_norm)."""
    p = [a.copy() for a in init]
    m = [np.zeros_like(a) for a in init]
    v = [np.zeros_like(a) for a in init]
    hist = []
    for k in range(steps):
        lr, b1, b2, eps, wd, mode, max_norm = hyper(name, golden, k)
        norm = np.float32(OR.total_norm64(grads[k]))
        clip = OR.clip32(norm, max_norm)
        for i in range(len(p)):
            p[i], m[i], v[i] = OR.adam_step32(p[i], grads[k][i], m[i], v[i], k + 1, lr, b1, b2, eps, wd, mode, clip)
        hist.append(([a.copy() for a in p], [a.copy() for a in m], [a.copy() for a in v], norm))
    return hist


@pytest.mark.parametrize("name", ["onecycle7", "adam_l2", "adamw0"])
def test_fp32_restatement_follows_reference_trajectory(golden, name):
    model, init, grads = case_data(name)
    hist = run32(name, golden, grads, init, OR.K)
    for k in range(OR.K):
        for i in range(len(init)):
            assert_close_per_channel(hist[k][0][i], golden[f"{name}/p{k + 1}/{i}"], rtol=1e-3, atol_frac=1e-4, name=f"{name} step {k + 1} param {i}")
        if hyper(name, golden, k)[6]:
            ref = float(golden[f"{name}/total_norm"][k])
            # the reference sums n squares in fp32 in an order of torch's choosing: relative error <= (n + 2) u on the sum whatever the order,
            # half of that after the square root, plus the roundings of the root and of ours
            n = sum(a.size for a in grads[k])
            assert abs(float(hist[k][3]) - ref) <= ((n + 2) / 2 + 2) * OR.U * ref


def single_steps(name, golden):
    """(k, p, m, v, t) of the two single steps taken from the reference's own states: the seeded start, and its state_dict after step 3."""
    model, init, grads = case_data(name)
    n = len(init)
    zeros = [np.zeros_like(a) for a in init]
    yield 0, init, zeros, zeros, 1, grads[0]
    p3 = [golden[f"{name}/p3/{i}"] for i in range(n)]
    idx = OR.optimizer_index(model, split=OR.CASES[name]["kind"] == "pcdet" and OR.CASES[name]["cfg"].OPTIMIZER == "adam_onecycle")
    m3 = [golden[f"{name}/sd3/state/{idx[i]}/exp_avg"] for i in range(n)]
    v3 = [golden[f"{name}/sd3/state/{idx[i]}/exp_avg_sq"] for i in range(n)]
    assert all(float(golden[f"{name}/sd3/state/{i}/step"]) == 3.0 for i in range(n))
    yield 3, p3, m3, v3, 4, grads[3]


@pytest.mark.parametrize("name", ["onecycle7", "adam_l2", "adamw0"])
def test_single_steps_within_allowance(golden, name):
    """From the same state: the fp32 restatement and the reference's own fp32 result, each against the float64 step, within the derived allowance."""
    for k, p, m, v, t, g in single_steps(name, golden):
        lr, b1, b2, eps, wd, mode, max_norm = hyper(name, golden, k)
        exact = OR.total_norm64(g)
        norm32 = np.float32(exact)
        assert abs(float(norm32) - exact) <= OR.total_norm_bound(exact, sum(a.size for a in g))
        recorded = float(golden[f"{name}/total_norm"][k])
        for i in range(len(p)):
            want, _, _, allow = OR.adam_step64(p[i], g[i], m[i], v[i], t, lr, b1, b2, eps, wd, mode, OR.clip64(exact, max_norm), with_allowance=True)
            ours = OR.adam_step32(p[i], g[i], m[i], v[i], t, lr, b1, b2, eps, wd, mode, OR.clip32(norm32, max_norm))[0]
            err = np.abs(ours.astype(np.float64) - want)
            assert (err <= allow).all(), (name, k, i, float((err / allow).max()))
            # the reference clipped with its own fp32-summed norm: the float64 step takes that norm, so that the element arithmetic is what is held
            want_r, _, _, allow_r = OR.adam_step64(p[i], g[i], m[i], v[i], t, lr, b1, b2, eps, wd, mode, OR.clip64(recorded, max_norm), with_allowance=True)
            err_r = np.abs(golden[f"{name}/p{k + 1}/{i}"].astype(np.float64) - want_r)
            assert (err_r <= allow_r).all(), (name, k, i, float((err_r / allow_r).max()))
            # and the allowance is tight enough to notice a wrong operation: an Adam update moves an element by about lr, so an error of 2 % of
            # one update (beyond the result's own rounding) must not fit inside it -- for the typical element: where grad * clip and wd * p
            # cancel, the first step's g / |g| is ill-conditioned and the allowance rightly grows
            assert np.median(allow) <= 0.02 * lr + 4 * OR.U * np.median(np.abs(want)), (name, k, i, float(np.median(allow)), lr)


@pytest.mark.parametrize("name", PCDET + ["adamw0"])
def test_state_dict_layout(golden, name):
    """The reference's group split from our own split_bn_bias: even groups the non-BatchNorm leaves, odd groups BatchNorm; per-index state arrays of
    the fp32 restatement after 3 steps against the recorded exp_avg / exp_avg_sq."""
    model, init, grads = case_data(name)
    params = list(model.parameters())
    ngroups = len(golden[f"{name}/weight_decay3"])
    if OR.CASES[name]["kind"] == "pcdet" and OR.CASES[name]["cfg"].OPTIMIZER == "adam_onecycle":
        from seevcn_amd.tools.train_utils.optimization import _leaves
        split = O.split_bn_bias([torch.nn.Sequential(*_leaves(model))])
        assert len(split) == ngroups == 2
        order = [p for g in split for p in g.parameters()]
        assert all(isinstance(c, O.fastai_optim.bn_types) for c in split[1].children()) and len(list(split[1].children())) == 3
        assert not any(isinstance(c, O.fastai_optim.bn_types) for c in split[0].children())
        sizes = [len(list(g.parameters())) for g in split]
        layout = OR.group_layout(model)
        assert [layout[[id(q) for q in params].index(id(p))] for p in order] == [(g, j) for g in range(2) for j in range(sizes[g])]
        assert (golden[f"{name}/weight_decay3"] == 0).all()          # true_wd leaves 0 in the groups
    else:
        order, sizes = params, [len(params)]
        assert ngroups == 1
    start = 0
    for gi, n in enumerate(sizes):
        assert golden[f"{name}/sd3/group/{gi}"].tolist() == list(range(start, start + n))
        start += n
    hist = run32(name, golden, grads, init, 3)
    where = {id(p): i for i, p in enumerate(params)}
    for idx, p in enumerate(order):
        i = where[id(p)]
        assert golden[f"{name}/sd3/state/{idx}/exp_avg"].shape == tuple(p.shape)
        assert_close_per_channel(hist[2][1][i], golden[f"{name}/sd3/state/{idx}/exp_avg"], rtol=1e-3, atol_frac=1e-4, name=f"{name} exp_avg {idx}")
        assert_close_per_channel(hist[2][2][i], golden[f"{name}/sd3/state/{idx}/exp_avg_sq"], rtol=1e-3, atol_frac=1e-4, name=f"{name} exp_avg_sq {idx}")
