"""GPU: seevcn_amd.optim.FusedAdam (csrc/optim.hip) against the float64 restatement of tests/optim_reference.py within its derived allowance, and
against the reference's recorded trajectories (tests/golden/optim.npz) through build_optimizer / build_scheduler / build_opti_sche."""
import os

import numpy as np
import pytest
import torch

import optim_reference as OR
from oracle.tolerances import assert_close_per_channel

pytestmark = pytest.mark.gpu

MODES = {"decoupled": dict(weight_decay=0.01, decoupled_weight_decay=True), "l2": dict(weight_decay=0.01, decoupled_weight_decay=False),
         "none": dict(weight_decay=0.0, decoupled_weight_decay=False)}
MODE_ID = {"decoupled": OR.DECOUPLED, "l2": OR.L2, "none": OR.NO_DECAY}
LR, BETAS, EPS = 2e-3, (0.9, 0.99), 1e-8


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "optim.npz"))


@pytest.fixture(scope="module")
def lib(hip_lib):
    return hip_lib


def FusedAdam(*a, **k):
    from seevcn_amd.optim import FusedAdam as F
    return F(*a, **k)


def edge_sizes(lib):
    C = lib.sv_optim_chunk_elems()
    return [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 7, 0]


def host(t):
    return t.detach().cpu().numpy().copy()


def snapshot(opt, params):
    """(P, M, V, T) of the optimizer's parameters as numpy; zeros before the first step."""
    opt._ensure_buffers()
    return ([host(p) for p in params], [host(opt.state[p]["exp_avg"]) for p in params], [host(opt.state[p]["exp_avg_sq"]) for p in params],
            [int(opt.state[p]["step"]) for p in params])


def check_step(opt, params, before, grads, wd, mode, max_norm, lr=LR, betas=BETAS, what=""):
    """The device's step from `before` with `grads` (numpy, None = no gradient) against the float64 restatement, element by element."""
    P, M, V, T = before
    present = [i for i, g in enumerate(grads) if g is not None]
    exact = OR.total_norm64([grads[i] for i in present])
    clip = OR.clip64(exact, max_norm)
    if max_norm:
        n = sum(grads[i].size for i in present)
        got = float(opt.last_total_norm)
        assert abs(got - exact) <= OR.total_norm_bound(exact, n), (what, got, exact)
    else:
        assert opt.last_total_norm is None
    Pn, Mn, Vn, Tn = snapshot(opt, params)
    for i in range(len(params)):
        if grads[i] is None:
            assert np.array_equal(Pn[i], P[i]) and np.array_equal(Mn[i], M[i]) and np.array_equal(Vn[i], V[i]) and Tn[i] == T[i], (what, i)
            continue
        assert Tn[i] == T[i] + 1, (what, i, Tn[i], T[i])
        want = OR.adam_step64(P[i], grads[i], M[i], V[i], T[i] + 1, lr, betas[0], betas[1], EPS, wd, mode, clip, with_allowance="all")
        for tag, got, ref, allow in (("p", Pn[i], want[0], want[3]), ("exp_avg", Mn[i], want[1], want[4]), ("exp_avg_sq", Vn[i], want[2], want[5])):
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= allow).all(), (what, tag, i, P[i].shape, float((err / np.maximum(allow, 1e-300)).max()))


def seeded(sizes, seed, scale=1.0):
    rng = np.random.RandomState(seed)
    return [(rng.standard_normal(n) * scale).astype(np.float32) for n in sizes]


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else torch.from_numpy(g.copy()).to(p.device)


# ---- chunk edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_chunk_edges(cuda, lib, mode):
    """1 .. 2C+7 elements and an empty tensor, two steps (the second from non-zero moments); the gradient norm is far above max_norm in step 1
    (clipped) and below it in step 2."""
    sizes = edge_sizes(lib)
    params = [torch.nn.Parameter(torch.from_numpy(a).to(cuda)) for a in seeded(sizes, 1, 0.5)]
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=5.0, **MODES[mode])
    for k, scale in enumerate((1.0, 0.01)):
        grads = seeded(sizes, 10 + k, scale)
        before = snapshot(opt, params)
        set_grads(params, grads)
        opt.step()
        check_step(opt, params, before, grads, MODES[mode]["weight_decay"], MODE_ID[mode], 5.0, what=f"{mode} step {k + 1}")
    assert int(opt.state[params[-1]]["step"]) == 2                  # the empty tensor has a gradient, so it counts its steps


# ---- alignment -----------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 777.0


def views_into(buf, sizes, offset, gap=8):
    """Consecutive views of `sizes` elements into buf, each starting at an element index = offset (mod 4), with untouched gaps between."""
    out, at = [], 0
    for n in sizes:
        at = (at + 3) // 4 * 4 + offset
        out.append((at, n))
        at += n + gap
    assert at <= buf.numel()
    return out


@pytest.mark.parametrize("p_off,g_off", [(1, 0), (0, 2), (3, 3), (2, 1)])
def test_misaligned_views(cuda, lib, p_off, g_off):
    """Parameters and / or gradients as views at element offsets 1, 2, 3 into one buffer each; whatever lies between the views must keep its
    sentinel (an over-wide vector store would change it), with consume_grads storing into the gradient buffer as well."""
    sizes = [n for n in edge_sizes(lib) if n]
    total = sum(sizes) + 16 * len(sizes) + 16
    pbuf = torch.full((total,), SENTINEL, device=cuda)
    gbuf = torch.full((total,), SENTINEL, device=cuda)
    pv, gv = views_into(pbuf, sizes, p_off), views_into(gbuf, sizes, g_off)
    init, grads = seeded(sizes, 2, 0.5), seeded(sizes, 3)
    params = []
    for (at, n), a in zip(pv, init):
        pbuf[at:at + n] = torch.from_numpy(a).to(cuda)
        params.append(torch.nn.Parameter(pbuf[at:at + n]))
        assert params[-1].data_ptr() == pbuf.data_ptr() + 4 * at
    for (at, n), g, p in zip(gv, grads, params):
        gbuf[at:at + n] = torch.from_numpy(g).to(cuda)
        p.grad = gbuf[at:at + n]
        assert p.grad.data_ptr() == gbuf.data_ptr() + 4 * at
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=5.0, consume_grads=True, **MODES["decoupled"])
    before = snapshot(opt, params)
    opt.step()
    check_step(opt, params, before, grads, 0.01, OR.DECOUPLED, 5.0, what=f"offsets {p_off},{g_off}")
    for buf, views in ((pbuf, pv), (gbuf, gv)):
        keep = np.ones(total, bool)
        for at, n in views:
            keep[at:at + n] = False
        assert (host(buf)[keep] == SENTINEL).all()
    for at, n in gv:
        assert not host(gbuf[at:at + n]).any()                      # consumed


# ---- presence ------------------------------------------------------------------------------------------------------------------------------------
def test_absent_gradients_are_skipped(cuda, lib):
    sizes = [37, 5000, 64, 9]
    params = [torch.nn.Parameter(torch.from_numpy(a).to(cuda)) for a in seeded(sizes, 4, 0.5)]
    params[2].requires_grad_(False)
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=5.0, **MODES["decoupled"])
    grads = seeded(sizes, 5)
    grads[1] = grads[2] = None
    before = snapshot(opt, params)
    set_grads(params, grads)
    opt.step()
    check_step(opt, params, before, grads, 0.01, OR.DECOUPLED, 5.0, what="absent")
    assert sorted(opt.state_dict()["state"]) == [0, 3]
    # the skipped parameter gets a gradient: its bias corrections use its own t = 1 while the others are at t = 2
    grads = seeded(sizes, 6)
    grads[2] = None
    before = snapshot(opt, params)
    assert before[3] == [1, 0, 0, 1]
    set_grads(params, grads)
    opt.step()
    check_step(opt, params, before, grads, 0.01, OR.DECOUPLED, 5.0, what="late joiner")
    assert snapshot(opt, params)[3] == [2, 1, 0, 2]


# ---- clipping ------------------------------------------------------------------------------------------------------------------------------------
def one_step(cuda, init, grads, max_norm, mode="decoupled", **kw):
    params = [torch.nn.Parameter(torch.from_numpy(a).to(cuda)) for a in init]
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=max_norm, **MODES[mode], **kw)
    before = snapshot(opt, params)
    set_grads(params, grads)
    opt.step()
    return opt, params, before


def test_clip_below_above_and_at_max_norm(cuda, lib):
    sizes = [300, 4100, 7]
    init, grads = seeded(sizes, 7, 0.5), seeded(sizes, 8)
    exact = OR.total_norm64(grads)
    at = np.float32(exact)
    for max_norm in (100.0 * exact, 0.01 * exact, float(at), float(np.nextafter(at, np.float32(np.inf))), float(np.nextafter(at, np.float32(0)))):
        opt, params, before = one_step(cuda, init, grads, max_norm)
        check_step(opt, params, before, grads, 0.01, OR.DECOUPLED, max_norm, what=f"max_norm {max_norm!r}")


def test_all_zero_gradients_only_decay(cuda, lib):
    sizes = [300, 4100, 7]
    init = seeded(sizes, 9, 0.5)
    grads = [np.zeros(n, np.float32) for n in sizes]
    opt, params, before = one_step(cuda, init, grads, 10.0)
    assert float(opt.last_total_norm) == 0.0 and float(opt._norm_out[1]) == 1.0
    decay = np.float32(1.0 - LR * 0.01)
    for p, a in zip(params, init):
        assert np.array_equal(host(p), a * decay)


def test_no_clipping_equals_huge_max_norm(cuda, lib):
    sizes = [300, 4100, 7]
    init, grads = seeded(sizes, 11, 0.5), seeded(sizes, 12)
    a, pa, _ = one_step(cuda, init, grads, None)
    b, pb, _ = one_step(cuda, init, grads, 1e30)
    assert a.last_total_norm is None and b.last_total_norm is not None
    for x, y in zip(pa, pb):
        assert np.array_equal(host(x), host(y))


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_non_finite_gradient_pattern_equals_torch_cpu(cuda, lib, bad):
    sizes = [300, 4100]
    init, grads = seeded(sizes, 13, 0.5), seeded(sizes, 14)
    grads[1][4097] = bad
    opt, params, _ = one_step(cuda, init, grads, 10.0, mode="none")
    ref = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
    set_grads(ref, grads)
    torch.nn.utils.clip_grad_norm_(ref, 10.0)
    torch.optim.Adam(ref, lr=LR, betas=BETAS, eps=EPS).step()
    for p, r in zip(params, ref):
        assert np.array_equal(np.isfinite(host(p)), np.isfinite(host(r)))
    torch.cuda.synchronize()


# ---- the reference's trajectories ------------------------------------------------------------------------------------------------------------------
def build(name, cuda, init):
    from seevcn_amd.tools.train_utils import optimization as O
    from seevcn_amd.vcn.tools import builder
    case = OR.CASES[name]
    model = OR.make_model().to(cuda)
    OR.load_params(model, init)
    if case["kind"] == "pcdet":
        opt = O.build_optimizer(model, case["cfg"])
        sched, _ = O.build_scheduler(opt, case["iters"], case["epochs"], -1, case["cfg"])
        return model, opt, sched, case["cfg"].OPTIMIZER == "adam_onecycle"
    opt, sched = builder.build_opti_sche(model, case["cfg"], case["iters"], case["epochs"])
    return model, opt, sched, False


def run_step(model, opt, sched, onecycle, k, grads):
    if onecycle:
        sched.step(k)
    opt.zero_grad()
    OR.set_grads(model, grads)
    lr, mom = [g["lr"] for g in opt.param_groups], [g["betas"][0] for g in opt.param_groups]
    opt.step()
    if not onecycle:
        sched.step()
    return lr, mom


def case_arrays(name):
    model = OR.make_model()
    return OR.seeded_arrays(model, seed=100 + list(OR.CASES).index(name))


@pytest.mark.parametrize("name", list(OR.CASES))
def test_trajectory_equals_reference(cuda, golden, name):
    init, grads = case_arrays(name)
    model, opt, sched, onecycle = build(name, cuda, init)
    inner = opt.opt if onecycle else opt
    n = sum(a.size for a in init)
    for k in range(OR.K):
        lr, mom = run_step(model, opt, sched, onecycle, k, grads[k])
        assert lr == golden[f"{name}/lr"][k].tolist() and mom == golden[f"{name}/mom"][k].tolist(), (k, lr, mom)
        for i, p in enumerate(model.parameters()):
            assert_close_per_channel(host(p), golden[f"{name}/p{k + 1}/{i}"], rtol=1e-3, atol_frac=1e-4, name=f"{name} step {k + 1} param {i}")
        ref = float(golden[f"{name}/total_norm"][k])
        if ref:
            assert abs(float(inner.last_total_norm) - ref) <= ((n + 2) / 2 + 2) * OR.U * ref      # the reference's own fp32 sum: test_optim_reference.py
        else:
            assert inner.last_total_norm is None
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == len(golden[f"{name}/weight_decay3"])
    for gi, g in enumerate(sd["param_groups"]):
        assert g["params"] == golden[f"{name}/sd3/group/{gi}"].tolist()
    assert [g["weight_decay"] for g in sd["param_groups"]] == golden[f"{name}/weight_decay3"].tolist()
    if onecycle:
        bn = {id(p) for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d) for p in m.parameters()}
        assert {id(p) for p in inner.param_groups[1]["params"]} == bn and not bn & {id(p) for p in inner.param_groups[0]["params"]}


def reference_checkpoint(golden, name, lr, betas):
    """The reference wrapper's state_dict after step 3 as torch.optim.Adam writes it (no key of ours in the groups)."""
    ngroups = len(golden[f"{name}/weight_decay3"])
    groups = [dict(lr=lr, betas=betas, eps=1e-8, weight_decay=float(golden[f"{name}/weight_decay3"][gi]), amsgrad=False, maximize=False, foreach=None,
                   capturable=False, differentiable=False, fused=None, params=golden[f"{name}/sd3/group/{gi}"].tolist()) for gi in range(ngroups)]
    state = {}
    for gi in range(ngroups):
        for idx in groups[gi]["params"]:
            state[idx] = {k: torch.from_numpy(np.asarray(golden[f"{name}/sd3/state/{idx}/{k}"])) for k in ("step", "exp_avg", "exp_avg_sq")}
    return {"state": state, "param_groups": groups}


def test_checkpoint_from_reference_and_round_trip(cuda, golden):
    name = "onecycle7"
    init, grads = case_arrays(name)
    p3 = [golden[f"{name}/p3/{i}"] for i in range(len(init))]
    model, opt, sched, _ = build(name, cuda, p3)
    opt.load_state_dict(reference_checkpoint(golden, name, float(golden[f"{name}/lr"][2, 0]), (float(golden[f"{name}/mom"][2, 0]), 0.99)))
    run_step(model, opt, sched, True, 3, grads[3])
    for i, p in enumerate(model.parameters()):
        assert_close_per_channel(host(p), golden[f"{name}/p4/{i}"], rtol=1e-3, atol_frac=1e-4, name=f"step 4 from the reference's checkpoint, param {i}")
    # our own checkpoint has the reference's layout, and a fresh optimizer that loads it continues with equal bits
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(len(init))) and all(float(s["step"]) == 4.0 and s["step"].dtype == torch.float32 for s in sd["state"].values())
    idx = OR.optimizer_index(model, split=True)
    for i, p in enumerate(model.parameters()):
        assert tuple(sd["state"][idx[i]]["exp_avg"].shape) == tuple(p.shape)
    p4 = [host(p) for p in model.parameters()]
    run_step(model, opt, sched, True, 4, grads[4])
    model2, opt2, sched2, _ = build(name, cuda, p4)
    opt2.load_state_dict(sd)
    run_step(model2, opt2, sched2, True, 4, grads[4])
    for a, b in zip(model.parameters(), model2.parameters()):
        assert np.array_equal(host(a), host(b))
    assert float(opt.opt.last_total_norm) == float(opt2.opt.last_total_norm)
    opt2.clear()
    assert opt2.state_dict()["state"] == {}


# ---- repeatability ---------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_equal_bits(cuda, lib):
    C = lib.sv_optim_chunk_elems()
    sizes = [300 * C + 5, 33, C + 1]
    init = seeded(sizes, 15, 0.5)
    grads = [seeded(sizes, 16 + k, s) for k, s in enumerate((1.0, 0.001, 0.1))]
    runs = []
    for _ in range(2):
        params = [torch.nn.Parameter(torch.from_numpy(a).to(cuda)) for a in init]
        opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=5.0, **MODES["decoupled"])
        norms = []
        for g in grads:
            set_grads(params, g)
            opt.step()
            norms.append(opt.last_total_norm.clone())
        assert opt._nchunks >= 300
        runs.append(([host(p) for p in params], [float(x) for x in norms]))
    assert runs[0][1] == runs[1][1]
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    exact = OR.total_norm64(grads[0])
    assert abs(runs[0][1][0] - exact) <= OR.total_norm_bound(exact, sum(sizes))


# ---- consume_grads and the cost of a step --------------------------------------------------------------------------------------------------------
class Counting:
    """The loaded library with every call through it recorded by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def counted(opt, monkeypatch):
    """Record every call into the loaded library, whoever makes it: the entries of the library object itself are wrapped until the test ends."""
    from seevcn_amd._lib import SIGNATURES
    calls = Counting(opt._lib)
    for name in SIGNATURES:
        monkeypatch.setattr(opt._lib, name, getattr(calls, name))
    return calls


def test_consume_grads(cuda, lib, monkeypatch):
    w = torch.nn.Parameter(torch.from_numpy(seeded([5000], 20)[0]).to(cuda))
    x = torch.from_numpy(seeded([5000], 21)[0]).to(cuda)
    opt = FusedAdam([w], lr=LR, betas=BETAS, eps=EPS, max_grad_norm=5.0, consume_grads=True)
    calls = counted(opt, monkeypatch)
    (w * x).sum().backward()
    (w * x).sum().backward()                                        # two backward passes accumulate as usual
    assert np.array_equal(host(w.grad), 2 * host(x))
    addr = w.grad.data_ptr()
    opt.step()
    assert not host(w.grad).any() and w.grad.data_ptr() == addr
    n = len(calls.calls)
    opt.zero_grad()
    assert len(calls.calls) == n and w.grad is not None and w.grad.data_ptr() == addr
    (w * x).sum().backward()
    assert np.array_equal(host(w.grad), host(x))
    opt.step()
    assert opt.table_uploads == 1 and not host(w.grad).any()


def sync_mode_is_honoured(cuda):
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=cuda).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("ntensors", [3, 300])
def test_cost_shape(cuda, lib, ntensors, monkeypatch):
    """At most 3 library calls a step whatever the number of tensors, one table upload (again only after the gradients moved), no host read."""
    sizes = [17 + (i % 5) for i in range(ntensors)]
    params = [torch.nn.Parameter(torch.from_numpy(a).to(cuda)) for a in seeded(sizes, 22, 0.5)]
    opt = FusedAdam(params, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=5.0, **MODES["decoupled"])
    calls = counted(opt, monkeypatch)
    set_grads(params, seeded(sizes, 23))
    opt.step()
    first = list(calls.calls)
    assert first == ["sv_optim_grad_sqnorm", "sv_optim_adam_step"] and opt.table_uploads == 1
    opt.zero_grad(set_to_none=False)                                # in place: the gradients stay where they are
    for p in params:
        p.grad.add_(1.0)
    honoured = sync_mode_is_honoured(cuda)
    del calls.calls[:]
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls.calls == first and len(calls.calls) <= 3 and opt.table_uploads == 1
    old = [p.grad for p in params]                                  # kept alive, so that the new gradients cannot land on the old addresses
    opt.zero_grad(set_to_none=True)                                 # the gradients move: one more upload, once
    set_grads(params, seeded(sizes, 24))
    assert all(p.grad.data_ptr() != g.data_ptr() for p, g in zip(params, old))
    opt.step()
    assert opt.table_uploads == 2
    opt.max_grad_norm = None
    del calls.calls[:]
    opt.step()
    assert calls.calls == ["sv_optim_adam_step"] and opt.table_uploads == 2


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(cuda, lib):
    from seevcn_amd._lib import SeevcnHipError
    good = torch.nn.Parameter(torch.zeros(4, 6, device=cuda))
    with pytest.raises(TypeError, match=r"parameter 1 .*float16"):
        FusedAdam([good, torch.nn.Parameter(torch.zeros(3, device=cuda, dtype=torch.float16))])
    with pytest.raises(ValueError, match=r"parameter 1 .*not contiguous"):
        FusedAdam([good, torch.nn.Parameter(torch.zeros(6, 4, device=cuda).t())])
    with pytest.raises(SeevcnHipError, match=r"'head\.weight', parameter 0 .*CPU"):
        p = torch.nn.Parameter(torch.zeros(3))
        FusedAdam([p], names={id(p): "head.weight"})
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam([good], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        FusedAdam([good], maximize=True)
    opt = FusedAdam([good])
    good.grad = torch.zeros(6, 4, device=cuda).t()
    with pytest.raises(ValueError, match=r"gradient of parameter 0 .*not contiguous"):
        opt.step()
    good.grad = torch.zeros(4, 6, device=cuda).to_sparse()
    with pytest.raises(ValueError, match=r"gradient of parameter 0 .*sparse"):
        opt.step()
