"""The opt-in order-fixed gradients of the dense-batch point ops (PointRCNN's PointNet2MSG and the SA stack of PointRCNNHead):
sv_group_points_grad_batch_ordered, sv_gather_points_grad_batch_ordered, sv_three_interpolate_grad_batch_ordered, and the wrappers of
pointnet2_batch_cuda that follow seevcn_amd.set_ordered_gradients.

As in test_ordered_gradients.py: every entry states its result as ONE fp32 expression per element (include/seevcn_hip.h); the references
(batch_grad_reference.py) are numpy loops over ascending keys with np.float32 products and adds, and the GPU results must equal them bit for
bit (int32 patterns).  Against float64 the bound is per element (T + 3) * 2^-24 * sum |t_i| and holds for BOTH routes; an element with no
terms is exactly +0.0, and no output element may carry the bits 0x80000000.  Output buffers are pre-filled with NaN."""
import contextlib

import numpy as np
import pytest

import batch_grad_reference as R
from test_ordered_gradients import U, _assert_bits, _assert_bound, _bits

F = np.float32
ENTRIES = ["sv_group_points_grad_batch_ordered", "sv_gather_points_grad_batch_ordered", "sv_three_interpolate_grad_batch_ordered"]
COUNTERS = ["group_points_batch", "gather_points_batch", "three_interpolate_batch"]


def _bound(mag, cnt):
    return (cnt[:, None, :] + 3) * U * mag


# ================================================================================================ CPU tests
def test_batch_ordered_entries_are_declared_bound_and_exported(hip_lib):
    """The six names: declared in the header, exported, bound with the header's types; an ordered prototype = the plain one + `void* scratch`
    in front of the output pointer; the scratch functions return exactly 16 + 4 * (2 * rows + 2 * keys)."""
    import ctypes
    import seevcn_amd._lib as L
    with open(L.HEADER_PATH) as f:
        protos = L.parse_declarations(f.read())
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    for name in ENTRIES + [n + "_scratch_bytes" for n in ENTRIES]:
        assert name in protos, f"{name} is not declared in seevcn_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
        ret, params = protos[name]
        restype, argtypes = L.SIGNATURES[name]
        assert restype == kinds[ret] and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            assert a == (ctypes.c_void_p if "*" in prm else kinds[prm.rsplit(" ", 1)[0]]), (name, prm)
    for name in ENTRIES:
        old, new = protos[name.replace("_ordered", "")][1], protos[name][1]
        assert new == old[:-2] + ["void* scratch"] + old[-2:], name               # ..., scratch, float* grad_points, void* stream
    assert hip_lib.sv_group_points_grad_batch_ordered_scratch_bytes(3, 70, 9, 16) == 16 + 4 * (2 * 210 + 2 * 432)
    assert hip_lib.sv_gather_points_grad_batch_ordered_scratch_bytes(2, 64, 40) == 16 + 4 * (2 * 128 + 2 * 80)
    assert hip_lib.sv_three_interpolate_grad_batch_ordered_scratch_bytes(2, 300, 257) == 16 + 4 * (2 * 514 + 2 * 1800)
    assert hip_lib.sv_group_points_grad_batch_ordered_scratch_bytes(2, 5, 0, 16) == 16 + 4 * (2 * 10)     # no keys: the rows alone


def test_batch_ordered_entries_refuse_keys_past_int32_and_cpu_tensors(hip_lib):
    import torch
    import seevcn_amd
    import seevcn_amd._lib as L
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_batch_cuda as raw
    # sizes only: the argument checks come before any pointer is read.  Keys: 2^16 * 2^15 = 2^31; 3 * 2^30; rows: 2^16 * 2^15
    assert hip_lib.sv_group_points_grad_batch_ordered_scratch_bytes(1, 1, 1 << 16, 1 << 15) == 0
    with pytest.raises(L.SeevcnHipError, match="int32"):
        L.check(hip_lib.sv_group_points_grad_batch_ordered(1, 1, 1, 1 << 16, 1 << 15, None, None, None, None, None), ENTRIES[0])
    with pytest.raises(L.SeevcnHipError, match="int32"):
        L.check(hip_lib.sv_group_points_grad_batch_ordered(1 << 16, 1, 1 << 15, 1, 1, None, None, None, None, None), ENTRIES[0])
    assert hip_lib.sv_gather_points_grad_batch_ordered_scratch_bytes(2, 1, 1 << 30) == 0
    with pytest.raises(L.SeevcnHipError, match="int32"):
        L.check(hip_lib.sv_gather_points_grad_batch_ordered(2, 1, 1, 1 << 30, None, None, None, None, None), ENTRIES[1])
    assert hip_lib.sv_three_interpolate_grad_batch_ordered_scratch_bytes(1, 1 << 30, 1) == 0
    with pytest.raises(L.SeevcnHipError, match="int32"):
        L.check(hip_lib.sv_three_interpolate_grad_batch_ordered(1, 1, 1 << 30, 1, None, None, None, None, None, None), ENTRIES[2])
    with pytest.raises(L.SeevcnHipError, match="null"):
        L.check(hip_lib.sv_group_points_grad_batch_ordered(1, 1, 4, 2, 2, None, None, None, None, None), ENTRIES[0])
    # nothing to do: SV_OK, no pointer is looked at
    assert hip_lib.sv_group_points_grad_batch_ordered(0, 1, 4, 2, 2, None, None, None, None, None) == 0
    assert hip_lib.sv_three_interpolate_grad_batch_ordered(1, 0, 4, 2, None, None, None, None, None, None) == 0
    assert hip_lib.sv_three_interpolate_grad_batch_ordered(1, 1, 4, 0, None, None, None, None, None, None) == 0
    i32 = dict(dtype=torch.int32)
    with seevcn_amd.set_ordered_gradients(True):
        with pytest.raises(L.SeevcnHipError):
            raw.group_points_grad_wrapper(1, 1, 4, 2, 2, torch.zeros(1, 1, 2, 2), torch.zeros(1, 2, 2, **i32), torch.zeros(1, 1, 4))
        with pytest.raises(L.SeevcnHipError):
            raw.gather_points_grad_wrapper(1, 1, 4, 2, torch.zeros(1, 1, 2), torch.zeros(1, 2, **i32), torch.zeros(1, 1, 4))
        with pytest.raises(L.SeevcnHipError):
            raw.three_interpolate_grad_wrapper(1, 1, 4, 2, torch.zeros(1, 1, 4), torch.zeros(1, 4, 3, **i32), torch.zeros(1, 4, 3), torch.zeros(1, 1, 2))
    assert not seevcn_amd.ordered_gradients()


def test_ordered_gradient_calls_reports_the_batch_entries():
    import seevcn_amd
    calls = seevcn_amd.ordered_gradient_calls()
    assert set(COUNTERS) <= set(calls)
    assert {"chamfer", "group_points", "sa_train", "roiaware_pool", "three_interpolate", "vector_pool"} <= set(calls)
    assert all(isinstance(calls[k], int) for k in COUNTERS)


def _cpu_cases():
    yield from ((f"balls C={C}", R.balls_ref(C)) for C in R.BALLS_CHANNELS)
    yield "tile edge", R.tile_ref()
    yield "gather", R.gather_ref()
    yield from ((f"interpolate c={c} m={m}", R.interp_ref(c, m)) for c in R.INTERP_CHANNELS for m in R.INTERP_M)


def test_stated_order_agrees_with_its_own_float64_sum():
    for name, (ref, exact, mag, cnt) in _cpu_cases():
        _assert_bound(ref, exact, _bound(mag, cnt), f"{name}: fp32 loop vs its float64 terms")
        assert np.all(_bits(ref).transpose(0, 2, 1)[cnt == 0] == 0), name
        assert not np.any(_bits(ref) == np.int32(-2 ** 31)), name
    for c in R.INTERP_CHANNELS:
        for m in R.INTERP_M:
            b, row = R.interp_case(c, m)[3]
            ref, _, mag, cnt = R.interp_ref(c, m)
            assert cnt[b, row] >= 1 and np.all(mag[b, :, row] == 0) and np.all(_bits(ref)[b, :, row] == 0)   # -1.5 * +0.0 entered, +0.0 came out


def test_strays_name_nothing_in_the_reference():
    """The reference drops a -1 and an index equal to the row count; unguarded they would be the neighbouring batch element's rows."""
    grad_out, idx = R.balls_case(5)
    stray = R.with_strays(idx, R.BALLS["N"])
    assert (stray == -1).sum() == 2 and (stray == R.BALLS["N"]).sum() == 2 and stray[0, 17] == R.BALLS["N"] and stray[-1, 29] == -1
    _, _, _, cnt = R.group_grad(grad_out, stray, R.BALLS["N"])
    assert cnt.sum() == idx.size - 4


# ================================================================================================ GPU tests
def _group_gpu(cuda, lib, grad_out, idx, n, ordered, nsample=None):
    """nsample None: the gather entries (idx (B, npoint)); else the group entries with npoint = per / nsample"""
    import torch
    import seevcn_amd._lib as L
    B, C, per = grad_out.shape
    g, i = torch.from_numpy(grad_out).to(cuda), torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)
    out = torch.full((B, C, n), float("nan"), dtype=torch.float32, device=cuda)
    p = L.ptr
    sizes = (B, C, n, per) if nsample is None else (B, C, n, per // nsample, nsample)
    name = "sv_gather_points_grad_batch" if nsample is None else "sv_group_points_grad_batch"
    if ordered:
        nbytes = getattr(lib, name + "_ordered_scratch_bytes")(sizes[0], *sizes[2:])
        assert nbytes == 16 + 4 * (2 * B * n + 2 * B * per)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
        L.check(getattr(lib, name + "_ordered")(*sizes, p(g), p(i), p(scratch), p(out), L.stream()), name + "_ordered")
    else:
        L.check(getattr(lib, name)(*sizes, p(g), p(i), p(out), L.stream()), name)
    return out.cpu().numpy()


def _interp_gpu(cuda, lib, grad_out, idx, weight, m, ordered):
    import torch
    import seevcn_amd._lib as L
    B, c, n = grad_out.shape
    g, i, w = (torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (grad_out, idx, weight))
    out = torch.full((B, c, m), float("nan"), dtype=torch.float32, device=cuda)
    p = L.ptr
    if ordered:
        nbytes = lib.sv_three_interpolate_grad_batch_ordered_scratch_bytes(B, n, m)
        assert nbytes == 16 + 4 * (2 * B * m + 2 * 3 * B * n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
        L.check(lib.sv_three_interpolate_grad_batch_ordered(B, c, n, m, p(g), p(i), p(w), p(scratch), p(out), L.stream()), ENTRIES[2])
    else:
        L.check(lib.sv_three_interpolate_grad_batch(B, c, n, m, p(g), p(i), p(w), p(out), L.stream()), "sv_three_interpolate_grad_batch")
    return out.cpu().numpy()


def _check_case(name, run, ref4):
    """run(ordered) -> the entry's output.  Ordered == the stated order, bit for bit, twice; both routes within the bound; unnamed rows +0.0."""
    ref, exact, mag, cnt = ref4
    got, again, atom = run(True), run(True), run(False)
    _assert_bits(got, ref, name)
    _assert_bits(again, got, name + ", second call")
    bound = _bound(mag, cnt)
    _assert_bound(got, exact, bound, name + ": ordered")
    _assert_bound(atom, exact, bound, name + ": atomic")
    for route, a in (("ordered", got), ("atomic", atom)):
        assert np.all(_bits(a).transpose(0, 2, 1)[cnt == 0] == 0), f"{name}: an unnamed row is not +0.0 on the {route} route"


@pytest.mark.gpu
@pytest.mark.parametrize("C", R.BALLS_CHANNELS)
def test_hip_group_points_grad_batch_ordered_balls(cuda, hip_lib, C):
    """B 3, N 70, npoint 9, nsample 16: padded balls, a row with >= 80 keys, rows named by nothing; C = 1, 5, 35 (one channel, a tile and a
    lone channel, eight tiles and three channels)."""
    grad_out, idx = R.balls_case(C)
    _check_case(f"group_points_grad_batch balls C={C}", lambda o: _group_gpu(cuda, hip_lib, grad_out, idx, R.BALLS["N"], o, R.BALLS["nsample"]),
                R.balls_ref(C))


@pytest.mark.gpu
def test_hip_group_points_grad_batch_ordered_tile_edge(cuda, hip_lib):
    """B 2, N 257, npoint 33, nsample 32, C 3: rows cross a 256-thread tile, per = 1056 is no multiple of 256."""
    grad_out, idx = R.tile_case()
    _check_case("group_points_grad_batch tile edge", lambda o: _group_gpu(cuda, hip_lib, grad_out, idx, R.TILE["N"], o, R.TILE["nsample"]),
                R.tile_ref())


@pytest.mark.gpu
def test_hip_gather_points_grad_batch_ordered(cuda, hip_lib):
    grad_out, idx = R.gather_case()
    _check_case("gather_points_grad_batch", lambda o: _group_gpu(cuda, hip_lib, grad_out, idx, R.GATHER["N"], o), R.gather_ref())


@pytest.mark.gpu
@pytest.mark.parametrize("m", R.INTERP_M)
@pytest.mark.parametrize("c", R.INTERP_CHANNELS)
def test_hip_three_interpolate_grad_batch_ordered(cuda, hip_lib, c, m):
    """B 2, n 300; m = 2: slots of one p repeat a row; m = 5: lists of about 180 keys; m = 257: many empty rows.  One -1.5 * +0.0: plus zero."""
    grad_out, idx, weight, (b, row) = R.interp_case(c, m)
    ref4 = R.interp_ref(c, m)
    _check_case(f"three_interpolate_grad_batch c={c} m={m}", lambda o: _interp_gpu(cuda, hip_lib, grad_out, idx, weight, m, o), ref4)
    assert np.all(_bits(_interp_gpu(cuda, hip_lib, grad_out, idx, weight, m, True))[b, :, row] == 0)


@pytest.mark.gpu
def test_hip_batch_ordered_entries_drop_out_of_range_indices(cuda, hip_lib):
    """ORDERED ENTRIES ONLY (a plain entry writes wherever the index points).  A -1 and an index equal to the row count, each once in batch
    element 0 and once in the last one, name nothing: the result is the reference's, which drops them -- so nothing shows up in the
    neighbouring batch element's rows either."""
    N = R.BALLS["N"]
    grad_out, idx = R.balls_case(5)
    stray = R.with_strays(idx, N)
    ref = R.group_grad(grad_out, stray, N)[0]
    assert not np.array_equal(_bits(ref), _bits(R.balls_ref(5)[0]))
    _assert_bits(_group_gpu(cuda, hip_lib, grad_out, stray, N, True, R.BALLS["nsample"]), ref, "group_points_grad_batch_ordered with strays")
    g_out, g_idx = R.gather_case()
    g_stray = R.with_strays(g_idx, R.GATHER["N"])
    _assert_bits(_group_gpu(cuda, hip_lib, g_out, g_stray, R.GATHER["N"], True), R.group_grad(g_out, g_stray, R.GATHER["N"])[0],
                 "gather_points_grad_batch_ordered with strays")
    grad_out, idx, weight, _ = R.interp_case(7, 5)
    stray = R.with_strays(idx, 5)
    ref = R.interpolate_grad(grad_out, stray, weight, 5)[0]
    assert not np.array_equal(_bits(ref), _bits(R.interp_ref(7, 5)[0]))
    _assert_bits(_interp_gpu(cuda, hip_lib, grad_out, stray, weight, 5, True), ref, "three_interpolate_grad_batch_ordered with strays")


@pytest.mark.gpu
def test_hip_batch_ordered_entries_without_keys_write_plus_zero(cuda, hip_lib):
    """per == 0 (n == 0 for the interpolation): every element is written, +0.0f; batch == 0 writes nothing."""
    import torch
    import seevcn_amd._lib as L
    p = L.ptr
    out = torch.full((2, 5, 300), float("nan"), dtype=torch.float32, device=cuda)
    scratch = torch.empty(hip_lib.sv_group_points_grad_batch_ordered_scratch_bytes(2, 300, 0, 16), dtype=torch.uint8, device=cuda)
    L.check(hip_lib.sv_group_points_grad_batch_ordered(2, 5, 300, 0, 16, None, None, p(scratch), p(out), L.stream()), ENTRIES[0])
    assert np.all(_bits(out.cpu().numpy()) == 0)
    out.fill_(float("nan"))
    scratch = torch.empty(hip_lib.sv_three_interpolate_grad_batch_ordered_scratch_bytes(2, 0, 300), dtype=torch.uint8, device=cuda)
    L.check(hip_lib.sv_three_interpolate_grad_batch_ordered(2, 5, 0, 300, None, None, None, p(scratch), p(out), L.stream()), ENTRIES[2])
    assert np.all(_bits(out.cpu().numpy()) == 0)
    out.fill_(float("nan"))
    L.check(hip_lib.sv_group_points_grad_batch_ordered(0, 5, 300, 9, 16, None, None, p(scratch), p(out), L.stream()), ENTRIES[0])
    assert bool(torch.isnan(out).all())


@contextlib.contextmanager
def _on(how):
    import torch
    import seevcn_amd
    if how == "switch":
        with seevcn_amd.set_ordered_gradients(True):
            yield
    else:
        before = torch.are_deterministic_algorithms_enabled()
        try:
            torch.use_deterministic_algorithms(True)
            yield
        finally:
            torch.use_deterministic_algorithms(before)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["switch", "torch_deterministic"])
def test_hip_batch_autograd_follows_the_switch(cuda, hip_lib, how):
    """GroupingOperation, GatherOperation and ThreeInterpolate through .backward(): off, the counters stand still; on (the package switch, or
    torch's deterministic mode), each moves by one per backward -- also for a graph that was built with the switch off -- and the gradient has
    the direct entry's bits."""
    import torch
    import seevcn_amd
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pu
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    B, N, npoint, nsample = (R.BALLS[k] for k in ("B", "N", "npoint", "nsample"))
    g_out, g_idx = R.balls_case(5)
    a_out, a_idx = R.gather_case()
    i_out, i_idx, i_w, _ = R.interp_case(7, 5)
    ops = [
        ("group_points_batch", lambda f: pu.grouping_operation(f, t(g_idx.reshape(B, npoint, nsample))), (B, 5, N), t(g_out.reshape(B, 5, npoint, nsample)),
         lambda: _group_gpu(cuda, hip_lib, g_out, g_idx, N, True, nsample), R.balls_ref(5)),
        ("gather_points_batch", lambda f: pu.gather_operation(f, t(a_idx)), (R.GATHER["B"], R.GATHER["C"], R.GATHER["N"]), t(a_out),
         lambda: _group_gpu(cuda, hip_lib, a_out, a_idx, R.GATHER["N"], True), R.gather_ref()),
        ("three_interpolate_batch", lambda f: pu.three_interpolate(f, t(i_idx), t(i_w)), (R.INTERP_B, 7, 5), t(i_out),
         lambda: _interp_gpu(cuda, hip_lib, i_out, i_idx, i_w, 5, True), R.interp_ref(7, 5)),
    ]
    for key, forward, shape, grad_out, direct, (_, exact, mag, cnt) in ops:
        feats = torch.zeros(shape, device=cuda, requires_grad=True)

        def backward(on):
            feats.grad = None
            out = forward(feats)                                                 # the graph is built with the switch off
            assert not seevcn_amd.ordered_gradients()
            with (_on(how) if on else contextlib.nullcontext()):
                out.backward(grad_out)
            return feats.grad.cpu().numpy()

        calls = seevcn_amd.ordered_gradient_calls()[key]
        off = backward(False)
        assert seevcn_amd.ordered_gradient_calls()[key] == calls, key            # off: the atomic entry
        a, b = backward(True), backward(True)
        assert seevcn_amd.ordered_gradient_calls()[key] == calls + 2, key
        _assert_bits(a, direct(), f"{key} backward, ordered ({how})")
        _assert_bits(b, a, f"{key} backward, second call ({how})")
        _assert_bound(off, exact, _bound(mag, cnt), f"{key} backward, switch off")   # the default route: the same sum in another order
        feats.grad = None
        with _on(how):                                                           # built and run with the switch on
            forward(feats).backward(grad_out)
        assert seevcn_amd.ordered_gradient_calls()[key] == calls + 3, key
        _assert_bits(feats.grad.cpu().numpy(), a, f"{key} backward, graph built with the switch on ({how})")


@contextlib.contextmanager
def _fixed_order_backends():
    """torch's own convolutions and BatchNorm sum their weight gradients in a fixed order only when asked to (as in test_pvrcnn_plusplus.py)"""
    import torch
    import seevcn_amd
    before = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        with seevcn_amd.set_ordered_gradients(True):
            yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["sa_msg", "fp"])
def test_hip_batch_modules_repeat_bit_for_bit(cuda, hip_lib, which):
    """PointnetSAModuleMSG (max_pool) and PointnetFPModule, train mode, at the sizes of test_pointnet2_batch_modules.py: two forward + backward
    runs on the order-fixed route give the same bits in every parameter gradient and in the gradient of the input features."""
    import torch
    import seevcn_amd
    import test_pointnet2_batch_modules as TM
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as M
    xyz, feat = TM._inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    if which == "sa_msg":
        m = TM._seed_module(M.PointnetSAModuleMSG(npoint=16, radii=list(TM.RADII), nsamples=[8, 16], mlps=[[TM.C, 8, 16], [TM.C, 8, 12]],
                                                  pool_method="max_pool"), 1).to(cuda).train()
        keys = ("group_points_batch",)
    else:
        m = TM._seed_module(M.PointnetFPModule(mlp=[6 + TM.C, 16, 8]), 3).to(cuda).train()
        known_feats = np.random.default_rng(3).standard_normal((TM.B, 6, 12)).astype(F)
        keys = ("three_interpolate_batch",)

    def step():
        m.zero_grad(set_to_none=True)
        if which == "sa_msg":
            leaves = [t(feat).requires_grad_(True)]
            out = m(t(xyz), leaves[0])[1]
        else:
            leaves = [t(feat[:, :, :40]).requires_grad_(True), t(known_feats).requires_grad_(True)]
            out = m(t(xyz[:, :40]), t(xyz[:, 40:52]), leaves[0], leaves[1])
        w = t(np.random.default_rng(5).standard_normal(tuple(out.shape)).astype(F))
        (out * w).sum().backward()
        grads = {n: p.grad.cpu().numpy() for n, p in m.named_parameters()}
        grads.update({f"input {k}": v.grad.cpu().numpy() for k, v in enumerate(leaves)})
        return grads

    calls = seevcn_amd.ordered_gradient_calls()
    with _fixed_order_backends():
        first, second = step(), step()
    for k in keys:
        assert seevcn_amd.ordered_gradient_calls()[k] > calls[k], k
    assert len(first) >= 5
    for n in first:
        assert np.isfinite(first[n]).all(), n
        _assert_bits(second[n], first[n], f"{which}: gradient of {n}, second run", ordered_sum=False)


@pytest.mark.gpu
def test_hip_pointrcnn_train_step_repeats_bit_for_bit(cuda, hip_lib):
    """PointRCNN (the small config) on 2 x 512 points, seeded state dict: two train steps on the order-fixed route, each behind the same seeds
    (the proposal target layer samples), give equal bytes in the loss and in every parameter gradient."""
    import torch
    import seevcn_amd
    import pointrcnn_inputs as I
    import test_pointrcnn as TP
    from seeding import seeded_state_dict
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import detectors
    pts, gt = TP._detector_inputs()
    net = detectors.build_detector(C.pointrcnn_model_cfg(**I.SMALL), num_class=3, dataset=C.SyntheticDatasetInfo(num_point_features=4))
    net.load_state_dict(seeded_state_dict(net, seed=6))
    net = net.to(cuda).train()
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda), "points_per_scene": [512, 512]}

    def step():
        np.random.seed(0)
        torch.manual_seed(0)
        net.zero_grad(set_to_none=True)
        ret, _, _ = net(dict(batch))
        ret["loss"].backward()
        return ret["loss"].detach().cpu().numpy(), {n: p.grad.cpu().numpy() for n, p in net.named_parameters() if p.grad is not None}

    calls = seevcn_amd.ordered_gradient_calls()
    with _fixed_order_backends():
        (loss, grads), (loss2, grads2) = step(), step()
    after = seevcn_amd.ordered_gradient_calls()
    assert after["group_points_batch"] > calls["group_points_batch"] and after["three_interpolate_batch"] > calls["three_interpolate_batch"]
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
    differ = [n for n in grads if grads[n].tobytes() != grads2[n].tobytes()]
    print(len(grads), "parameter gradients compared,", len(differ), "differ between the two steps")
    assert sorted(grads) == sorted(grads2) and len(grads) > 0
    assert loss.tobytes() == loss2.tobytes(), (loss, loss2)
    assert differ == [], (len(differ), differ[:10])
