"""The opt-in order-fixed gradients: sv_chamfer_backward_ordered, sv_group_points_grad_stack_ordered, sv_sa_train_backward_ordered and the
package switch seevcn_amd.set_ordered_gradients.

Every entry states its result as ONE fp32 expression per element (include/seevcn_hip.h): a sum that starts at +0.0f and takes its terms in
ascending key order, every product and sum rounded to fp32.  The references below are plain Python loops over ascending keys with np.float32
adds; the GPU results must equal them bit for bit (compared as int32 patterns).  Against the float64 oracle the bound is per element
(T + 3) * 2^-24 * sum |t_i|  (T terms t_i: recursive summation, T - 1 roundings, plus the term's own roundings and the oracle's rounding to
fp32), computed here in float64; it holds for the ordered and for the atomic route, and an element whose terms are all zero must be exactly zero.
A sum that starts at +0.0f is never -0.0f (x + y is -0 only when both are), so no output element may carry the bits 0x80000000."""
import functools

import numpy as np
import pytest

F = np.float32
U = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.int32)


def _assert_bits(got, want, name, ordered_sum=True):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{name}: {len(bad)} of {got.size} elements differ in their bits, first at {bad[0].tolist()}"
    assert not (ordered_sum and np.any(got == np.int32(-2 ** 31))), f"{name}: -0.0 in a sum that starts at +0.0"


def _assert_bound(got, exact, bound, name):
    err = np.abs(np.asarray(got, np.float64) - exact)
    print(f"{name}: largest error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}, elements with zero bound: {int(np.sum(bound == 0))}")
    assert np.all(err <= bound), f"{name}: {int(np.sum(err > bound))} elements outside (T + 3) 2^-24 sum|t|, worst excess {np.max(err - bound):.3e}"


# ------------------------------------------------------------------------------------------------ Chamfer
def _chamfer_case(name):
    """xyz1 (B,n,3), xyz2 (B,m,3), idx1, idx2 (the oracle's nearest neighbours), grad_dist1, grad_dist2; full-mantissa values"""
    from oracle import chamfer as oc
    if name == "three":                        # every point of cloud 1 is nearest one of three points: lists of 100 hits, more than a wave
        rng = np.random.default_rng(11)
        x2 = np.array([[[0, 0, 0], [10, 0, 0], [0, 10, 0]]], F) + rng.normal(0, 0.1, (1, 3, 3)).astype(F)
        x1 = (np.repeat(x2, 100, axis=1) + rng.normal(0, 1, (1, 300, 3))).astype(F)
    else:
        B, n, m, seed = {"tile": (2, 7, 513, 12), "edge": (3, 256, 257, 13), "zero_g2": (2, 7, 513, 14)}[name]
        rng = np.random.default_rng(seed)
        x1, x2 = rng.normal(0, 1, (B, n, 3)).astype(F), rng.normal(0, 1, (B, m, 3)).astype(F)
        if name == "zero_g2":
            x1[0, 3] = x2[0, 100]              # a point on its neighbour: its own term is (2 g) * 0
    _, _, i1, i2 = oc.forward(x1, x2)
    g1, g2 = rng.normal(0, 1, i1.shape).astype(F), rng.normal(0, 1, i2.shape).astype(F)
    if name == "three":
        assert np.bincount(i1[0], minlength=3).min() >= 65
    if name == "zero_g2":
        g2[:] = 0
        g1[0, 3] = -1.5                        # (2 * -1.5) * +0.0 = -0.0, and +0.0 + -0.0 = +0.0: the expected sign is plus
    return x1, x2, i1, i2, g1, g2


def _chamfer_side(pa, pb, ia, ga, ib, gb):
    """One cloud of one object in the stated order -> (fp32 result, float64 sum, float64 sum of |terms|, term count), each (n, 3)"""
    n = len(pa)
    out, exact, mag, cnt = np.zeros((n, 3), F), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    pa64, pb64 = pa.astype(np.float64), pb.astype(np.float64)
    for i in range(n):
        acc = np.zeros(3, F)                                                     # +0.0f
        acc = acc + (F(2) * ga[i]) * (pa[i] - pb[ia[i]])                         # the point's own term first
        t = (2.0 * float(ga[i])) * (pa64[i] - pb64[ia[i]])
        exact[i] += t
        mag[i] += np.abs(t)
        cnt[i] += 1
        for k in np.nonzero(ib == i)[0]:                                         # then the other cloud's hits, ascending k
            acc = acc + -((F(2) * gb[k]) * (pb[k] - pa[i]))
            t = -((2.0 * float(gb[k])) * (pb64[k] - pa64[i]))
            exact[i] += t
            mag[i] += np.abs(t)
            cnt[i] += 1
        out[i] = acc
    return out, exact, mag, cnt


@functools.lru_cache(maxsize=None)
def _chamfer_ref(name):
    x1, x2, i1, i2, g1, g2 = _chamfer_case(name)
    r1, r2 = [], []
    for b in range(len(x1)):
        r1.append(_chamfer_side(x1[b], x2[b], i1[b], g1[b], i2[b], g2[b]))
        r2.append(_chamfer_side(x2[b], x1[b], i2[b], g2[b], i1[b], g1[b]))
    stack = lambda rs: tuple(np.stack([r[j] for r in rs]) for j in range(4))
    return stack(r1), stack(r2)


CHAMFER_CASES = ["tile", "three", "edge", "zero_g2"]


# ------------------------------------------------------------------------------------------------ stacked group-points gradient
GP_N, GP_M, GP_NS = (5, 9), (70, 3), 16
GP_EMPTY = 41                                   # the ball with the empty mark: idx = [-1, 0, 0, ...] as ball_query leaves it


def _balls(rng, n_rows, n_queries, nsample, unused):
    """(n_queries, nsample) scene-local indices as ball_query writes them: the hits ascending, the rest repeats of the first hit"""
    allowed = np.array([r for r in range(n_rows) if r not in unused])
    idx = np.empty((n_queries, nsample), np.int32)
    for q in range(n_queries):
        hits = np.sort(rng.choice(allowed, size=int(rng.integers(1, min(nsample, len(allowed)) + 1)), replace=False))
        idx[q] = hits[0]
        idx[q, :len(hits)] = hits
    return idx


@functools.lru_cache(maxsize=None)
def _gp_case(C):
    rng = np.random.default_rng(100 + C)
    idx = np.concatenate([_balls(rng, GP_N[0], GP_M[0], GP_NS, {3}), _balls(rng, GP_N[1], GP_M[1], GP_NS, {7})])
    idx[GP_EMPTY] = 0
    idx[GP_EMPTY, 0] = -1
    row_start = np.repeat(np.array([0, GP_N[0]], np.int32), GP_M)
    grad_out = rng.normal(0, 1, (sum(GP_M), C, GP_NS)).astype(F)
    return idx, row_start, grad_out


def _gp_loop(idx, row_start, grad_out, N):
    """-> fp32 result of the stated order (N, C), float64 sum of |terms|, term counts (N,)"""
    nsample, C = idx.shape[1], grad_out.shape[1]
    out, mag, cnt = np.zeros((N, C), F), np.zeros((N, C)), np.zeros(N)
    for key in range(idx.size):                                                  # ascending key = m * nsample + s
        m, s = divmod(key, nsample)
        if idx[m, s] < 0:
            continue                                                             # the empty-ball mark names nothing
        n = row_start[m] + idx[m, s]
        out[n] = out[n] + grad_out[m, :, s]
        mag[n] += np.abs(grad_out[m, :, s].astype(np.float64))
        cnt[n] += 1
    return out, mag, cnt


@functools.lru_cache(maxsize=None)
def _gp_ref(C):
    return _gp_loop(*_gp_case(C), sum(GP_N))


def _gp_without_mark(C):
    """The same terms for the entries that do not know the mark (the atomic route, the oracle): the marked slot names row 0 with a zero gradient"""
    idx, row_start, grad_out = _gp_case(C)
    idx, grad_out = idx.copy(), grad_out.copy()
    grad_out[GP_EMPTY, :, 0] = 0
    idx[GP_EMPTY, 0] = 0
    return idx, row_start, grad_out


GP_CHANNELS = [1, 3, 64, 130]

# lists at the 64-lane edge of the sort: 4 support rows named by exactly 65, 64, 63 and 0 of the 12 * 16 keys, in no particular key order
EDGE_N, EDGE_M, EDGE_COUNTS, EDGE_CHANNELS = 4, 12, (65, 64, 63, 0), [3, 130]


@functools.lru_cache(maxsize=None)
def _edge_case(C):
    rng = np.random.default_rng(200 + C)
    idx = rng.permutation(np.repeat(np.arange(EDGE_N, dtype=np.int32), EDGE_COUNTS)).reshape(EDGE_M, GP_NS)
    return idx, np.zeros(EDGE_M, np.int32), rng.normal(0, 1, (EDGE_M, C, GP_NS)).astype(F)


@functools.lru_cache(maxsize=None)
def _edge_ref(C):
    return _gp_loop(*_edge_case(C), EDGE_N)


# ------------------------------------------------------------------------------------------------ SA-MSG training backward
SA_N, SA_M, SA_NS, SA_C, SA_C1, SA_C2 = (5, 7), (25, 15), 16, 16, 16, 32
SA_EMPTY = 30


@functools.lru_cache(maxsize=None)
def _sa_case():
    rng = np.random.default_rng(7)
    N, M = sum(SA_N), sum(SA_M)
    idx = np.concatenate([_balls(rng, SA_N[0], SA_M[0], SA_NS, {2}), _balls(rng, SA_N[1], SA_M[1], SA_NS, set())])
    idx[SA_EMPTY] = 0
    idx[SA_EMPTY, 0] = -1
    d = dict(idx=idx, row_start=np.repeat(np.array([0, SA_N[0]], np.int32), SA_M))
    d["xyz"], d["new_xyz"] = rng.normal(0, 1, (N, 3)).astype(F), rng.normal(0, 1, (M, 3)).astype(F)
    d["feat"] = rng.normal(0, 1, (N, SA_C)).astype(F)
    d["w1"], d["w2"] = rng.normal(0, 0.3, (SA_C1, SA_C + 3)).astype(F), rng.normal(0, 0.3, (SA_C2, SA_C1)).astype(F)
    d["g1"], d["g2"] = rng.uniform(0.5, 1.5, SA_C1).astype(F), rng.uniform(0.5, 1.5, SA_C2).astype(F)
    d["g1"][::5] *= -1
    d["g2"][::5] *= -1
    d["b1"], d["b2"] = rng.uniform(-0.3, 0.3, SA_C1).astype(F), rng.uniform(-0.3, 0.3, SA_C2).astype(F)
    d["grad_out"] = rng.normal(0, 1, (M, SA_C2)).astype(F)
    return d


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product is exact in float64, the sum is rounded to ODD there (an inexact sum takes the neighbour with the odd last bit),
    and a round-to-odd value with 53 >= 24 + 2 bits rounds to fp32 like the exact one."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                              # TwoSum: s + err == p + c exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def _sa_scatter_ref(dz1):
    """scatter (N, C1) in the stated order from dz1 (R, C1) -> fp32 result, float64 sum, float64 sum of |terms|, counts"""
    d = _sa_case()
    idx, row_start = d["idx"], d["row_start"]
    N = sum(SA_N)
    out, exact, mag, cnt = np.zeros((N, SA_C1), F), np.zeros((N, SA_C1)), np.zeros((N, SA_C1)), np.zeros(N)
    for key in range(idx.size):                                                  # ascending key = q * nsample + slot
        q, s = divmod(key, SA_NS)
        if idx[q, 0] < 0:
            continue                                                             # an empty ball names nothing
        n = row_start[q] + idx[q, s]
        out[n] = out[n] + dz1[key]
        exact[n] += dz1[key].astype(np.float64)
        mag[n] += np.abs(dz1[key].astype(np.float64))
        cnt[n] += 1
    return out, exact, mag, cnt


def _sa_run(cuda, lib, ordered):
    """sv_sa_train_forward, then the backward entry -> its outputs and work buffers as numpy arrays"""
    import torch
    import seevcn_amd._lib as L
    d = _sa_case()
    t = {k: torch.from_numpy(v).to(cuda) for k, v in d.items()}
    N, M, R, C, C1, C2, ns = sum(SA_N), sum(SA_M), sum(SA_M) * SA_NS, SA_C, SA_C1, SA_C2, SA_NS
    f32 = dict(dtype=torch.float32, device=cuda)
    u8 = dict(dtype=torch.uint8, device=cuda)
    nan = lambda *shape: torch.full(shape, float("nan"), **f32)
    proj, z1, z2 = nan(N, C1), nan(R, C1), nan(R, C2)
    sm1, si1, sm2, si2 = nan(C1), nan(C1), nan(C2), nan(C2)
    sel, aux, out = nan(M, C2), nan(M, C2), nan(M, C2)
    arg, aux_arg = torch.zeros((M, C2), **u8), torch.zeros((M, C2), **u8)
    rm1, rv1, rm2, rv2 = torch.zeros(C1, **f32), torch.ones(C1, **f32), torch.zeros(C2, **f32), torch.ones(C2, **f32)
    nb1, nb2 = torch.zeros((), dtype=torch.int64, device=cuda), torch.zeros((), dtype=torch.int64, device=cuda)
    nbytes = lib.sv_sa_train_backward_ordered_scratch_bytes(M, N, C, ns, C1, C2)
    assert nbytes > lib.sv_sa_train_scratch_bytes(C, C1, C2)
    scratch = torch.zeros(nbytes, **u8)
    p = L.ptr
    L.check(lib.sv_sa_train_forward(p(t["xyz"]), p(t["feat"]), p(t["new_xyz"]), p(t["idx"]), p(t["row_start"]), M, N, C, ns, p(t["w1"]), p(t["g1"]), p(t["b1"]),
                                    p(rm1), p(rv1), p(nb1), C1, p(t["w2"]), p(t["g2"]), p(t["b2"]), p(rm2), p(rv2), p(nb2), C2, 0.1, 1e-5, p(scratch), p(proj),
                                    p(z1), p(z2), p(sm1), p(si1), p(sm2), p(si2), p(sel), p(aux), p(arg), p(aux_arg), p(out), L.stream()), "sv_sa_train_forward")
    dy1, aux2, scatter, gf = nan(R, C1), nan(M, C2), nan(N, C1), nan(N, C)
    gw1, gw2, dg1, db1, dg2, db2 = nan(C1, C + 3), nan(C2, C1), nan(C1), nan(C1), nan(C2), nan(C2)
    entry = lib.sv_sa_train_backward_ordered if ordered else lib.sv_sa_train_backward
    L.check(entry(p(t["xyz"]), p(t["feat"]), p(t["new_xyz"]), p(t["idx"]), p(t["row_start"]), M, N, C, ns, p(t["w1"]), p(t["g1"]), p(t["b1"]), C1, p(t["w2"]),
                  p(t["g2"]), p(t["b2"]), C2, p(z1), p(z2), p(sm1), p(si1), p(sm2), p(si2), p(sel), p(arg), p(out), p(t["grad_out"]), p(scratch), p(dy1), p(aux2),
                  p(scatter), p(gf), p(gw1), p(gw2), p(dg1), p(db1), p(dg2), p(db2), L.stream()), "sv_sa_train_backward")
    torch.cuda.synchronize()
    r = dict(scatter=scatter, gf=gf, gw1=gw1, gw2=gw2, dg1=dg1, db1=db1, dg2=dg2, db2=db2, dy1=dy1, z1=z1, si1=si1)
    r = {k: v.cpu().numpy() for k, v in r.items()}
    r["coef1"] = scratch[:16 * C1].cpu().numpy().view(F).reshape(4, C1)           # {k, mean(dy), mean(dy * xhat), mean} of BatchNorm 1 (seevcn_hip.h)
    return r


def _sa_dz1(r):
    """dz1 (R, C1) from the entry's own dy1 / z1 and coefficients, with bwd1's expressions: every product and sum rounded to fp32"""
    k, md, mx, mean = r["coef1"]
    is1 = r["si1"]
    A = ((-k) * mx) * is1
    B = k * (((mx * is1) * mean) - md)
    assert A.dtype == F and B.dtype == F
    return _fma32(k[None], r["dy1"], _fma32(A[None], r["z1"], B[None]))


# ================================================================================================ CPU tests
NEW_ENTRIES = ["sv_chamfer_backward_ordered", "sv_group_points_grad_stack_ordered", "sv_sa_train_backward_ordered"]


def test_ordered_entries_are_declared_bound_and_exported(hip_lib):
    """The three entries and their scratch functions: declared in the header, exported by the library, bound in _lib.py with the header's types."""
    import ctypes
    import seevcn_amd._lib as L
    with open(L.HEADER_PATH) as f:
        protos = L.parse_declarations(f.read())
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    for name in NEW_ENTRIES + [n + "_scratch_bytes" for n in NEW_ENTRIES]:
        assert name in protos, f"{name} is not declared in seevcn_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
        ret, params = protos[name]
        restype, argtypes = L.SIGNATURES[name]
        assert restype == kinds[ret] and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            assert a == (ctypes.c_void_p if "*" in prm else kinds[prm.rsplit(" ", 1)[0]]), (name, prm)
    for name in NEW_ENTRIES:                                     # the existing entry's arguments plus `void* scratch` (the SA entry has one already)
        old = protos[name.replace("_ordered", "")][1]
        assert [p for p in protos[name][1] if p != "void* scratch"] == [p for p in old if p != "void* scratch"], name
        assert "void* scratch" in protos[name][1]
    assert hip_lib.sv_chamfer_backward_ordered_scratch_bytes(64, 1024, 1024) == 0
    assert hip_lib.sv_group_points_grad_stack_ordered_scratch_bytes(73, 14, 16) == 16 + 4 * (2 * 14 + 2 * 73 * 16)


@pytest.mark.parametrize("name", CHAMFER_CASES)
def test_chamfer_stated_order_agrees_with_the_float64_oracle(name):
    from oracle import chamfer as oc
    x1, x2, i1, i2, g1, g2 = _chamfer_case(name)
    want = oc.backward(x1, x2, i1, i2, g1, g2)
    for (ref, exact, mag, cnt), w, side in zip(_chamfer_ref(name), want, ("grad_xyz1", "grad_xyz2")):
        bound = (cnt + 3) * U * mag
        _assert_bound(ref, w.astype(np.float64), bound, f"chamfer {name} {side}: fp32 loop vs oracle")
        _assert_bound(ref, exact, bound, f"chamfer {name} {side}: fp32 loop vs its float64 terms")
        assert not np.any(_bits(ref) == np.int32(-2 ** 31))
    if name == "zero_g2":
        assert _bits(_chamfer_ref(name)[0][0])[0, 3].tolist() == [0, 0, 0]            # (2 * -1.5) * 0 = -0.0 enters, +0.0 comes out


@pytest.mark.parametrize("C", GP_CHANNELS)
def test_group_points_stated_order_agrees_with_the_float64_oracle(C):
    from oracle import pointnet2 as op
    ref, mag, cnt = _gp_ref(C)
    idx, _, grad_out = _gp_without_mark(C)
    want = op.group_points_grad(grad_out, idx, np.array(GP_M), np.array(GP_N), sum(GP_N))
    _assert_bound(ref, want, (cnt[:, None] + 3) * U * mag, f"group_points_grad C={C}: fp32 loop vs oracle")
    assert cnt.max() > 64 and cnt[3] == 0 and cnt[GP_N[0] + 7] == 0
    assert np.all(_bits(ref)[cnt == 0] == 0)


@pytest.mark.parametrize("C", EDGE_CHANNELS)
def test_group_points_edge_lists_agree_with_the_float64_oracle(C):
    from oracle import pointnet2 as op
    ref, mag, cnt = _edge_ref(C)
    idx, _, grad_out = _edge_case(C)
    want = op.group_points_grad(grad_out, idx, np.array([EDGE_M]), np.array([EDGE_N]), EDGE_N)
    _assert_bound(ref, want, (cnt[:, None] + 3) * U * mag, f"group_points_grad edge lists C={C}: fp32 loop vs oracle")
    assert tuple(cnt) == EDGE_COUNTS
    assert np.all(_bits(ref)[3] == 0)


def test_fma_emulation_is_correctly_rounded():
    """_fma32 against exact rational arithmetic, including sums that sit next to an fp32 rounding tie"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a, b = rng.normal(0, 1, 2000).astype(F), rng.normal(0, 1, 2000).astype(F)
    c = rng.normal(0, 1, 2000).astype(F)
    c[:500] = (F(1) + F(2.0 ** -23) * rng.integers(0, 64, 500).astype(F)) + F(2.0 ** -24) - (a[:500].astype(np.float64) * b[:500]).astype(F)
    got = _fma32(a, b, c)
    for i in range(len(a)):
        v = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F(float(v))                                                        # candidates: the fp32 neighbours of the exact value
        cands = [lo, np.nextafter(lo, F(np.inf)), np.nextafter(lo, F(-np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - v), int(_bits(x).ravel()[0]) & 1))
        assert _bits(got[i]).ravel()[0] == _bits(best).ravel()[0], (i, a[i], b[i], c[i])


def test_ordered_entries_refuse_cpu_tensors_and_keys_past_int32(hip_lib):
    import torch
    import seevcn_amd
    import seevcn_amd._lib as L
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as raw
    from seevcn_amd.vcn.extensions.chamfer_dist import chamfer
    with seevcn_amd.set_ordered_gradients(True):
        with pytest.raises(L.SeevcnHipError):
            chamfer.backward(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32),
                             torch.zeros(1, 4), torch.zeros(1, 4))
        with pytest.raises(L.SeevcnHipError):
            raw.group_points_grad_wrapper(1, 2, 1, 3, 16, torch.zeros(2, 1, 16), torch.zeros(2, 16, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
                                          torch.tensor([3], dtype=torch.int32), torch.zeros(3, 1))
    assert not seevcn_amd.ordered_gradients()
    # sizes only: the argument checks come before any pointer is read
    M = 1 << 27                                                                  # M * 16 = 2^31: one past the int32 keys
    assert hip_lib.sv_group_points_grad_stack_ordered_scratch_bytes(M, 1, 16) == 0
    with pytest.raises(L.SeevcnHipError, match="int32"):
        L.check(hip_lib.sv_group_points_grad_stack_ordered(M, 1, 1, 16, None, None, None, None, None, None), "sv_group_points_grad_stack_ordered")
    assert hip_lib.sv_sa_train_backward_ordered_scratch_bytes(M, 1, 16, 16, 16, 16) == 0
    with pytest.raises(L.SeevcnHipError, match="int32"):
        L.check(hip_lib.sv_sa_train_backward_ordered(*([None] * 5), M, 1, 16, 16, None, None, None, 16, None, None, None, 16, *([None] * 22)),
                "sv_sa_train_backward_ordered")
    with pytest.raises(L.SeevcnHipError, match="MLP channels"):                  # C1 restricted as in the existing SA kernels
        L.check(hip_lib.sv_sa_train_backward_ordered(*([None] * 5), 4, 1, 16, 16, None, None, None, 24, None, None, None, 16, *([None] * 22)),
                "sv_sa_train_backward_ordered")


def test_switch_is_a_flag_a_context_manager_and_follows_torch():
    import torch
    import seevcn_amd
    assert not seevcn_amd.ordered_gradients()
    seevcn_amd.set_ordered_gradients(True)
    assert seevcn_amd.ordered_gradients()
    seevcn_amd.set_ordered_gradients(False)
    assert not seevcn_amd.ordered_gradients()
    with seevcn_amd.set_ordered_gradients(True):
        assert seevcn_amd.ordered_gradients()
        with seevcn_amd.set_ordered_gradients(False):
            assert not seevcn_amd.ordered_gradients()
        assert seevcn_amd.ordered_gradients()
    assert not seevcn_amd.ordered_gradients()
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert seevcn_amd.ordered_gradients()
    finally:
        torch.use_deterministic_algorithms(before)
    assert not seevcn_amd.ordered_gradients()


# ================================================================================================ GPU tests
def _chamfer_gpu(cuda, lib, name, ordered):
    import torch
    import seevcn_amd._lib as L
    x1, x2, i1, i2, g1, g2 = (torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in _chamfer_case(name))
    B, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    o1, o2 = torch.full_like(x1, float("nan")), torch.full_like(x2, float("nan"))
    p = L.ptr
    if ordered:
        L.check(lib.sv_chamfer_backward_ordered(p(x1), p(x2), p(i1), p(i2), p(g1), p(g2), B, n, m, None, p(o1), p(o2), L.stream()), "sv_chamfer_backward_ordered")
    else:
        L.check(lib.sv_chamfer_backward(p(x1), p(x2), p(i1), p(i2), p(g1), p(g2), B, n, m, p(o1), p(o2), L.stream()), "sv_chamfer_backward")
    return o1.cpu().numpy(), o2.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHAMFER_CASES)
def test_hip_chamfer_ordered_equals_the_stated_order_bit_for_bit(cuda, hip_lib, name):
    """The entry against the fp32 ascending-key loop (atol = 0, int32 patterns), twice (run to run), and both routes against the float64 terms."""
    r1, r2 = _chamfer_ref(name)
    first, second = _chamfer_gpu(cuda, hip_lib, name, True), _chamfer_gpu(cuda, hip_lib, name, True)
    atomic = _chamfer_gpu(cuda, hip_lib, name, False)
    for got, again, atom, (ref, exact, mag, cnt), side in zip(first, second, atomic, (r1, r2), ("grad_xyz1", "grad_xyz2")):
        _assert_bits(got, ref, f"chamfer {name} {side}")
        _assert_bits(again, got, f"chamfer {name} {side}, second call")
        bound = (cnt + 3) * U * mag
        _assert_bound(got, exact, bound, f"chamfer {name} {side}: ordered")
        _assert_bound(atom, exact, bound, f"chamfer {name} {side}: atomic")


def _gp_gpu(cuda, lib, C, ordered, case=None, N=sum(GP_N)):
    import torch
    import seevcn_amd._lib as L
    idx, row_start, grad_out = (torch.from_numpy(a).to(cuda) for a in case or (_gp_case(C) if ordered else _gp_without_mark(C)))
    M = len(idx)
    out = torch.full((N, C), float("nan"), dtype=torch.float32, device=cuda)
    p = L.ptr
    if ordered:
        scratch = torch.empty(lib.sv_group_points_grad_stack_ordered_scratch_bytes(M, N, GP_NS), dtype=torch.uint8, device=cuda)
        L.check(lib.sv_group_points_grad_stack_ordered(M, C, N, GP_NS, p(grad_out), p(idx), p(row_start), p(scratch), p(out), L.stream()),
                "sv_group_points_grad_stack_ordered")
    else:
        L.check(lib.sv_group_points_grad_stack(M, C, N, GP_NS, p(grad_out), p(idx), p(row_start), p(out), L.stream()), "sv_group_points_grad_stack")
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("C", GP_CHANNELS)
def test_hip_group_points_grad_ordered_equals_the_stated_order_bit_for_bit(cuda, hip_lib, C):
    """Two scenes with row_start offsets, padded balls, one empty mark, a row with more than 64 keys and rows with none (bits 0x00000000)."""
    ref, mag, cnt = _gp_ref(C)
    got, again, atom = _gp_gpu(cuda, hip_lib, C, True), _gp_gpu(cuda, hip_lib, C, True), _gp_gpu(cuda, hip_lib, C, False)
    _assert_bits(got, ref, f"group_points_grad C={C}")
    _assert_bits(again, got, f"group_points_grad C={C}, second call")
    assert np.all(_bits(got)[cnt == 0] == 0)
    idx, _, grad_out = _gp_without_mark(C)
    from oracle import pointnet2 as op
    exact = op.group_points_grad(grad_out, idx, np.array(GP_M), np.array(GP_N), sum(GP_N))
    bound = (cnt[:, None] + 3) * U * mag
    _assert_bound(got, exact, bound, f"group_points_grad C={C}: ordered")
    _assert_bound(atom, exact, bound, f"group_points_grad C={C}: atomic")


@pytest.mark.gpu
@pytest.mark.parametrize("C", EDGE_CHANNELS)
def test_hip_group_points_grad_ordered_lists_at_the_wave_edge(cuda, hip_lib, C):
    """Rows named by exactly 65, 64 and 63 keys (the sort's second trip of a wave, a full wave, one lane short) and a row named by none;
    C = 130 crosses the 128-channel trip.  Bit for bit the fp32 ascending-key loop, twice; the unnamed row is +0.0f."""
    ref, _, cnt = _edge_ref(C)
    got, again = (_gp_gpu(cuda, hip_lib, C, True, _edge_case(C), EDGE_N) for _ in range(2))
    _assert_bits(got, ref, f"group_points_grad edge lists C={C}")
    _assert_bits(again, got, f"group_points_grad edge lists C={C}, second call")
    assert tuple(cnt) == EDGE_COUNTS and np.all(_bits(got)[3] == 0)


@pytest.mark.gpu
def test_hip_group_points_grad_through_autograd_follows_the_switch(cuda, hip_lib):
    import torch
    import seevcn_amd
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    C = 3
    idx, _, grad_out = (torch.from_numpy(a).to(cuda) for a in _gp_without_mark(C))
    ref = _gp_ref(C)[0]
    feats = torch.zeros((sum(GP_N), C), device=cuda, requires_grad=True)
    fcnt, qcnt = torch.tensor(GP_N, dtype=torch.int32, device=cuda), torch.tensor(GP_M, dtype=torch.int32, device=cuda)

    def grad():
        feats.grad = None
        pu.grouping_operation(feats, fcnt, idx, qcnt).backward(grad_out)
        return feats.grad.cpu().numpy()

    calls = seevcn_amd.ordered_gradient_calls()["group_points"]
    grad()
    assert seevcn_amd.ordered_gradient_calls()["group_points"] == calls          # off: the atomic entry
    with seevcn_amd.set_ordered_gradients(True):
        a, b = grad(), grad()
    assert seevcn_amd.ordered_gradient_calls()["group_points"] == calls + 2
    _assert_bits(a, ref, "grouping_operation backward, ordered")
    _assert_bits(b, a, "grouping_operation backward, second call")


@pytest.mark.gpu
def test_hip_sa_train_backward_ordered_scatter(cuda, hip_lib):
    """One scale (C 16, C1 16, C2 32, nsample 16, 40 queries over 12 support points in two scenes, padded balls, one empty ball, one unnamed point).
    (a) a second call gives the same bits in every output; (b) scatter equals, bit for bit, the fp32 ascending-key loop over dz1, where dz1 is formed
    here from the entry's own dy1 / z1 buffers and BatchNorm-1 coefficients with the kernel's fmaf expression (an exact fmaf emulation, see
    _fma32); grad_features = scatter . w1[:, 3:] comes from the unchanged k_sa_feat_grad and is covered by (a).  Both routes lie within the
    float64 bound over the dz1 terms, and everything but scatter / grad_features has the atomic route's bits."""
    first, second, atomic = _sa_run(cuda, hip_lib, True), _sa_run(cuda, hip_lib, True), _sa_run(cuda, hip_lib, False)
    for k in ("scatter", "gf", "gw1", "gw2", "dg1", "db1", "dg2", "db2", "dy1"):
        assert not np.isnan(first[k]).any(), f"{k}: an element was never written"
        _assert_bits(second[k], first[k], f"sa_train_backward_ordered {k}, second call", ordered_sum=False)
    for k in ("gw2", "dg1", "db1", "dg2", "db2", "dy1", "coef1"):
        assert np.array_equal(_bits(atomic[k]), _bits(first[k])), f"{k} differs from the default route"
    assert np.array_equal(_bits(atomic["gw1"][:, :3]), _bits(first["gw1"][:, :3]))
    dz1 = _sa_dz1(first)
    ref, exact, mag, cnt = _sa_scatter_ref(dz1)
    assert cnt.max() > 64 and cnt[2] == 0
    _assert_bits(first["scatter"], ref, "scatter")
    assert np.all(_bits(first["scatter"])[cnt == 0] == 0)
    bound = (cnt[:, None] + 3) * U * mag
    _assert_bound(first["scatter"], exact, bound, "scatter: ordered")
    _assert_bound(atomic["scatter"], exact, bound, "scatter: atomic")


def _chamfer_loss_grads(cuda):
    import torch
    from seevcn_amd.vcn.extensions.chamfer_dist import ChamferDistanceL2
    x1, x2 = (torch.from_numpy(a).to(cuda).requires_grad_(True) for a in _chamfer_case("three")[:2])
    loss = ChamferDistanceL2()(x1, x2)
    return loss, (x1, x2)


def _sa_module_step(cuda):
    """forward of a two-scale train-mode StackSAModuleMSG on 40 queries over 12 points -> (loss, tensors whose .grad is compared)"""
    import torch
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm
    d = _sa_case()
    torch.manual_seed(0)
    m = pm.StackSAModuleMSG(radii=[0.8, 1.6], nsamples=[16, 16], mlps=[[SA_C, 16, 32], [SA_C, 16, 16]], use_xyz=True, pool_method='max_pool').to(cuda).train()
    xyz, new_xyz = torch.from_numpy(d["xyz"]).to(cuda), torch.from_numpy(d["new_xyz"]).to(cuda)
    feats = torch.from_numpy(d["feat"]).to(cuda).requires_grad_(True)
    cnt, qcnt = torch.tensor(SA_N, dtype=torch.int32, device=cuda), torch.tensor(SA_M, dtype=torch.int32, device=cuda)
    assert m._train_ok(0, xyz, new_xyz, feats) and m._train_ok(1, xyz, new_xyz, feats)
    _, out = m(xyz, cnt, new_xyz, qcnt, features=feats)
    w = torch.from_numpy(np.random.default_rng(1).normal(0, 1, tuple(out.shape)).astype(F)).to(cuda)
    return (out * w).sum(), [feats] + list(m.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["switch", "torch_deterministic"])
def test_hip_backward_reads_the_switch(cuda, hip_lib, how):
    """ChamferDistanceL2(...).backward() and one StackSAModuleMSG training backward: with the package switch, and separately with torch's
    deterministic mode, the ordered entries run (call counters) and two backwards in a row give the same bits; with both off the existing
    entries run (the counters stand still: an atomic run may legitimately have the ordered run's bits)."""
    import contextlib
    import torch
    import seevcn_amd

    @contextlib.contextmanager
    def on():
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

    for step, key, per_backward in ((_chamfer_loss_grads, "chamfer", 1), (_sa_module_step, "sa_train", 2)):
        runs = []
        for _ in range(2):
            loss, leaves = step(cuda)
            calls = seevcn_amd.ordered_gradient_calls()[key]
            with on():                                                           # read at BACKWARD time: the forward ran with the switch off
                loss.backward()
            assert seevcn_amd.ordered_gradient_calls()[key] == calls + per_backward
            runs.append([t.grad.cpu().numpy() for t in leaves])
        for a, b in zip(*runs):
            assert np.isfinite(a).all()
            _assert_bits(b, a, f"{key} gradients, second backward ({how})", ordered_sum=False)
        loss, leaves = step(cuda)
        calls = seevcn_amd.ordered_gradient_calls()[key]
        assert not seevcn_amd.ordered_gradients()
        loss.backward()
        assert seevcn_amd.ordered_gradient_calls()[key] == calls
        for t, a in zip(leaves, runs[0]):                                        # the default route: the same gradient up to the summation order
            np.testing.assert_allclose(t.grad.cpu().numpy(), a, rtol=1e-4, atol=1e-5)
        if key == "chamfer" and how == "switch":                                 # through autograd the ordered route is the stated order too
            x1, x2, i1, i2, _, _ = _chamfer_case("three")
            g1, g2 = np.full(i1.shape, 1.0 / i1.shape[1], F), np.full(i2.shape, 1.0 / i2.shape[1], F)
            want = [_chamfer_side(x1[0], x2[0], i1[0], g1[0], i2[0], g2[0])[0], _chamfer_side(x2[0], x1[0], i2[0], g2[0], i1[0], g1[0])[0]]
            _assert_bits(runs[0][0][0], want[0], "ChamferDistanceL2 backward grad_xyz1")
            _assert_bits(runs[0][1][0], want[1], "ChamferDistanceL2 backward grad_xyz2")
