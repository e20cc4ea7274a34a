"""Training-side dense-layer kernels (csrc/dense_train.hip) and the autograd functions over them (seevcn_amd/dense_ops.py) against plain torch fp32
ops of the same layers (tolerances written per check)."""

import numpy as np
import pytest
import torch


def _close(a, b, rtol, name, atol=1e-12):
    """|a - b| <= rtol * max|b| + atol (a GEMM's sums of 10^2..10^5 fp32 products: error relative to the tensor's scale)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= rtol * scale + atol, (name, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(65536, 128, 64), (13001, 1024, 512), (512, 256, 27648), (4096, 9, 512), (65536, 128, 3), (100, 64, 64), (37, 5, 7), (1, 64, 64)])
def test_hip_gemm_tn_matches_torch(cuda, hip_lib, M, N, K):
    """dW = dY^T X (sv_gemm_tn: matrix-core path with M split over workgroups, or the strided path for odd shapes) vs float64; twice: bitwise equal"""
    from seevcn_amd import _lib
    g = torch.Generator().manual_seed(M + N + K)
    a, b = torch.randn(M, N, generator=g).to(cuda), torch.randn(M, K, generator=g).to(cuda)
    sc = torch.empty(hip_lib.sv_gemm_tn_scratch_bytes(M, N, K), dtype=torch.uint8, device=cuda)
    outs = []
    for _ in range(2):
        c = torch.full((N, K), float("nan"), device=cuda)
        _lib.check(hip_lib.sv_gemm_tn(a.data_ptr(), N, b.data_ptr(), K, c.data_ptr(), K, M, N, K, sc.data_ptr(), _lib.stream()), "sv_gemm_tn")
        outs.append(c)
    _close(outs[0], a.double().t() @ b.double(), 2e-5, "gemm_tn")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_hip_column_sums_and_segments_match_torch(cuda, hip_lib):
    from seevcn_amd import _lib
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8 * 1024, 96, generator=g).to(cuda)
    sc = torch.empty(hip_lib.sv_column_sums_scratch_bytes(x.shape[0], 96), dtype=torch.uint8, device=cuda)
    out = torch.empty(96, device=cuda)
    _lib.check(hip_lib.sv_column_sums(x.data_ptr(), 96, x.shape[0], 96, out.data_ptr(), sc.data_ptr(), _lib.stream()), "sv_column_sums")
    _close(out, x.double().sum(0), 1e-5, "column sums")
    mx, arg = torch.empty(8, 96, device=cuda), torch.empty(8, 96, dtype=torch.int32, device=cuda)
    _lib.check(hip_lib.sv_segment_max(x.data_ptr(), 96, 8, 1024, 96, mx.data_ptr(), arg.data_ptr(), _lib.stream()), "sv_segment_max")
    want, widx = x.view(8, 1024, 96).max(dim=1)
    assert torch.equal(mx, want) and torch.equal(x.view(8, 1024, 96).gather(1, arg.long()[:, None, :])[:, 0], want)
    dout = torch.randn(8, 96, generator=g).to(cuda)
    dx = torch.full_like(x, float("nan"))
    _lib.check(hip_lib.sv_segment_max_backward(dout.data_ptr(), arg.data_ptr(), 8, 1024, 96, dx.data_ptr(), 96, _lib.stream()), "sv_segment_max_backward")
    ref = torch.zeros(8, 1024, 96, device=cuda).scatter_(1, arg.long()[:, None, :], dout[:, None, :])
    assert torch.equal(dx.view(8, 1024, 96), ref)
    ss = torch.empty(8, 96, device=cuda)
    _lib.check(hip_lib.sv_segment_sum(x.data_ptr(), 96, 8, 1024, 96, ss.data_ptr(), _lib.stream()), "sv_segment_sum")
    _close(ss, x.view(8, 1024, 96).double().sum(1), 1e-5, "segment sum")


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N,act,gb", [(4096, 3, 64, 2, False), (4096, 64, 128, 2, False), (8192, 256, 512, 0, True), (64, 1024, 9, 0, False), (64, 512, 3072, 1, False),
                                           (300, 640, 128, 1, False), (512, 27648, 256, 1, False), (2048, 2048, 128, 2, True)])
def test_hip_linear_function_matches_torch_autograd(cuda, hip_lib, M, K, N, act, gb):
    """dense_ops.linear: forward and every gradient (input, weight, bias, group bias) vs torch.nn.functional.linear + activation under autograd.
    (512, 27648, 256) is the shared FC over the pooled RoI grid of PV-RCNN's head and (2048, 2048, 128) another few-tile product: split-K forward."""
    from seevcn_amd import dense_ops as D
    if K >= 2048:
        assert hip_lib.sv_gemm_splitk_splits(M, N, K) > 1
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g).to(cuda).requires_grad_(True)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda).requires_grad_(True)
    b = torch.randn(N, generator=g).to(cuda).requires_grad_(True)
    rpg = 1024
    gbt = torch.randn(M // rpg, N, generator=g).to(cuda).requires_grad_(True) if gb else None
    up = torch.randn(M, N, generator=g).to(cuda)
    y = D.linear(x, w, b, act, 0.01, gbt, rpg if gb else 1)
    (y * up).sum().backward()
    got = [y] + [t.grad.clone() for t in (x, w, b) + ((gbt,) if gb else ())]
    for t in (x, w, b) + ((gbt,) if gb else ()):
        t.grad = None
    z = torch.nn.functional.linear(x.double(), w.double(), b.double())
    if gb:
        z = z + gbt.double().repeat_interleave(rpg, dim=0)
    yr = z if act == 0 else torch.relu(z) if act == 1 else torch.nn.functional.leaky_relu(z, 0.01)
    (yr * up.double()).sum().backward()
    want = [yr] + [t.grad for t in (x, w, b) + ((gbt,) if gb else ())]
    for name, a_, b_ in zip(("y", "dx", "dw", "db", "dgb"), got, want):
        _close(a_, b_, 5e-5, name)


# VCN_VC / VCN_CN in training mode on these kernels: tests/test_vcn_train.py (against the float64 oracle pinned to the reference's float64 modules; the
# round-4 comparison with torch's fp32 modules on the GPU was a coin toss -- both fp32 sides flip ReLU branches within rounding distance of zero,
# profiles/r05_vcn_train_diag.txt)


def test_dense_ops_refuse_cpu(hip_lib):
    from seevcn_amd import _lib, dense_ops as D
    with pytest.raises(_lib.SeevcnHipError):
        D.linear(torch.zeros(4, 32), torch.zeros(8, 32))
    with pytest.raises(_lib.SeevcnHipError):
        D.segment_max(torch.zeros(8, 4), 4)


# ------------------------------------------------------------------------------------------ every training-side entry against float64 / numpy
# Tolerance: (contraction + 4) * 2^-23 * (|A| @ |B|) element by element -- tests/dense_reference.py.
def _scratch(cuda, nbytes):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=cuda).fill_(0xFF)      # NaN bit patterns: a partial sum that is read was written first


@pytest.mark.gpu
def test_hip_gemm_tn_edges_vs_float64(cuda, hip_lib):
    """sv_gemm_tn with lda / ldb / ldc larger than the widths (NaN padding in, sentinel padding out), M in {0, 1, 63, 4097}, on the matrix-core path
    (N, K multiples of 4 but not of 16: partial tiles) and the strided path (odd N, K); M = 0 gives an all-zero C; two launches agree bit for bit."""
    import dense_reference as R
    from seevcn_amd import _lib
    g = torch.Generator().manual_seed(31)
    assert {s[0] for s in R.TN_SHAPES} == {0, 1, 63, 4097}
    for (M, N, K) in R.TN_SHAPES:
        a, b = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
        z, absz = (t.to(cuda) for t in R.products(a.t(), b.t()))
        ap, bp = R.pad_cols(a.to(cuda), N + 4), R.pad_cols(b.to(cuda), K + 8)
        sc = _scratch(cuda, hip_lib.sv_gemm_tn_scratch_bytes(M, N, K))
        outs = []
        for _ in range(2):
            c = torch.full((N, K + 3), R.SENTINEL, device=cuda)
            _lib.check(hip_lib.sv_gemm_tn(ap.data_ptr() if M else None, N + 4, bp.data_ptr() if M else None, K + 8, c.data_ptr(), K + 3, M, N, K, sc.data_ptr(),
                                          _lib.stream()), "sv_gemm_tn")
            outs.append(c)
        name = f"gemm_tn {M}x{N}x{K}"
        R.assert_within(outs[0][:, :K], z, (M + 4) * R.EPS * absz, name)
        assert bool((outs[0][:, K:] == R.SENTINEL).all()), name + ": wrote into the padding of C"
        assert R.bits_equal(outs[0], outs[1]), name + ": two launches differ"
        if M == 0:
            assert bool((outs[0][:, :K] == 0).all())


@pytest.mark.gpu
def test_hip_gemm_strided_orientations_vs_float64(cuda, hip_lib):
    """sv_gemm_strided directly: the forward orientation of dense_ops (A (K,1), B (1,K)), its data-gradient orientation (A (N,1), B (K,1)), the
    weight-gradient one (both operands transposed: A (1,lda), B (ldb,1)) and A transposed against B (1,L); ldc > cols; contraction 0 .. 27 648."""
    import dense_reference as R
    from seevcn_amd import _lib
    g = torch.Generator().manual_seed(32)
    for L in R.STRIDED_CONTRACTIONS:
        for (I, J) in R.STRIDED_ROWS_COLS:
            a, b = torch.randn(I, L, generator=g), torch.randn(L, J, generator=g)            # C = a @ b
            z, absz = (t.to(cuda) for t in R.products(a, b.t()))
            a, b = a.to(cuda), b.to(cuda)
            a_t, b_t = a.t().contiguous(), b.t().contiguous()                                 # (L, I) and (J, L)
            forms = [("x @ w.T", a, (L, 1), b_t, (1, L)), ("dz @ w", a, (L, 1), b, (J, 1)), ("dz.T @ x", a_t, (1, I), b, (J, 1)), ("a.T @ w.T", a_t, (1, I), b_t, (1, L))]
            sc = _scratch(cuda, hip_lib.sv_gemm_strided_scratch_bytes(I, J, L))
            for (fname, A, (sar, sac), B, (sbc, sbj)) in forms:
                c = torch.full((I, J + 3), R.SENTINEL, device=cuda)
                _lib.check(hip_lib.sv_gemm_strided(A.data_ptr() if L else None, sar, sac, B.data_ptr() if L else None, sbc, sbj, c.data_ptr(), J + 3, I, J, L,
                                                   sc.data_ptr(), _lib.stream()), "sv_gemm_strided")
                name = f"gemm_strided {fname} {I}x{J}x{L}"
                R.assert_within(c[:, :J], z, (L + 4) * R.EPS * absz, name)
                assert bool((c[:, J:] == R.SENTINEL).all()), name + ": wrote into the padding of C"


def _flip_allowance(z64, ybound, up, act, slope):
    """A pre-activation within its forward bound of zero (and not exactly zero on both sides: bound 0) may take either activation branch in fp32.
    Such an element's dz may differ from the float64 one by |up| * (1 - slope') -- slope' = 0 for ReLU; returned as a matrix that is zero elsewhere
    and enters the gradient bounds through the same products as dz."""
    if act == 0:
        return torch.zeros_like(z64)
    amb = (z64.detach().abs() <= ybound) & (ybound > 0)
    return amb.double() * up.double().abs() * (1.0 - (slope if act == 2 else 0.0))


def _tied_rows(g, groups, rpg, C):
    """(groups * rpg, C) post-ReLU rows duplicated the way ResamplePoints duplicates an object's points (tile, permute, cut): every column max is a
    tie; column 0 is zero everywhere (all rows tie) and about half of all entries are exact zeros"""
    out = []
    for _ in range(groups):
        ni = max(1, rpg // 5)
        base = torch.relu(torch.randn(ni, C, generator=g))
        base[:, 0] = 0.0
        tiled = base.repeat(-(-rpg // ni), 1)
        out.append(tiled[torch.randperm(tiled.shape[0], generator=g)[:rpg]])
    return torch.cat(out)


@pytest.mark.gpu
def test_hip_column_sums_and_segments_with_ties_and_strides(cuda, hip_lib):
    """sv_column_sums, sv_segment_sum against float64; sv_segment_max on inputs full of ties (post-ReLU zeros, duplicated rows): arg = numpy's argmax
    (the first maximal row), and the backward writes the gradient on exactly that row, zero on the others and nothing into the padding of dx.
    ldx > channels throughout."""
    import dense_reference as R
    from seevcn_amd import _lib
    g = torch.Generator().manual_seed(33)
    G = R.SEG_GROUPS
    for C in R.SEG_CHANNELS:
        for rpg in R.SEG_RPG:
            name = f"channels={C} rows_per_group={rpg}"
            ldx, M = C + 3, G * rpg
            x = _tied_rows(g, G, rpg, C)
            x3 = x.view(G, rpg, C).double()
            xp = R.pad_cols(x.to(cuda), ldx)
            out = torch.full((C,), R.SENTINEL, device=cuda)
            sc = _scratch(cuda, hip_lib.sv_column_sums_scratch_bytes(M, C))
            _lib.check(hip_lib.sv_column_sums(xp.data_ptr(), ldx, M, C, out.data_ptr(), sc.data_ptr(), _lib.stream()), "sv_column_sums")
            R.assert_within(out.cpu(), x.double().sum(0), (M + 4) * R.EPS * x.double().abs().sum(0), "column sums " + name)
            ss = torch.full((G, C), R.SENTINEL, device=cuda)
            _lib.check(hip_lib.sv_segment_sum(xp.data_ptr(), ldx, G, rpg, C, ss.data_ptr(), _lib.stream()), "sv_segment_sum")
            R.assert_within(ss.cpu(), x3.sum(1), (rpg + 4) * R.EPS * x3.abs().sum(1), "segment sum " + name)
            mx, arg = torch.full((G, C), R.SENTINEL, device=cuda), torch.full((G, C), -7, dtype=torch.int32, device=cuda)
            _lib.check(hip_lib.sv_segment_max(xp.data_ptr(), ldx, G, rpg, C, mx.data_ptr(), arg.data_ptr(), _lib.stream()), "sv_segment_max")
            x_np = x.view(G, rpg, C).numpy()
            want_arg = x_np.argmax(axis=1)                                                        # numpy: the first occurrence
            if rpg > 1:
                assert (np.sort(x_np, axis=1)[:, -1] == np.sort(x_np, axis=1)[:, -2]).mean() > 0.5, "the input is meant to be full of ties"
            assert np.array_equal(arg.cpu().numpy(), want_arg), "segment max arg-max is not the first maximal row, " + name
            assert np.array_equal(mx.cpu().numpy(), x_np.max(axis=1)), "segment max " + name
            dout = torch.randn(G, C, generator=g)
            dx, dout_d = torch.full((M, ldx), float("nan"), device=cuda), dout.to(cuda)
            _lib.check(hip_lib.sv_segment_max_backward(dout_d.data_ptr(), arg.data_ptr(), G, rpg, C, dx.data_ptr(), ldx, _lib.stream()),
                       "sv_segment_max_backward")
            want_dx = np.zeros((G, rpg, C), np.float32)
            np.put_along_axis(want_dx, want_arg[:, None, :], dout.numpy()[:, None, :], axis=1)
            dx = dx.cpu().numpy()
            assert np.array_equal(dx[:, :C].reshape(G, rpg, C), want_dx), "segment max backward " + name
            assert np.isnan(dx[:, C:]).all(), "segment max backward wrote into the padding of dx, " + name


@pytest.mark.gpu
def test_hip_act_backward_at_zero_matches_torch(cuda, hip_lib):
    """sv_act_backward for the three activations on outputs that are exactly +0.0 / -0.0, positive and negative: bit for bit what torch's own relu /
    leaky_relu backward gives at the same points -- and the same through dense_ops.linear on zero rows with zero bias (pre-activation exactly 0),
    where every gradient is pinned to torch autograd in float64."""
    import dense_reference as R
    from seevcn_amd import _lib, dense_ops as D
    F = torch.nn.functional
    g = torch.Generator().manual_seed(34)
    n = 4099
    pre = torch.randn(n, generator=g)
    pre[::5] = 0.0
    pre[1::10] = -0.0
    dy = torch.randn(n, generator=g)
    for act in R.ACTS:
        p = pre.clone().requires_grad_(True)
        y = p * 1.0 if act == R.ACT_NONE else torch.relu(p) if act == R.ACT_RELU else F.leaky_relu(p, R.SLOPE)
        (want,) = torch.autograd.grad(y, p, dy)                                                 # torch's CPU backward at the same points
        dz, dy_d, y_d = torch.full((n,), float("nan"), device=cuda), dy.to(cuda), y.detach().to(cuda)       # named: both inputs stay allocated over the launch
        _lib.check(hip_lib.sv_act_backward(dy_d.data_ptr(), y_d.data_ptr(), n, act, R.SLOPE, dz.data_ptr(), _lib.stream()), "sv_act_backward")
        assert torch.equal(dz.cpu(), want), f"act backward act={act}"
    M, K, N = 256, 64, 96
    for act in (R.ACT_RELU, R.ACT_LRELU):
        x0 = torch.randn(M, K, generator=g)
        x0[::2] = 0.0                                                                           # every other row: pre-activation exactly 0
        w0, up = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(M, N, generator=g)
        x, w, b = x0.to(cuda).requires_grad_(True), w0.to(cuda).requires_grad_(True), torch.zeros(N, device=cuda, requires_grad=True)
        y = D.linear(x, w, b, act, R.SLOPE)
        assert bool((y[::2] == 0).all())
        (y * up.to(cuda)).sum().backward()
        x64, w64, b64 = x0.double().requires_grad_(True), w0.double().requires_grad_(True), torch.zeros(N, dtype=torch.float64, requires_grad=True)
        z64 = F.linear(x64, w64, b64)
        y64 = torch.relu(z64) if act == R.ACT_RELU else F.leaky_relu(z64, float(torch.tensor(R.SLOPE, dtype=torch.float32)))
        (dz64,) = torch.autograd.grad(y64, z64, up.double(), retain_graph=True)
        (y64 * up.double()).sum().backward()
        flip = _flip_allowance(z64, (K + 4) * R.EPS * (x0.double().abs() @ w0.double().abs().t()), up, act, R.SLOPE)
        assert bool((flip[::2] == 0).all())                                                     # the zero rows are exact on both sides: no allowance there
        R.assert_within(x.grad.cpu(), x64.grad, (N + 4) * R.EPS * (dz64.abs() @ w0.double().abs()) + flip @ w0.double().abs(), f"dx act={act}")
        R.assert_within(w.grad.cpu(), w64.grad, (M + 4) * R.EPS * (dz64.abs().t() @ x0.double().abs()) + flip.t() @ x0.double().abs(), f"dw act={act}")
        R.assert_within(b.grad.cpu(), b64.grad, (M + 4) * R.EPS * dz64.abs().sum(0) + flip.sum(0), f"db act={act}")
        if act == R.ACT_LRELU:
            assert float(b64.grad.abs().min()) > 0 and bool((dz64[::2] == up.double()[::2] * float(torch.tensor(R.SLOPE, dtype=torch.float32))).all())


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N", [(300, 40, 64), (1000, 131, 128), (64, 7, 5), (512, 3, 6), (0, 40, 64), (0, 3, 6)])
def test_hip_linear_function_odd_shapes_vs_float64_autograd(cuda, hip_lib, M, K, N):
    """dense_ops.linear where K % 32 != 0 (sv_gemm_strided forward with the epilogue in torch ops), K = 3 with N % 4 != 0, M = 0 and a non-contiguous
    x (a column slice of a wider tensor): forward and every gradient against torch autograd in float64, with and without group bias, every activation.
    Bounds: the contraction-length form of dense_reference per product, plus _flip_allowance for the few pre-activations that lie within their forward
    bound of zero (fp32 may take the other activation branch there)."""
    import dense_reference as R
    from seevcn_amd import dense_ops as D
    F = torch.nn.functional
    assert (M, K, N) in R.LINEAR_SHAPES
    slope = float(torch.tensor(R.SLOPE, dtype=torch.float32))
    g = torch.Generator().manual_seed(1000 + M + K + N)
    rpg = 4 if M else 1
    wide = torch.randn(M, K + 5, generator=g)
    w0, b0, gb0, up = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(M // rpg, N, generator=g), torch.randn(M, N, generator=g)
    x0 = wide[:, 2:K + 2]
    for act in R.ACTS:
        for hg in (True, False):
            name = f"linear {M}x{K}x{N} act={act} gb={hg}"
            wide_d = wide.to(cuda).requires_grad_(True)
            x = wide_d[:, 2:K + 2]
            assert not x.is_contiguous() or M == 0
            w, b = w0.to(cuda).requires_grad_(True), b0.to(cuda).requires_grad_(True)
            gb = gb0.to(cuda).requires_grad_(True) if hg else None
            y = D.linear(x, w, b, act, R.SLOPE, gb, rpg if hg else 1)
            (y * up.to(cuda)).sum().backward()
            x64, w64, b64 = x0.double().requires_grad_(True), w0.double().requires_grad_(True), b0.double().requires_grad_(True)
            gb64 = gb0.double().requires_grad_(True) if hg else None
            z64 = F.linear(x64, w64, b64) + (gb64.repeat_interleave(rpg, dim=0) if hg else 0)
            y64 = z64 if act == R.ACT_NONE else torch.relu(z64) if act == R.ACT_RELU else F.leaky_relu(z64, slope)
            (dz64,) = torch.autograd.grad(y64, z64, up.double(), retain_graph=True)
            (y64 * up.double()).sum().backward()
            ax, aw, adz = x0.double().abs(), w0.double().abs(), dz64.abs()
            ybound = (K + 4) * R.EPS * (ax @ aw.t() + b0.double().abs() + (gb0.double().abs().repeat_interleave(rpg, dim=0) if hg else 0))
            flip = _flip_allowance(z64, ybound, up, act, R.SLOPE)
            assert int((flip != 0).sum()) <= max(1, M * N // 1000), name + ": the branch allowance must stay an exception"
            assert y.shape == (M, N)
            R.assert_within(y.detach().cpu(), y64.detach(), ybound, name + " y")
            gx = wide_d.grad.cpu()
            assert bool((gx[:, :2] == 0).all()) and bool((gx[:, K + 2:] == 0).all())
            R.assert_within(gx[:, 2:K + 2], x64.grad, (N + 4) * R.EPS * (adz @ aw) + flip @ aw, name + " dx")
            R.assert_within(w.grad.cpu(), w64.grad, (M + 4) * R.EPS * (adz.t() @ ax) + flip.t() @ ax, name + " dw")
            R.assert_within(b.grad.cpu(), b64.grad, (M + 4) * R.EPS * adz.sum(0) + flip.sum(0), name + " db")
            if hg:
                R.assert_within(gb.grad.cpu(), gb64.grad, (rpg + 4) * R.EPS * adz.view(M // rpg, rpg, N).sum(1) + flip.view(M // rpg, rpg, N).sum(1), name + " dgb")
            if M == 0:
                assert bool((w.grad == 0).all()) and bool((b.grad == 0).all())
