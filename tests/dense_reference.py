"""Float64 reference, derived tolerance and case lists for the dense-layer GEMM family (csrc/vcn.hip, csrc/dense_train.hip).

Reference: act(A64 @ W64.T + bias64 + group_bias64[group(row)]) with every operand the fp32 input widened to float64.

Tolerance (derived, not measured): a K-term fp32 dot product in ANY summation order followed by two additions satisfies
    |got - ref| <= (K + 4) * 2^-23 * (|A| @ |W|.T + |bias| + |group_bias|)        element by element,
2^-23 being twice the unit roundoff of fp32 (so the bound holds whatever rounding the matrix cores use inside a product-sum, as long as every step
is within one ulp).  ReLU and LeakyReLU are 1-Lipschitz: the bound survives the activation and needs no allowance for branch flips.  The same form
with the contraction length in place of K serves sv_gemm_tn, sv_gemm_strided, sv_column_sums, sv_segment_sum and the split-K entry.

Everything here works on torch tensors of any device: the big products are made once on the CPU (products()) and the element-wise part follows the
tensors to wherever the test puts them."""
import torch

EPS = 2.0 ** -23
SLOPE = 0.01
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU)
SENTINEL = -12345.678                                   # fills what a kernel must not write; no result of the random cases is near it

# ---------------------------------------------------------------------------------------------------------------- case lists (shared by the CPU and GPU tests)
# (M, N) of the tile kernel with the tile shape gemm_tile_mode (csrc/vcn.hip) gives: t128 = ceil(M / 128) * ceil(N / 128); t128 >= 600 -> 128 x 128 (0);
# 2 * t128 >= 600 or N <= 64 -> 64 x 128 (1); else 64 x 64 (2).  M is never a multiple of 64; N = 100 / 200 / 9 leave partial column tiles.
TILE_SHAPES = [(9637, 1024, 0),     # t128 = 76 * 8 = 608 >= 600
               (5000, 1024, 1),     # t128 = 40 * 8 = 320, 2 * 320 = 640 >= 600
               (300, 9, 1),         # N <= 64
               (3000, 256, 2),      # t128 = 24 * 2 = 48
               (3000, 100, 2),      # t128 = 24
               (3000, 200, 2)]      # t128 = 48
TILE_KS = [16, 48, 128, 512]
TILE_M, TILE_N = 9637, 1024                             # every shape above is a leading block of one (TILE_M, K) x (TILE_N, K) pair per K
UNIFORM_RPG = [1, 100, 128, 1024]
MDEV_CAPACITY, MDEV_N, MDEV_K = 16384, 1024, 128
MDEV_ROWS = [1, 63, 64, 65, 3000, 5000, 16384]          # device-side tile modes 2, 2, 2, 2, 2, 1, 0 at N = 1024
LD_SHAPES = [(3000, 200, 48), (300, 9, 16), (5000, 1024, 128)]

SMALL_MS = [1, 15, 16, 17, 64]
SMALL_NS = [1, 15, 16, 17, 40]
SMALL_KS = [16, 32, 48, 80, 256, 496, 512, 528, 1040]   # < 512: 4 waves, else 16; 4-step unrolled loop with / without tail; waves without a k-step

# sv_gemm_splitk_splits >= 2: M > 64, fewer than 64 output tiles, K >= 512.  K = 1040 -> 4 splits of 272, 272, 272, 224
SPLITK_SHAPES = [(65, 100, 1040, 13), (70, 100, 2064, 7), (300, 100, 4112, 100), (130, 256, 27648, 65)]      # (M, N, K, rows_per_group)

TN_SHAPES = [(0, 100, 68), (1, 100, 68), (63, 100, 68), (4097, 100, 68),      # N, K multiples of 4, not of 16: matrix cores from M = 64 on, partial tiles
             (0, 37, 5), (1, 37, 5), (63, 37, 5), (4097, 37, 5),              # odd N, K: the strided path
             (4097, 132, 260)]                                                # several output tiles, the last ones partial
STRIDED_CONTRACTIONS = [0, 1, 7, 131, 27648]
STRIDED_ROWS_COLS = [(37, 5), (64, 40)]
SEG_CHANNELS = [1, 5, 96, 130]
SEG_RPG = [1, 7, 1024]
SEG_GROUPS = 5
LINEAR_SHAPES = [(300, 40, 64), (1000, 131, 128), (64, 7, 5), (512, 3, 6), (0, 40, 64), (0, 3, 6)]           # (M, K, N)

# group sizes of the ragged layouts: every size the issue names, boundaries on multiples of 64 and 128, tiles with one, two and many groups
GROUP_SIZES = [128,              # [0, 128): one group per tile, ends on a multiple of 128
               64, 64,           # boundaries at 192 and 256: a 128-row tile split exactly at row 64
               65, 63,           # 321, 384: second group starts in the second half of a 128-row tile, at row 1 of a 64-row tile
               1, 2, 127, 129,   # 385, 387, 514, 643
               230] + [1] * 20 + [    # 873, then twenty 1-row groups to 893: more than two groups per tile -> the general epilogue
               1024,             # 1917
               3]                # 1920 = 15 * 128


def ragged_groups(M, skip_every=7):
    """(row_group int32 (M,), number of groups): GROUP_SIZES repeated until M rows are covered (the last group is cut: it ends in a partial tile).  Every
    `skip_every`-th group id is left without rows (such a group's column max must stay -inf) and one more empty group follows the last."""
    ids, gid, rows, i = [], 0, 0, 0
    while rows < M:
        n = min(GROUP_SIZES[i % len(GROUP_SIZES)], M - rows)
        if gid % skip_every == skip_every - 1:
            gid += 1
        ids.append(torch.full((n,), gid, dtype=torch.int32))
        rows, gid, i = rows + n, gid + 1, i + 1
    return torch.cat(ids), gid + 1


# ---------------------------------------------------------------------------------------------------------------- reference
def products(a, w):
    """fp32 a (M, K), w (N, K) -> (a64 @ w64.T, |a64| @ |w64|.T), float64"""
    a64, w64 = a.detach().double(), w.detach().double()
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def act64(z, act, slope=SLOPE):
    """the activation in float64, the slope being the fp32 value the kernels receive"""
    if act == ACT_RELU:
        return z.clamp_min(0)
    if act == ACT_LRELU:
        s = float(torch.tensor(slope, dtype=torch.float32))
        return torch.where(z >= 0, z, z * s)
    return z


def expected(z, absz, contraction, bias=None, group_bias=None, groups=None, act=ACT_NONE, slope=SLOPE):
    """(reference, bound) from products(): bias (N,), group_bias (G, N) fp32 and groups (M,) integer group of every row"""
    ref, mag = z, absz
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if group_bias is not None:
        gb = group_bias.double()[groups.long()]
        ref, mag = ref + gb, mag + gb.abs()
    return act64(ref, act, slope), (contraction + 4) * EPS * mag


def assert_within(got, ref, bound, name=""):
    """|got - ref| <= bound element by element; NaN / inf in `got` fail"""
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return
    g = got.detach().double()
    assert bool(torch.isfinite(g).all()), (name, "non-finite result")
    excess = (g - ref).abs() - bound
    worst = int(excess.argmax())
    assert float(excess.reshape(-1)[worst]) <= 0.0, (name, "flat index", worst, "error", float((g - ref).abs().reshape(-1)[worst]), "bound",
                                                     float(bound.reshape(-1)[worst]) if bound.dim() else float(bound))


def _order_key(x):
    """fp32 -> int32 whose integer order is the floats' order (-0.0 below +0.0)"""
    b = x.contiguous().view(torch.int32)
    return torch.where(b >= 0, b, b ^ 0x7FFFFFFF)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def group_max_of(c, groups, n_groups):
    """column max of fp32 c (M, N) over the rows of every group -> (n_groups, N); a group without rows keeps -inf"""
    key = _order_key(torch.full((n_groups, c.shape[1]), float("-inf"), dtype=torch.float32, device=c.device))
    idx = groups.long().to(c.device)[:, None].expand(-1, c.shape[1])
    key = key.scatter_reduce(0, idx, _order_key(c), "amax", include_self=True)
    return torch.where(key >= 0, key, key ^ 0x7FFFFFFF).view(torch.float32)


def assert_group_max(gmax, c, groups, n_groups, name=""):
    """gmax must be, bit for bit, the column max of the stored c over each group's rows"""
    want = group_max_of(c, groups, n_groups)
    if not bits_equal(gmax, want):
        bad = (gmax.view(torch.int32) != want.view(torch.int32)).nonzero()
        g, n = (int(v) for v in bad[0])
        raise AssertionError((name, "group max differs at (group, column)", (g, n), "got", float(gmax[g, n]), "want", float(want[g, n]), "entries", len(bad)))


def pad_cols(t, ld, fill=float("nan")):
    """t (R, C) inside a (R, ld) buffer whose padding columns hold `fill` (NaN: must never reach a result)"""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf
