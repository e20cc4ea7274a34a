"""VCN_VC / VCN_CN: oracle vs the reference's goldens (CPU); HIP path vs goldens and oracle (GPU).
Tolerance: 1e-3 relative on feature/point tensors (BASELINE.json north_star)."""
import os

import numpy as np
import pytest
import torch

from oracle import vcn as ovcn
from seeding import seeded_state_dict

RTOL = 1e-3


def _ok(a, b, rtol=RTOL, atol_frac=1e-4, name=""):
    """element-wise |a-b| <= rtol*|b| + atol_frac * max|b[..., c]| per coordinate / channel (tests/tolerances.py)"""
    from tolerances import assert_close_per_channel
    assert_close_per_channel(a, b, rtol=rtol, atol_frac=atol_frac, name=name)
    return True


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _models():
    import seevcn_amd.vcn as V
    return V


def test_registry_and_state_dict_keys():
    V = _models()
    assert set(V.MODELS.module_dict) >= {"VCN_VC", "VCN_CN"}
    m = V.MODELS.build({"NAME": "VCN_VC"})
    assert sum(p.numel() for p in m.parameters()) == 7534476
    keys = list(m.state_dict())
    assert "pose_encoder.4.weight" in keys and "encoder.mlp_conv2.1.running_var" in keys and "final_conv.6.bias" in keys
    with pytest.raises(KeyError):
        V.MODELS.build({"NAME": "nope"})
    with pytest.raises(KeyError):
        V.MODELS.build({})


def test_oracle_vcn_vc_matches_reference_golden(golden_dir):
    V = _models()
    g = np.load(os.path.join(golden_dir, "vcn_vc.npz"))
    sd = seeded_state_dict(V.MODELS.build({"NAME": "VCN_VC"}), seed=0)
    out = ovcn.vcn_vc_forward(sd, torch.from_numpy(g["input"]))
    for k in ("coarse", "reg_rot", "reg_centre"):
        assert _rel_err(out[k].numpy(), g[k]) < 1e-4, k


def test_oracle_vcn_cn_matches_reference_golden(golden_dir):
    V = _models()
    g = np.load(os.path.join(golden_dir, "vcn_cn.npz"))
    sd = seeded_state_dict(V.MODELS.build({"NAME": "VCN_CN"}), seed=0)
    out = ovcn.vcn_cn_forward(sd, torch.from_numpy(g["input"]), torch.from_numpy(g["gt_boxes"]))
    assert _rel_err(out["coarse"].numpy(), g["coarse"]) < 1e-4


def test_eval_forward_refuses_cpu_tensors():
    V = _models()
    import seevcn_amd._lib as L
    m = V.MODELS.build({"NAME": "VCN_VC"})
    with pytest.raises(L.SeevcnHipError):
        m.eval()({"input": torch.zeros(1, 1024, 3)})  # the HIP inference path has no CPU fallback
    with pytest.raises(L.SeevcnHipError):                # nor have the loss ops of the (torch-autograd) training path
        m.get_loss({"coarse": torch.zeros(1, 1024, 3), "reg_rot": torch.eye(3)[None], "reg_centre": torch.zeros(1, 3)},
                   {"gt_boxes": torch.ones(1, 7), "training": True, "complete": torch.zeros(1, 2048, 3), "input": torch.zeros(1, 1024, 3)})


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_hip_gemm_epilogues(cuda, hip_lib):
    """sv_gemm_bias_act against a torch fp32 reference: masks on M/N, bias, group bias, activations, group max."""
    from seevcn_amd.vcn.models import layers as L
    g = torch.Generator().manual_seed(0)
    for (M, N, K, rpg) in [(256, 128, 64, 128), (300, 9, 32, 100), (1024, 200, 96, 1024), (64, 3072, 1024, 1), (2048, 256, 128, 512)]:
        a = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g)
        ng = (M + rpg - 1) // rpg
        gb = torch.randn(ng, N, generator=g)
        ref = a.double() @ w.double().t() + b.double() + gb.double().repeat_interleave(rpg, 0)[:M]
        for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU):
            r = ref.clone()
            if act == L.ACT_RELU:
                r = r.clamp_min(0)
            elif act == L.ACT_LRELU:
                r = torch.where(r >= 0, r, r * 0.01)
            gm = L.neg_inf((ng, N), cuda)
            out = L.gemm(a.to(cuda), w.to(cuda), b.to(cuda), act, group_bias=gb.to(cuda), rows_per_group=rpg, group_max=gm)
            torch.cuda.synchronize()
            np.testing.assert_allclose(out.cpu().numpy(), r.numpy(), rtol=1e-4, atol=1e-4)
            rmax = torch.stack([r[i * rpg:(i + 1) * rpg].max(0)[0] for i in range(ng)])
            np.testing.assert_allclose(gm.cpu().numpy(), rmax.numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_hip_gemm_small_m_kernel(cuda, hip_lib):
    """M <= 64 without group options runs k_gemm_small_m (16 columns per workgroup, K split over the waves): every M / N / K edge,
    bias or not, all activations, against float64; and the same rows through the 128x128-tile kernel agree to fp32 rounding."""
    from seevcn_amd.vcn.models import layers as L
    g = torch.Generator().manual_seed(1)
    for (M, N, K) in [(64, 1024, 1024), (1, 9, 512), (5, 3072, 1024), (64, 9, 32), (33, 40, 64), (17, 512, 256)]:
        a = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g)
        for bias in (b, None):
            ref = a.double() @ w.double().t() + (bias.double() if bias is not None else 0)
            for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU):
                r = ref.clamp_min(0) if act == L.ACT_RELU else (torch.where(ref >= 0, ref, ref * 0.01) if act == L.ACT_LRELU else ref)
                out = L.gemm(a.to(cuda), w.to(cuda), bias.to(cuda) if bias is not None else None, act)
                np.testing.assert_allclose(out.cpu().numpy(), r.numpy(), rtol=1e-4, atol=1e-4)
        # 65 rows take the tile kernel: its first 64 rows must match the small-M result closely (different summation order)
        a65 = torch.cat([a, a[:1]], 0) if M == 64 else None
        if a65 is not None:
            big = L.gemm(a65.to(cuda), w.to(cuda), b.to(cuda), L.ACT_NONE)[:64]
            small = L.gemm(a.to(cuda), w.to(cuda), b.to(cuda), L.ACT_NONE)
            np.testing.assert_allclose(big.cpu().numpy(), small.cpu().numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_hip_vcn_vc_matches_reference_golden(golden_dir, cuda, hip_lib):
    V = _models()
    g = np.load(os.path.join(golden_dir, "vcn_vc.npz"))
    m = V.MODELS.build({"NAME": "VCN_VC"})
    m.load_state_dict(seeded_state_dict(m, seed=0))
    m = m.to(cuda).eval()
    out = m({"input": torch.from_numpy(g["input"]).to(cuda)})
    torch.cuda.synchronize()
    for k in ("coarse", "reg_rot", "reg_centre"):
        assert out[k].shape == g[k].shape
        assert _ok(out[k].cpu().numpy(), g[k], name=k)


@pytest.mark.gpu
def test_hip_vcn_cn_matches_reference_golden(golden_dir, cuda, hip_lib):
    V = _models()
    g = np.load(os.path.join(golden_dir, "vcn_cn.npz"))
    m = V.MODELS.build({"NAME": "VCN_CN"})
    m.load_state_dict(seeded_state_dict(m, seed=0))
    m = m.to(cuda).eval()
    out = m({"input": torch.from_numpy(g["input"]).to(cuda), "gt_boxes": torch.from_numpy(g["gt_boxes"]).to(cuda)})
    torch.cuda.synchronize()
    assert _ok(out["coarse"].cpu().numpy(), g["coarse"], name="coarse")


@pytest.mark.gpu
def test_hip_vcn_vc_batch64_vs_oracle_and_batch_invariance(cuda, hip_lib):
    """BASELINE config 2 size (64 objects x 1024 pts): vs oracle, and each object's result must not depend on its batch."""
    import seevcn_amd.synth as synth
    V = _models()
    clouds, _ = synth.make_object_batch(64, seed=1000)
    m = V.MODELS.build({"NAME": "VCN_VC"})
    sd = seeded_state_dict(m, seed=0)
    m.load_state_dict(sd)
    m = m.to(cuda).eval()
    x = torch.from_numpy(clouds).to(cuda)
    out = m({"input": x})
    ref = ovcn.vcn_vc_forward(sd, torch.from_numpy(clouds[:8]))
    for k in ("coarse", "reg_rot", "reg_centre"):
        assert _ok(out[k][:8].cpu().numpy(), ref[k].numpy(), name=k)
    sub = m({"input": x[5:8].contiguous()})
    assert _rel_err(sub["coarse"].cpu().numpy(), out["coarse"][5:8].cpu().numpy()) < 1e-5
    # padded zero objects (VCN.inference pads chunks with zeros, models/VCN.py:55-59) must not produce NaN
    z = m({"input": torch.zeros(2, 1024, 3, device=cuda)})
    assert torch.isfinite(z["coarse"]).all()


def test_resample_points_contract():
    from seevcn_amd.vcn.datasets.data_transforms import ResamplePoints
    pts = np.arange(90, dtype=np.float64).reshape(30, 3)
    np.random.seed(0)
    out = ResamplePoints({"n_points": 1024})(pts)
    np.random.seed(0)
    ref = np.tile(pts, (35, 1))[np.random.permutation(1050)[:1024]]          # data_transforms.py:254-262
    assert out.shape == (1024, 3) and np.array_equal(out, ref)
    big = np.random.default_rng(0).normal(size=(5000, 3))
    assert ResamplePoints({"n_points": 1024})(big).shape == (1024, 3)


@pytest.mark.gpu
def test_hip_vcn_inference_wrapper_chunking(cuda, hip_lib):
    """VCN.inference: resample -> pad to BATCH_SIZE_LIMIT -> chunks -> first num_objs rows (models/VCN.py:43-83)."""
    import seevcn_amd.synth as synth
    from seevcn_amd.vcn.VCN import VCN
    V = _models()
    sd = seeded_state_dict(V.MODELS.build({"NAME": "VCN_VC"}), seed=0)
    vcn = VCN({"MODEL": "VCN_VC", "NORM_WITH_GT": False, "SEL_K_NEAREST": 20, "CLUSTER_EPS": 0.3, "BATCH_SIZE_LIMIT": 4}, 0,
              state_dict={"module." + k: v for k, v in sd.items()})
    objs = [synth.make_object(np.random.default_rng(1000 + i))[0] for i in range(6)]
    np.random.seed(3)
    out = vcn.inference(objs, batch_size_limit=4)
    assert out["input"].shape == (6, 1024, 3) and out["coarse"].shape == (6, 1024, 3)
    ref = ovcn.vcn_vc_forward(sd, torch.from_numpy(out["input"]))["coarse"].numpy()
    assert _ok(out["coarse"], ref, name="coarse")
    # post-processing on the GPU's own coarse output (models/VCN.py:89-93) against the CPU restatement
    from oracle import postprocess as opp
    surf = opp.get_partial_mesh_batch(out["input"], out["coarse"], k=30)
    assert out["surface"].dtype == np.float32 and np.array_equal(out["surface"], surf)
    assert out["clustered"].dtype == np.float64 and np.array_equal(out["clustered"], opp.get_largest_cluster_batch(surf, eps=0.4, min_points=2))
    np.random.seed(3)
    single = vcn.inference(objs[0])
    assert np.array_equal(single["input"][0], out["input"][0]) and _ok(single["coarse"][0], ref[0], name="single coarse")


@pytest.mark.gpu
def test_hip_vcn_distinct_row_path_is_bit_identical(cuda, hip_lib):
    """ResamplePoints tiles Ni points to 1024: the per-point layers run on the distinct rows only (sv_unique_rows +
    sv_gemm_bias_act_ragged).  Output must equal the full 1024-row execution bit for bit, for VCN_VC and VCN_CN, including an
    all-zero padding object (one distinct row) and an object with 1024 distinct points."""
    import seevcn_amd.synth as synth
    V = _models()
    clouds, boxes = synth.make_object_batch(6, seed=1000)
    clouds[4] = 0.0
    clouds[5] = np.random.default_rng(0).normal(size=(1024, 3)).astype(np.float32) + np.array([20, 3, -1], np.float32)
    x, bx = torch.from_numpy(clouds).to(cuda), torch.from_numpy(boxes).to(cuda)
    for name, extra in (("VCN_VC", {}), ("VCN_CN", {"gt_boxes": bx})):
        m = V.MODELS.build({"NAME": name})
        m.load_state_dict(seeded_state_dict(m, seed=0))
        m = m.to(cuda).eval()
        m.dedup_points = True
        a = m({"input": x, **extra})                      # default: the distinct-row count never leaves the device (capacity-sized launches)
        m.dedup_points = False
        b = m({"input": x, **extra})
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)
        if name == "VCN_VC":
            import seevcn_amd.vcn.models.VCN_VC as vc_mod
            m.dedup_points = True
            saved, vc_mod.LAZY_ROWS = vc_mod.LAZY_ROWS, False
            try:
                c = m({"input": x, **extra})                  # the count read on the host, exact-size layers
            finally:
                vc_mod.LAZY_ROWS = saved
            for k in a:
                assert torch.equal(a[k], c[k]), (name, k, "host-read row count")
    from seevcn_amd.vcn.models import layers as L
    sel, rg = L.distinct_rows(x)
    sel_cap, rg_cap, u_dev = L.distinct_rows(x, sync=False)
    assert int(u_dev) == sel.shape[0] and sel_cap.shape[0] == x.shape[0] * x.shape[1]
    assert torch.equal(sel_cap[:sel.shape[0]], sel) and torch.equal(rg_cap[:sel.shape[0]], rg)
    counts = torch.bincount(rg.long(), minlength=6).cpu().numpy()
    want = [len(np.unique(clouds[i], axis=0)) for i in range(6)]
    assert counts.tolist() == want and counts[4] == 1 and counts[5] == 1024


# ------------------------------------------------------------------------------------------ the dense-layer GEMM family against float64
# Reference, tolerance |got - ref| <= (K + 4) 2^-23 (|A| @ |W|.T + |bias| + |group_bias|) and the case lists: tests/dense_reference.py.
def _tile_mode(rows, N):
    """gemm_tile_mode of csrc/vcn.hip restated: the largest tile that still gives the chip >= 600 workgroups"""
    t128 = -(-rows // 128) * -(-N // 128)
    return 0 if t128 >= 600 else 1 if (2 * t128 >= 600 or N <= 64) else 2


def _lin_ref(R, a, w, bias, act):
    z, absz = R.products(a, w)
    return R.expected(z, absz, a.shape[1], bias, None, None, act)


def test_dense_reference_bound_holds_for_torch_cpu_fp32():
    """The reference alone stays inside the derived bound: torch's own CPU fp32 linear / matmul on every shape of the case lists."""
    import dense_reference as R
    F = torch.nn.functional
    g = torch.Generator().manual_seed(7)
    for K in R.TILE_KS:                                            # every TILE_SHAPES entry is a leading block of this product
        a, w, b = torch.randn(R.TILE_M, K, generator=g), torch.randn(R.TILE_N, K, generator=g) / K ** 0.5, torch.randn(R.TILE_N, generator=g)
        z, absz = R.products(a, w)
        rg, ng = R.ragged_groups(R.TILE_M)
        gb = torch.randn(ng, R.TILE_N, generator=g)
        got = F.linear(a, w, b) + gb[rg.long()]
        for act in R.ACTS:
            ref, bound = R.expected(z, absz, K, b, gb, rg, act)
            out = got if act == R.ACT_NONE else torch.relu(got) if act == R.ACT_RELU else F.leaky_relu(got, R.SLOPE)
            for (M, N, _) in R.TILE_SHAPES:
                R.assert_within(out[:M, :N], ref[:M, :N], bound[:M, :N], f"tile K={K} {M}x{N} act={act}")
    shapes = [(max(R.SMALL_MS), max(R.SMALL_NS), K) for K in R.SMALL_KS] + [s[:3] for s in R.SPLITK_SHAPES] + [(R.MDEV_CAPACITY, R.MDEV_N, R.MDEV_K)]
    shapes += list(R.LD_SHAPES) + [(M, N, K) for (M, K, N) in R.LINEAR_SHAPES] + [(1000, 4, 3), (1000, 128, 3)]
    for (M, N, K) in shapes:
        a, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
        ref, bound = _lin_ref(R, a, w, b, R.ACT_NONE)
        R.assert_within(F.linear(a, w, b), ref, bound, f"linear {M}x{N}x{K}")
    for (M, N, K) in R.TN_SHAPES:                                  # C (N, K) = A^T B, contraction M
        a, b = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
        z, absz = R.products(a.t(), b.t())
        R.assert_within(a.t() @ b, z, (M + 4) * R.EPS * absz, f"tn {M}x{N}x{K}")
    for L in R.STRIDED_CONTRACTIONS:
        for (I, J) in R.STRIDED_ROWS_COLS:
            a, b = torch.randn(I, L, generator=g), torch.randn(J, L, generator=g)
            z, absz = R.products(a, b)
            R.assert_within(a @ b.t(), z, (L + 4) * R.EPS * absz, f"strided {I}x{J}x{L}")
    for C in R.SEG_CHANNELS:
        for rpg in R.SEG_RPG:
            x = torch.randn(R.SEG_GROUPS, rpg, C, generator=g)
            R.assert_within(x.sum(1), x.double().sum(1), (rpg + 4) * R.EPS * x.double().abs().sum(1), f"segment sum {C} {rpg}")
            R.assert_within(x.view(-1, C).sum(0), x.double().view(-1, C).sum(0), (R.SEG_GROUPS * rpg + 4) * R.EPS * x.double().abs().view(-1, C).sum(0), "col sums")


def test_dense_reference_checker_notices_faults():
    """One element moved by 4x its bound fails; a single group-max entry replaced by the second-largest value of its group fails."""
    import dense_reference as R
    g = torch.Generator().manual_seed(8)
    M, N, K = 300, 40, 48
    a, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    rg, ng = R.ragged_groups(M)
    z, absz = R.products(a, w)
    ref, bound = R.expected(z, absz, K, b, None, None, R.ACT_LRELU)
    good = ref.float()
    R.assert_within(good, ref, bound, "rounded reference")
    bad = good.clone()
    bad[123, 17] = float(ref[123, 17] + 4 * bound[123, 17])
    with pytest.raises(AssertionError):
        R.assert_within(bad, ref, bound, "moved element")
    nan = good.clone()
    nan[5, 5] = float("nan")
    with pytest.raises(AssertionError):
        R.assert_within(nan, ref, bound, "NaN element")
    gm = R.group_max_of(good, rg, ng)
    R.assert_group_max(gm, good, rg, ng, "true group max")
    empty = sorted(set(range(ng)) - set(rg.tolist()))
    assert empty and bool(torch.isinf(gm[empty]).all()) and bool((gm[empty] < 0).all())           # groups without rows keep -inf
    grp = int(rg[200])
    rows = good[rg == grp, 3]
    assert rows.numel() >= 2
    second = gm.clone()
    second[grp, 3] = torch.sort(rows, descending=True)[0][1]
    with pytest.raises(AssertionError):
        R.assert_group_max(second, good, rg, ng, "second-largest value")
    signed = torch.tensor([[-0.0], [0.0], [-1.0]])                                              # +0.0 is the max of {-0.0, +0.0}, bit for bit
    assert R.bits_equal(R.group_max_of(signed, torch.zeros(3, dtype=torch.int32), 1), torch.tensor([[0.0]]))


class _Gemm:
    """Direct calls of the three C entries with explicit leading dimensions; C starts as SENTINEL, group_max as -inf."""

    def __init__(self, lib, dev):
        from seevcn_amd import _lib
        self.lib, self.dev, self.L = lib, dev, _lib

    def __call__(self, A, lda, W, ldw, bias, gb, M, N, K, act, *, n_groups, rpg=1, row_group=None, m_dev=None, store=True, want_max=True, ldc=None):
        import dense_reference as R
        L, ldc = self.L, ldc or N
        C = torch.full((M, ldc), R.SENTINEL, device=self.dev) if store else None
        gm = torch.full((n_groups, N), float("-inf"), device=self.dev) if want_max else None
        p = lambda t: None if t is None else t.data_ptr()
        if row_group is None:
            rc = self.lib.sv_gemm_bias_act(p(A), lda, p(W), ldw, p(bias), p(gb), rpg, p(C), ldc, p(gm), M, N, K, act, R.SLOPE, L.stream())
        elif m_dev is None:
            rc = self.lib.sv_gemm_bias_act_ragged(p(A), lda, p(W), ldw, p(bias), p(gb), p(row_group), p(C), ldc, p(gm), M, N, K, act, R.SLOPE, L.stream())
        else:
            rc = self.lib.sv_gemm_bias_act_ragged_dev(p(A), lda, p(W), ldw, p(bias), p(gb), p(row_group), p(C), ldc, p(gm), M, p(m_dev), N, K, act, R.SLOPE,
                                                      L.stream())
        L.check(rc, "sv_gemm_bias_act*")
        return C, gm


def _check_instances(R, run, kw, ref, bound, groups, n_groups, rows, N, name):
    """store + max, store only and max only of one launch description: C vs float64, group_max = column max of the stored C bit for bit, the three
    instances bit-identical, padding columns and rows past `rows` still SENTINEL.  Returns the stored C (rows, N)."""
    C, gm = run(**kw, store=True, want_max=True)
    C0, _ = run(**kw, store=True, want_max=False)
    _, gm2 = run(**kw, store=False, want_max=True)
    R.assert_within(C[:rows, :N], ref, bound, name + " C")
    assert bool((C[:, N:] == R.SENTINEL).all()) and bool((C[rows:] == R.SENTINEL).all()), name + ": wrote outside the result"
    assert R.bits_equal(C0, C), name + ": store-only C differs from store+max C"
    R.assert_group_max(gm, C[:rows, :N].contiguous(), groups[:rows], n_groups, name)
    assert R.bits_equal(gm2, gm), name + ": max-only group_max differs"
    return C[:rows, :N]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [16, 48, 128, 512])
def test_hip_gemm_tile_kernel_every_path_vs_float64(cuda, hip_lib, K):
    """k_gemm_f32 through sv_gemm_bias_act and sv_gemm_bias_act_ragged: the three tile shapes, partial column tiles, the one-group / two-group fast
    epilogues and the general one (ragged layout of dense_reference.GROUP_SIZES, uniform groups of 1 / 100 / 128 / 1024 rows), every activation with
    and without bias and group bias, store+max / store / max-only.  Rows common to two shapes (leading blocks of one product) are bit-identical
    whatever the tile shape, and the uniform entry equals the ragged one on row // rows_per_group."""
    import dense_reference as R
    assert K in R.TILE_KS and [K_ for K_ in R.TILE_KS] == [16, 48, 128, 512]
    run = _Gemm(hip_lib, cuda)
    g = torch.Generator().manual_seed(100 + K)
    a, w = torch.randn(R.TILE_M, K, generator=g), torch.randn(R.TILE_N, K, generator=g) / K ** 0.5
    bias_all, gb_all = torch.randn(R.TILE_N, generator=g).to(cuda), torch.randn(R.TILE_M + 2, R.TILE_N, generator=g).to(cuda)
    z, absz = (t.to(cuda) for t in R.products(a, w))
    a, w = a.to(cuda), w.to(cuda)
    rg_all, _ = R.ragged_groups(R.TILE_M)
    rg_all = rg_all.to(cuda)
    rows_all = torch.arange(R.TILE_M, device=cuda)
    full = {}                                                      # (layout, act, bias?, group bias?) -> C of the first (128 x 128-tile) shape
    for (M, N, mode) in R.TILE_SHAPES:
        assert _tile_mode(M, N) == mode and M % 64 != 0
        A, W, zs, azs = a[:M], w[:N].contiguous(), z[:M, :N], absz[:M, :N]
        layouts = [("ragged", rg_all[:M].contiguous(), int(rg_all[M - 1]) + 2, None)]
        layouts += [(f"rpg{r}", (rows_all[:M] // r).int(), -(-M // r), r) for r in R.UNIFORM_RPG]
        for (lname, groups, ng, rpg) in layouts:
            for act in R.ACTS:
                for hb in (True, False):
                    for hg in (True, False):
                        bias = bias_all[:N].contiguous() if hb else None
                        gb = gb_all[:ng, :N].contiguous() if hg else None
                        ref, bound = R.expected(zs, azs, K, bias, gb, groups, act)
                        name = f"K={K} {M}x{N} {lname} act={act} bias={hb} gb={hg}"
                        kw = dict(A=A, lda=K, W=W, ldw=K, bias=bias, gb=gb, M=M, N=N, K=K, act=act, n_groups=ng)
                        C = _check_instances(R, run, dict(kw, row_group=groups), ref, bound, groups, ng, M, N, name + " ragged entry")
                        if rpg is not None:
                            Cu = _check_instances(R, run, dict(kw, rpg=rpg), ref, bound, groups, ng, M, N, name + " uniform entry")
                            assert R.bits_equal(Cu, C), name + ": uniform and ragged entries differ"
                        key = (lname, act, hb, hg)
                        if (M, N) == (R.TILE_M, R.TILE_N):
                            full[key] = C
                        else:
                            assert R.bits_equal(C, full[key][:M, :N]), name + f": rows differ from the {R.TILE_M} x {R.TILE_N} launch (other tile shape)"


@pytest.mark.gpu
def test_hip_gemm_ragged_dev_row_count_on_device(cuda, hip_lib):
    """sv_gemm_bias_act_ragged_dev at capacity 16 384 with *m_dev = 1 .. 16 384 (the kernel picks the tile shape from the count: 64 x 64, 64 x 128 and
    128 x 128 all occur): the first *m_dev rows against float64 and bit-identical to sv_gemm_bias_act_ragged on exactly those rows and to the same rows
    of the full-capacity launch (another tile shape); rows past *m_dev keep the sentinel; group_max only sees the counted rows."""
    import dense_reference as R
    run = _Gemm(hip_lib, cuda)
    cap, N, K = R.MDEV_CAPACITY, R.MDEV_N, R.MDEV_K
    g = torch.Generator().manual_seed(21)
    a, w = torch.randn(cap, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    bias, gb_all = torch.randn(N, generator=g).to(cuda), torch.randn(cap + 2, N, generator=g).to(cuda)
    z, absz = (t.to(cuda) for t in R.products(a, w))
    a, w = a.to(cuda), w.to(cuda)
    rg, ng = R.ragged_groups(cap)
    rg = rg.to(cuda)
    gb = gb_all[:ng].contiguous()
    assert sorted({_tile_mode(m, N) for m in R.MDEV_ROWS}) == [0, 1, 2] and set(R.MDEV_ROWS) >= {1, 63, 64, 65, 3000, 16384}
    for act, hb, hg in [(R.ACT_LRELU, True, True), (R.ACT_RELU, False, True), (R.ACT_NONE, True, False), (R.ACT_RELU, False, False)]:
        b_, gb_ = (bias if hb else None), (gb if hg else None)
        ref, bound = R.expected(z, absz, K, b_, gb_, rg, act)
        kw = dict(A=a, lda=K, W=w, ldw=K, bias=b_, gb=gb_, N=N, K=K, act=act, n_groups=ng)
        whole = None
        for m in sorted(R.MDEV_ROWS, reverse=True):
            m_dev = torch.tensor([m], dtype=torch.int32, device=cuda)
            name = f"m_dev={m} act={act} bias={hb} gb={hg}"
            C = _check_instances(R, run, dict(kw, M=cap, row_group=rg, m_dev=m_dev), ref[:m], bound[:m], rg, ng, m, N, name + " dev")
            Ch = _check_instances(R, run, dict(kw, M=m, row_group=rg[:m].contiguous()), ref[:m], bound[:m], rg, ng, m, N, name + " host")
            assert R.bits_equal(C, Ch), name + ": device-count and host-count launches differ"
            whole = C if whole is None else whole
            assert R.bits_equal(C, whole[:m]), name + ": rows differ from the full-capacity launch"


@pytest.mark.gpu
def test_hip_gemm_leading_dimensions(cuda, hip_lib):
    """lda in {K + 4, K + 32}, ldw = K + 4, ldc = N + 3: the NaN padding of A and W never reaches a result, the padding columns of C keep the
    sentinel, and the result is bit-identical to the contiguous launch -- uniform, ragged and device-count entries."""
    import dense_reference as R
    run = _Gemm(hip_lib, cuda)
    g = torch.Generator().manual_seed(22)
    for (M, N, K) in R.LD_SHAPES:
        a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        bias = torch.randn(N, generator=g).to(cuda)
        z, absz = (t.to(cuda) for t in R.products(a, w))
        a, w = a.to(cuda), w.to(cuda)
        rg, ng = R.ragged_groups(M)
        rg = rg.to(cuda)
        gb = torch.randn(ng, N, generator=g).to(cuda)
        m_dev = torch.tensor([M - 37], dtype=torch.int32, device=cuda)
        for act in R.ACTS:
            ref, bound = R.expected(z, absz, K, bias, gb, rg, act)
            plain = _check_instances(R, run, dict(A=a, lda=K, W=w, ldw=K, bias=bias, gb=gb, M=M, N=N, K=K, act=act, n_groups=ng, row_group=rg), ref, bound, rg, ng,
                                     M, N, f"{M}x{N}x{K} contiguous act={act}")
            for lda in (K + 4, K + 32):
                ap, wp = R.pad_cols(a, lda), R.pad_cols(w, K + 4)
                kw = dict(A=ap, lda=lda, W=wp, ldw=K + 4, bias=bias, gb=gb, N=N, K=K, act=act, n_groups=ng, ldc=N + 3)
                name = f"{M}x{N}x{K} lda={lda} act={act}"
                C = _check_instances(R, run, dict(kw, M=M, row_group=rg), ref, bound, rg, ng, M, N, name + " ragged")
                assert R.bits_equal(C, plain), name + ": differs from the contiguous launch"
                Cd = _check_instances(R, run, dict(kw, M=M, row_group=rg, m_dev=m_dev), ref[:M - 37], bound[:M - 37], rg, ng, M - 37, N, name + " dev")
                assert R.bits_equal(Cd, plain[:M - 37]), name + ": device-count launch differs"
                ug = (torch.arange(M, device=cuda) // 100).int()
                ngu = -(-M // 100)
                refu, boundu = R.expected(z, absz, K, bias, gb[:ngu].contiguous(), ug, act)
                _check_instances(R, run, dict(kw, gb=gb[:ngu].contiguous(), n_groups=ngu, M=M, rpg=100), refu, boundu, ug, ngu, M, N, name + " uniform")


@pytest.mark.gpu
def test_hip_gemm_small_m_every_edge_vs_float64(cuda, hip_lib):
    """k_gemm_small_m<4> (K < 512) and <16>: M, N around the 16-wide MFMA tiles, K with and without a tail after the 4-step unrolled loop and with
    waves that get no k-step at all, lda / ldw / ldc larger than the widths (NaN padding, sentinel columns), bias or not, every activation."""
    import dense_reference as R
    run = _Gemm(hip_lib, cuda)
    g = torch.Generator().manual_seed(23)
    Mx, Nx = max(R.SMALL_MS), max(R.SMALL_NS)
    for K in R.SMALL_KS:
        a, w = torch.randn(Mx, K, generator=g), torch.randn(Nx, K, generator=g) / K ** 0.5
        bias_all = torch.randn(Nx, generator=g).to(cuda)
        z, absz = (t.to(cuda) for t in R.products(a, w))
        ap, wp = R.pad_cols(a.to(cuda), K + 4), R.pad_cols(w.to(cuda), K + 8)
        for M in R.SMALL_MS:
            for N in R.SMALL_NS:
                for hb in (True, False):
                    bias = bias_all[:N].contiguous() if hb else None
                    for act in R.ACTS:
                        ref, bound = R.expected(z[:M, :N], absz[:M, :N], K, bias, None, None, act)
                        C, _ = run(A=ap, lda=K + 4, W=wp, ldw=K + 8, bias=bias, gb=None, M=M, N=N, K=K, act=act, n_groups=0, want_max=False, ldc=N + 3)
                        R.assert_within(C[:, :N], ref, bound, f"small-M {M}x{N}x{K} act={act} bias={hb}")
                        assert bool((C[:, N:] == R.SENTINEL).all()), f"small-M {M}x{N}x{K}: wrote into the padding of C"


@pytest.mark.gpu
def test_hip_gemm_split_k_vs_float64_and_one_pass(cuda, hip_lib):
    """sv_gemm_bias_act_splitk where sv_gemm_splitk_splits >= 2 (M just above 64, N = 100, uneven last split, ldc > N, uniform group bias):
    reproducible bit for bit, within the bound of float64 and of the one-pass kernel."""
    import dense_reference as R
    from seevcn_amd import _lib
    run = _Gemm(hip_lib, cuda)
    g = torch.Generator().manual_seed(24)
    for (M, N, K, rpg) in R.SPLITK_SHAPES:
        splits = hip_lib.sv_gemm_splitk_splits(M, N, K)
        assert splits >= 2
        if K == 1040:
            assert splits == 4                                     # chunks of 272, 272, 272 and 224
        a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        bias, gb = torch.randn(N, generator=g).to(cuda), torch.randn(-(-M // rpg), N, generator=g).to(cuda)
        z, absz = (t.to(cuda) for t in R.products(a, w))
        a, w = a.to(cuda), w.to(cuda)
        groups = torch.arange(M, device=cuda) // rpg
        sc = torch.empty(hip_lib.sv_gemm_splitk_scratch_bytes(M, N, K), dtype=torch.uint8, device=cuda)
        for act in R.ACTS:
            for hb, hg in ((True, True), (False, True), (True, False), (False, False)):
                b_, gb_ = (bias if hb else None), (gb if hg else None)
                ref, bound = R.expected(z, absz, K, b_, gb_, groups, act)
                outs = []
                for _ in range(2):
                    C = torch.full((M, N + 3), R.SENTINEL, device=cuda)
                    sc.fill_(0xFF)                                 # NaN bit patterns: every partial sum that is read must have been written first
                    _lib.check(hip_lib.sv_gemm_bias_act_splitk(a.data_ptr(), K, w.data_ptr(), K, None if b_ is None else b_.data_ptr(),
                                                               None if gb_ is None else gb_.data_ptr(), rpg, C.data_ptr(), N + 3, M, N, K, act, R.SLOPE,
                                                               sc.data_ptr(), _lib.stream()), "sv_gemm_bias_act_splitk")
                    outs.append(C)
                name = f"split-K {M}x{N}x{K} act={act} bias={hb} gb={hg}"
                assert R.bits_equal(outs[0], outs[1]), name + ": two launches differ"
                assert bool((outs[0][:, N:] == R.SENTINEL).all()), name + ": wrote into the padding of C"
                R.assert_within(outs[0][:, :N], ref, bound, name + " vs float64")
                one, _ = run(A=a, lda=K, W=w, ldw=K, bias=b_, gb=gb_, M=M, N=N, K=K, act=act, rpg=rpg, n_groups=0, want_max=False)
                R.assert_within(one, ref, bound, name + " one-pass vs float64")
                R.assert_within(outs[0][:, :N], one.double(), bound, name + " vs one-pass")


@pytest.mark.gpu
def test_hip_pointwise_conv3_and_gather_vs_float64(cuda, hip_lib):
    """sv_pointwise_conv3 / sv_pointwise_conv3_gather (the K = 3 first layers): C in {4, 128}, bias or not, every activation, against float64 at the
    bound with 3 in place of K; the gather form on a permuted `sel` with repeats and *m_dev below the capacity, rows past it keep the sentinel."""
    import dense_reference as R
    from seevcn_amd import _lib
    g = torch.Generator().manual_seed(25)
    P, cap, m = 1500, 2048, 1777
    xyz = (torch.randn(P, 3, generator=g) * 5).to(cuda)
    sel = torch.randint(0, P, (cap,), generator=g).to(cuda)
    sel[:P // 2] = torch.randperm(P, generator=g)[:P // 2].to(cuda)
    sel[100:110] = sel[99]                                                       # a run of repeats
    m_dev = torch.tensor([m], dtype=torch.int32, device=cuda)
    for C in (4, 128):
        w, b = torch.randn(C, 3, generator=g).to(cuda), torch.randn(C, generator=g).to(cuda)
        z, absz = R.products(xyz, w)
        for bias in (b, None):
            for act in R.ACTS:
                ref, bound = R.expected(z, absz, 3, bias, None, None, act)
                for M in (P, 1):
                    out = torch.full((M, C), R.SENTINEL, device=cuda)
                    _lib.check(hip_lib.sv_pointwise_conv3(xyz.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(), M, C, act,
                                                          R.SLOPE, _lib.stream()), "sv_pointwise_conv3")
                    R.assert_within(out, ref[:M], bound[:M], f"pointwise3 M={M} C={C} act={act} bias={bias is not None}")
                out = torch.full((cap, C), R.SENTINEL, device=cuda)
                _lib.check(hip_lib.sv_pointwise_conv3_gather(xyz.data_ptr(), sel.data_ptr(), cap, m_dev.data_ptr(), w.data_ptr(),
                                                             None if bias is None else bias.data_ptr(), out.data_ptr(), C, act, R.SLOPE, _lib.stream()),
                           "sv_pointwise_conv3_gather")
                R.assert_within(out[:m], ref[sel[:m]], bound[sel[:m]], f"pointwise3 gather C={C} act={act} bias={bias is not None}")
                assert bool((out[m:] == R.SENTINEL).all()), "pointwise3 gather wrote past *m_dev"


@pytest.mark.gpu
def test_hip_unique_rows_and_compact_vs_numpy(cuda, hip_lib):
    """sv_unique_rows + sv_unique_rows_compact against numpy.unique on six clouds: three tiled by ResamplePoints, an all-zero cloud, 1024 distinct rows
    and one with -0.0 / +0.0 coordinates.  The kernel compares coordinates with ==, so -0.0 equals +0.0 and such rows count as ONE distinct row
    (numpy.unique does the same); which of the copies is kept is not specified, so rows are compared as values."""
    from seevcn_amd.vcn.datasets.data_transforms import ResamplePoints
    from seevcn_amd.vcn.models import layers as L
    rng = np.random.default_rng(5)
    np.random.seed(11)
    clouds = [ResamplePoints({"n_points": 1024})(rng.normal(size=(ni, 3)).astype(np.float32) * 3) for ni in (30, 231, 1000)]
    clouds.append(np.zeros((1024, 3), np.float32))
    clouds.append(rng.normal(size=(1024, 3)).astype(np.float32))
    signed = rng.integers(-1, 2, size=(1024, 3)).astype(np.float32)               # coordinates in {-1, 0, 1}: at most 27 distinct rows
    signed[rng.random((1024, 3)) < 0.5] *= -1.0                                   # half of the zeros become -0.0
    assert np.signbit(signed[signed == 0]).any() and not np.signbit(signed[signed == 0]).all()
    clouds.append(signed)
    x_np = np.stack(clouds).astype(np.float32)
    x = torch.from_numpy(x_np).to(cuda)
    sel, rg = L.distinct_rows(x)
    sel_cap, rg_cap, total = L.distinct_rows(x, sync=False)
    assert int(total) == sel.shape[0] and torch.equal(sel_cap[:len(sel)], sel) and torch.equal(rg_cap[:len(sel)], rg)
    sel, rg = sel.cpu().numpy(), rg.cpu().numpy()
    assert (np.diff(rg) >= 0).all() and rg.min() == 0 and rg.max() == len(clouds) - 1
    flat = x_np.reshape(-1, 3)
    for b in range(len(clouds)):
        mine = sel[rg == b]
        assert ((mine >= b * 1024) & (mine < (b + 1) * 1024)).all()
        want = np.unique(x_np[b] + 0.0, axis=0)                                   # + 0.0 turns -0.0 into +0.0: one canonical copy of each value
        got = flat[mine] + 0.0
        assert len(got) == len(want), (b, len(got), len(want))
        assert np.array_equal(np.unique(got, axis=0), want), b                    # same set, and no row twice (the counts agree)
    counts = np.bincount(rg, minlength=len(clouds)).tolist()
    assert counts == [len(np.unique(c + 0.0, axis=0)) for c in x_np]
    assert counts[:2] == [30, 231] and 512 <= counts[2] <= 1000 and counts[3:5] == [1, 1024] and counts[5] <= 27
