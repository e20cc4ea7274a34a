"""Eval-mode sparse backbones as one launch list with folded BatchNorm (seevcn_amd/spconv/chain.py: flatten / eval_applicable / run_eval_chain),
the one-launch eval coefficients (sv_batchnorm_eval_coef_batch) and the whole-row store path of the planned conv kernel's epilogue.  The module path
(SEEVCN_EVAL_CHAIN=0) is the bitwise reference of the chain, the float64 oracle (oracle/spconv.py) the reference of both."""
import re
import struct
from functools import partial

import numpy as np
import pytest
import torch

from oracle import spconv as osp
from seeding import seeded_state_dict
from tolerances import assert_close_per_channel
from test_spconv import EPILOGUES, KITTI_GEOMETRY, _epilogue_kwargs, _epilogue_ref, _epilogue_terms, _ok

STAGES = ("conv_input", "conv1", "conv2", "conv3", "conv4", "conv_out")
TAPS = ("x_conv1", "x_conv2", "x_conv3", "x_conv4")


def _backbone(name, channels=3, grid=KITTI_GEOMETRY[2]):
    from seevcn_amd.pcdet.models import backbones_3d
    return backbones_3d.__all__[name]({}, channels, grid)


# ---------------------------------------------------------------------------------- 1. symbol + flattening (no GPU)
def test_eval_coef_batch_is_declared_exported_and_bound(hip_lib):
    import ctypes
    import os
    from seevcn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "seevcn_hip.h")).read()
    assert re.search(r"\bint\s+sv_batchnorm_eval_coef_batch\s*\(\s*const\s+int64_t\s*\*\s*jobs_host\s*,\s*int\s+n_jobs\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"#define\s+SV_OP_BN_EVAL_COEF_BATCH\s+15\b", header)
    assert _lib.SIGNATURES["sv_batchnorm_eval_coef_batch"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
    fn = hip_lib.sv_batchnorm_eval_coef_batch                                       # exported by the built library (ctypes resolves the symbol here)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 3
    assert hip_lib.sv_batchnorm_eval_coef_batch(None, 0, None) == 0                 # no jobs: nothing is launched, no device is touched


def test_flatten_of_both_backbones():
    """12 / 21 entries, every one with a ReLU; the identity of a residual block is the entry in front of the block; taps behind conv1..conv4 and conv_out."""
    from seevcn_amd.spconv import chain
    from seevcn_amd.spconv.conv import SparseConvolution
    m = _backbone("VoxelBackBone8x")
    e = m._chain_blocks()
    assert len(e) == 12 and all(x.relu for x in e) and all(x.residual_from is None for x in e)
    assert [k for k, x in enumerate(e) if x.tap] == [1, 4, 7, 10, 11]
    assert [x.conv for x in e] == [mod for mod in m.modules() if isinstance(mod, SparseConvolution)]          # execution order = definition order
    conv, bn, relu, residual_from, tap = e[0]                                       # an entry unpacks as the five fields
    assert conv is m.conv_input[0] and bn is m.conv_input[1] and relu is True and residual_from is None and tap is False
    # flatten itself: the last entry of EVERY stage is a tap (the backbone clears conv_input's)
    raw = chain.flatten([getattr(m, s) for s in STAGES])
    assert [k for k, x in enumerate(raw) if x.tap] == [0, 1, 4, 7, 10, 11]
    # the training chain reads the same list: no residual identity in it, plain or after convert_sync_batchnorm (chain.applicable declines one that has)
    s = torch.nn.SyncBatchNorm.convert_sync_batchnorm(_backbone("VoxelBackBone8x"))
    es = s._chain_blocks()
    assert len(es) == 12 and all(x.residual_from is None for x in es) and all(type(x.bn) is torch.nn.SyncBatchNorm for x in es)
    assert [k for k, x in enumerate(es) if x.tap] == [1, 4, 7, 10, 11] and len(es.walked) == len(e.walked)
    assert isinstance(e[0].mom_eps, tuple) and e[0].mom_eps == (chain._bits(0.01), chain._bits(1e-3))

    r = _backbone("VoxelResBackBone8x", 5, [1440, 1440, 40])
    e = r._chain_blocks()
    assert len(e) == 21 and all(x.relu for x in e)
    want_res = {2: 0, 4: 2, 7: 5, 9: 7, 12: 10, 14: 12, 17: 15, 19: 17}              # conv2 of every block <- the entry in front of its conv1
    assert {k: x.residual_from for k, x in enumerate(e) if x.residual_from is not None} == want_res
    assert [k for k, x in enumerate(e) if x.tap] == [4, 9, 14, 19, 20]
    blk = r.conv1[0]
    assert e[1].conv is blk.conv1 and e[1].bn is blk.bn1 and e[2].conv is blk.conv2 and e[2].bn is blk.bn2 and e[2].conv.bias is not None
    for x in e:
        assert x.cin == x.conv.in_channels and x.cout == x.conv.out_channels and x.bn.num_features == x.cout
    assert set(e.walked) >= {r.conv1, blk, blk.conv1, blk.bn1, blk.relu, blk.conv2, blk.bn2, r.conv_out[0]}
    # a chain whose first module is a residual block reads the chain's input as the identity
    first = chain.flatten([r.conv1])
    assert [x.residual_from for x in first] == [None, -1, None, 1] and first[-1].tap


def test_flatten_declines_what_it_cannot_fold():
    import seevcn_amd.spconv as spconv
    from seevcn_amd.pcdet.models.backbones_3d.spconv_backbone import SparseBasicBlock
    from seevcn_amd.spconv import chain
    norm_fn = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    down = spconv.SparseSequential(spconv.SubMConv3d(16, 16, 1, bias=False, indice_key="d"), norm_fn(16))
    assert chain.flatten([spconv.SparseSequential(SparseBasicBlock(16, 16, norm_fn=norm_fn, downsample=down, indice_key="r"))]) is None

    class OwnForward(SparseBasicBlock):
        def forward(self, x):
            return super().forward(x)

    class SameForward(SparseBasicBlock):
        pass

    assert chain.flatten([spconv.SparseSequential(OwnForward(16, 16, norm_fn=norm_fn, indice_key="r"))]) is None
    assert len(chain.flatten([spconv.SparseSequential(SameForward(16, 16, norm_fn=norm_fn, indice_key="r"))])) == 2
    # conv -> norm without the ReLU, a GroupNorm, a bare ReLU, something that is no SparseSequential
    conv = lambda: spconv.SubMConv3d(16, 16, 3, bias=True, indice_key="s")
    assert chain.flatten([spconv.SparseSequential(conv(), norm_fn(16))]) is None
    assert chain.flatten([spconv.SparseSequential(conv(), torch.nn.GroupNorm(4, 16), torch.nn.ReLU())]) is None
    assert chain.flatten([spconv.SparseSequential(torch.nn.ReLU())]) is None
    assert chain.flatten([torch.nn.Sequential()]) is None and chain.flatten([spconv.SparseSequential()]) is None
    ok = chain.flatten([spconv.SparseSequential(conv(), norm_fn(16), torch.nn.ReLU())])              # a conv bias is taken
    assert len(ok) == 1 and ok[0].conv.bias is not None and ok[0].tap
    # the backbone re-flattens when a module is assigned (registration epoch): a downsample set later sends it to the module tree
    r = _backbone("VoxelResBackBone8x")
    assert len(r._chain_blocks()) == 21
    r.conv3[1].downsample = down
    assert r._chain_blocks() is None
    r.conv3[1].downsample = None
    assert len(r._chain_blocks()) == 21
    # ... and the cleared slot stays registered as None in the block's _modules: it is not among the modules whose hooks are looked at
    assert "downsample" in r.conv3[1]._modules and None not in r._chain_blocks().walked
    assert not any(chain._has_hooks(mod) for mod in r._chain_blocks().walked)


# ---------------------------------------------------------------------------------- 2. coefficients
def _bits(x):
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


@pytest.mark.gpu
def test_hip_eval_coef_batch_vs_float64(cuda, hip_lib):
    """Eight layers (C in 16, 32, 64, 128, each with and without affine parameters, different eps) in ONE call.  The kernel is a handful of correctly
    rounded fp32 operations: |scale - ref| <= 4 * 2^-24 * |ref|, |shift - ref| <= 4 * 2^-24 * (|b| + |mean * scale|) (derived, not tuned)."""
    from seevcn_amd import _lib
    from seevcn_amd.spconv import chain
    rng = np.random.default_rng(17)
    layers, total = [], 0
    for q, (c, affine) in enumerate([(c, a) for c in (16, 32, 64, 128) for a in (True, False)]):
        h = {"g": rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c), "b": rng.normal(size=c), "mean": rng.normal(size=c) * 2.0, "var": rng.uniform(0.05, 4.0, c)}
        h = {k: v.astype(np.float32) for k, v in h.items()}
        layers.append((c, affine, (1e-3, 1e-5)[q % 2], h, {k: torch.from_numpy(v).to(cuda) for k, v in h.items()}, total))
        total += 2 * c
    u = 2.0 ** -24
    outs = []
    for via_list in (False, True):
        out = torch.full((total,), float("nan"), dtype=torch.float32, device=cuda)
        jobs = np.zeros((len(layers), 8), dtype=np.int64)
        for q, (c, affine, eps, h, d, off) in enumerate(layers):
            jobs[q, :7] = (d["g"].data_ptr() if affine else 0, d["b"].data_ptr() if affine else 0, d["mean"].data_ptr(), d["var"].data_ptr(),
                           out.data_ptr() + 4 * off, c, _bits(eps))
        if via_list:
            chain._run([chain._row(chain.OP_BN_EVAL_COEF_BATCH, i=(len(layers),), p=(jobs.ctypes.data,))], "SV_OP_BN_EVAL_COEF_BATCH")
        else:
            _lib.check(hip_lib.sv_batchnorm_eval_coef_batch(jobs.ctypes.data, len(layers), _lib.stream()), "sv_batchnorm_eval_coef_batch")
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])                                         # the launch-list form is the same call
    got = outs[0]
    assert np.isfinite(got).all()                                                   # every slot of every layer was written
    worst = [0.0, 0.0]
    for c, affine, eps, h, d, off in layers:
        g = h["g"].astype(np.float64) if affine else np.ones(c)
        b = h["b"].astype(np.float64) if affine else np.zeros(c)
        scale = g / np.sqrt(h["var"].astype(np.float64) + np.float64(np.float32(eps)))
        shift = b - h["mean"].astype(np.float64) * scale
        e_scale = np.abs(got[off:off + c] - scale) / (u * np.abs(scale))
        e_shift = np.abs(got[off + c:off + 2 * c] - shift) / (u * (np.abs(b) + np.abs(h["mean"].astype(np.float64) * scale)))
        worst = [max(worst[0], float(e_scale.max())), max(worst[1], float(e_shift.max()))]
        print(f"eval coefficients C {c} affine {affine}: scale error {e_scale.max():.2f} u, shift error {e_shift.max():.2f} u (bound 4 u)")
        assert (e_scale <= 4.0).all() and (e_shift <= 4.0).all(), (c, affine, float(e_scale.max()), float(e_shift.max()))
    # more jobs than one launch carries in its argument block (64): 70 jobs over the eight layers above give each layer's bits again
    n_many = 70
    slots = [layers[q % len(layers)] for q in range(n_many)]
    offs = np.concatenate([[0], np.cumsum([2 * l[0] for l in slots])])
    many = torch.full((int(offs[-1]),), float("nan"), dtype=torch.float32, device=cuda)
    jobs = np.zeros((n_many, 8), dtype=np.int64)
    for q, (c, affine, eps, h, d, off) in enumerate(slots):
        jobs[q, :7] = (d["g"].data_ptr() if affine else 0, d["b"].data_ptr() if affine else 0, d["mean"].data_ptr(), d["var"].data_ptr(),
                       many.data_ptr() + 4 * int(offs[q]), c, _bits(eps))
    _lib.check(hip_lib.sv_batchnorm_eval_coef_batch(jobs.ctypes.data, n_many, _lib.stream()), "sv_batchnorm_eval_coef_batch (70 jobs)")
    many_h = many.cpu().numpy()
    for q, (c, affine, eps, h, d, off) in enumerate(slots):
        assert np.array_equal(many_h[offs[q]:offs[q + 1]], got[off:off + 2 * c]), q
    # argument errors: every job is checked before the first launch, so a bad job behind the first 64 leaves the outputs of all jobs untouched
    bad = np.zeros((1, 8), dtype=np.int64)
    assert hip_lib.sv_batchnorm_eval_coef_batch(bad.ctypes.data, 1, None) == 1 and b"null pointer" in hip_lib.sv_last_error()
    many.fill_(float("nan"))
    jobs[n_many - 1, 3] = 0
    assert hip_lib.sv_batchnorm_eval_coef_batch(jobs.ctypes.data, n_many, _lib.stream()) == 1 and b"job 69: null pointer" in hip_lib.sv_last_error()
    assert bool(torch.isnan(many).all())


# ---------------------------------------------------------------------------------- 3./4. the backbones: chain vs module path vs float64
class _Spy:
    """Counts the sv_run_ops calls (and their list lengths) of the library object while it is installed."""

    def __init__(self, monkeypatch, lib):
        self.calls, real = [], lib.sv_run_ops

        def spy(ops, n_ops, stream):
            self.calls.append(int(n_ops))
            return real(ops, n_ops, stream)

        monkeypatch.setattr(lib, "sv_run_ops", spy, raising=False)


def _kitti_batch(cuda, n_scenes=2, n_az=100, seed=2000):
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.models.backbones_3d import vfe
    pts, _ = synth.make_scene_batch(n_scenes, seed=seed, n_az=n_az)
    pc_range, vs, grid = KITTI_GEOMETRY
    bd = {"batch_size": n_scenes, "points": torch.from_numpy(pts).to(cuda)}
    return vfe.__all__["DynMeanVFE"](model_cfg={}, num_point_features=3, voxel_size=vs, grid_size=grid, point_cloud_range=pc_range)(bd)


def _run_backbone(m, bd, monkeypatch, on, grad=False):
    """-> ({tap name: SparseConvTensor}, sv_run_ops list lengths): one forward on a copy of bd with the eval chain on / off."""
    from seevcn_amd import _lib
    from seevcn_amd.spconv import chain
    with monkeypatch.context() as mp:
        mp.setattr(chain, "EVAL_CHAIN_OFF", not on)
        spy = _Spy(mp, _lib.load())
        with (torch.enable_grad() if grad else torch.no_grad()):
            out = m(dict(bd))
    taps = dict(out["multi_scale_3d_features"])
    taps["out"] = out["encoded_spconv_tensor"]
    assert out["encoded_spconv_tensor_stride"] == 8 and out["multi_scale_3d_strides"] == {"x_conv1": 1, "x_conv2": 2, "x_conv3": 4, "x_conv4": 8}
    return taps, spy.calls


def _assert_same_taps(a, b, what):
    assert set(a) == set(b) == set(TAPS) | {"out"}
    for name in a:
        assert list(a[name].spatial_shape) == list(b[name].spatial_shape), (what, name)
        assert torch.equal(a[name].indices, b[name].indices), (what, name)
        assert a[name].features.shape == b[name].features.shape and torch.equal(a[name].features, b[name].features), \
            (what, name, float((a[name].features - b[name].features).abs().max()))


def _assert_taps_vs_oracle(taps, ref, what):
    for name, t in taps.items():
        f, c, shape = ref[name]
        assert list(t.spatial_shape) == list(shape) and np.array_equal(t.indices.cpu().numpy(), c), (what, name)
        assert_close_per_channel(t.features.cpu().numpy(), f, name=f"{what} {name}")


def _state_snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _assert_state_untouched(m, before):
    after = m.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_convs,oracle", [("VoxelBackBone8x", 12, "voxel_backbone8x_forward"), ("VoxelResBackBone8x", 21, "voxel_res_backbone8x_forward")])
def test_hip_eval_chain_vs_module_path_vs_float64(cuda, hip_lib, monkeypatch, name, n_convs, oracle):
    """2 scenes on the KITTI geometry, seeded weights and running statistics, under no_grad: the forward is ONE sv_run_ops call of (sparse convs + 1)
    operations; its taps equal the module path's bit for bit (the same kernels' accumulators, then bias add, one fma, residual add, max in the same
    order) and both meet the float64 oracle at the project's 1e-3 contract; nothing of the model is written."""
    bd = _kitti_batch(cuda)
    m = _backbone(name)
    sd = seeded_state_dict(m, seed=1)
    m.load_state_dict(sd)
    m = m.to(cuda).eval()
    before = _state_snapshot(m)
    assert sum(1 for _ in m._chain_blocks()) == n_convs
    chain_taps, calls = _run_backbone(m, bd, monkeypatch, on=True)
    assert calls == [n_convs + 1], calls                                            # the test that fails without the feature
    module_taps, calls_off = _run_backbone(m, bd, monkeypatch, on=False)
    assert calls_off == [], calls_off
    _assert_same_taps(chain_taps, module_taps, name)
    ref = getattr(osp, oracle)({k: v.numpy() for k, v in sd.items()}, bd["voxel_features"].cpu().numpy(), bd["voxel_coords"].cpu().numpy(), 2, m.sparse_shape)
    if name == "VoxelResBackBone8x":
        for tap in TAPS + ("out",):                                                 # a wrong epilogue order must not hide behind the ReLU
            assert (ref[tap][0] == 0).mean() > 0.05 and (ref[tap][0] > 0).mean() > 0.05, tap
    _assert_taps_vs_oracle(chain_taps, ref, f"{name} eval chain")
    _assert_taps_vs_oracle(module_taps, ref, f"{name} module path")
    _assert_state_untouched(m, before)
    assert all(not t.features.requires_grad and t.features.grad_fn is None for t in chain_taps.values())
    # a second forward gives the same bits (nothing carried over between forwards)
    again, calls = _run_backbone(m, bd, monkeypatch, on=True)
    assert calls == [n_convs + 1]
    _assert_same_taps(again, chain_taps, name + " repeated")


# ---------------------------------------------------------------------------------- 5. freshness
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["VoxelBackBone8x", "VoxelResBackBone8x"])
def test_hip_eval_chain_follows_the_live_buffers(cuda, hip_lib, monkeypatch, name):
    """No coefficient outlives a forward: load_state_dict of other weights and running statistics, then a train() step and back to eval(), each
    followed by a chain forward that equals the module path on the model's current state bit for bit."""
    bd = _kitti_batch(cuda, n_az=90)
    m = _backbone(name)
    m.load_state_dict(seeded_state_dict(m, seed=1))
    m = m.to(cuda).eval()
    first, calls = _run_backbone(m, bd, monkeypatch, on=True)
    assert len(calls) == 1
    sd2 = seeded_state_dict(m, seed=2)
    m.load_state_dict(sd2)
    fresh = _backbone(name)
    fresh.load_state_dict(sd2)
    fresh = fresh.to(cuda).eval()
    second, calls = _run_backbone(m, bd, monkeypatch, on=True)
    want, none = _run_backbone(fresh, bd, monkeypatch, on=False)
    assert len(calls) == 1 and none == []
    _assert_same_taps(second, want, name + " after load_state_dict")
    assert not torch.equal(second["out"].features, first["out"].features)
    # one training step: the running statistics and (after the optimiser) the weights move
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    out = m(dict(bd))
    out["encoded_spconv_tensor"].features.square().mean().backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    m.eval()
    assert not torch.equal(m.conv_out[1].running_mean, fresh.conv_out[1].running_mean)
    third, calls = _run_backbone(m, bd, monkeypatch, on=True)
    want, none = _run_backbone(m, bd, monkeypatch, on=False)
    assert len(calls) == 1 and none == []
    _assert_same_taps(third, want, name + " after a training step")
    assert not torch.equal(third["out"].features, second["out"].features)


# ---------------------------------------------------------------------------------- 6. standing down
@pytest.mark.gpu
def test_hip_eval_chain_stands_down(cuda, hip_lib, monkeypatch):
    """A hook, enabled gradients, a BatchNorm in train(), an empty input, a downsample module, a block with a forward of its own, SEEVCN_CHAIN=0: each
    takes the module path (no launch list is run in eval mode) and gives the module path's result."""
    import seevcn_amd.spconv as spconv
    from seevcn_amd.pcdet.models.backbones_3d.spconv_backbone import SparseBasicBlock
    from seevcn_amd.spconv import chain
    bd = _kitti_batch(cuda, n_az=90)

    def build(name="VoxelResBackBone8x"):
        m = _backbone(name)
        m.load_state_dict(seeded_state_dict(m, seed=1))
        return m.to(cuda).eval()

    m = build()
    base, calls = _run_backbone(m, bd, monkeypatch, on=True)
    assert calls == [22]
    want, _ = _run_backbone(m, bd, monkeypatch, on=False)
    _assert_same_taps(base, want, "baseline")

    # a forward hook on one conv (it must see the call)
    seen = []
    h = m.conv3[1].conv2.register_forward_hook(lambda mod, i, o: seen.append(o.features.shape))
    got, calls = _run_backbone(m, bd, monkeypatch, on=True)
    h.remove()
    assert calls == [] and len(seen) == 1
    _assert_same_taps(got, want, "forward hook")
    assert _run_backbone(m, bd, monkeypatch, on=True)[1] == [22]                    # hook removed: the chain is back

    # gradients enabled (a frozen-backbone fine-tune reads gradients through an eval-mode backbone)
    # -- the module path under the same condition: with a gradient to keep, its BatchNorms run as torch's own (seevcn_amd.spconv.norm.fusable)
    got, calls = _run_backbone(m, bd, monkeypatch, on=True, grad=True)
    ref, _ = _run_backbone(m, bd, monkeypatch, on=False, grad=True)
    assert calls == [] and got["out"].features.requires_grad and ref["out"].features.requires_grad
    detached = lambda taps: {k: spconv.SparseConvTensor(t.features.detach(), t.indices, t.spatial_shape, t.batch_size) for k, t in taps.items()}
    _assert_same_taps(detached(got), detached(ref), "grad enabled")
    for name, t in got.items():
        assert_close_per_channel(t.features.detach().cpu().numpy(), want[name].features.cpu().numpy().astype(np.float64), name=f"grad enabled {name}")

    # one BatchNorm left in train(): it normalises with batch statistics (and updates its running statistics) on both paths
    m2, m3 = build(), build()
    for mm in (m2, m3):
        mm.conv2[1].bn1.train()
    got, calls = _run_backbone(m2, bd, monkeypatch, on=True)
    ref, _ = _run_backbone(m3, bd, monkeypatch, on=False)
    assert calls == []
    _assert_same_taps(got, ref, "a norm in train mode")
    assert torch.equal(m2.conv2[1].bn1.running_mean, m3.conv2[1].bn1.running_mean) and int(m2.conv2[1].bn1.num_batches_tracked) == 1

    # an input with zero voxels
    empty = dict(bd)
    empty["voxel_features"], empty["voxel_coords"] = bd["voxel_features"][:0], bd["voxel_coords"][:0]
    got, calls = _run_backbone(m, empty, monkeypatch, on=True)
    ref, _ = _run_backbone(m, empty, monkeypatch, on=False)
    assert calls == [] and got["out"].features.shape[0] == 0
    _assert_same_taps(got, ref, "empty input")

    # a residual block with a downsample module
    norm_fn = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    m4 = build()
    down = spconv.SparseSequential(spconv.SubMConv3d(64, 64, 1, bias=False, indice_key="down3"), norm_fn(64)).to(cuda).eval()
    m4.conv3[1].downsample = down
    got, calls = _run_backbone(m4, bd, monkeypatch, on=True)
    ref, _ = _run_backbone(m4, bd, monkeypatch, on=False)
    assert calls == [] and m4._chain_blocks() is None
    _assert_same_taps(got, ref, "downsample")
    assert not torch.equal(got["x_conv3"].features, want["x_conv3"].features)       # the downsample branch took part

    # a subclass of the block with its own forward
    class Doubling(SparseBasicBlock):
        def forward(self, x):
            out = super().forward(x)
            return out.replace_feature(out.features * 2.0)

    m5 = build()
    blk = Doubling(64, 64, norm_fn=norm_fn, indice_key="res3")
    blk.load_state_dict(m5.conv3[2].state_dict())
    m5.conv3.add_module("2", blk.to(cuda).eval())
    got, calls = _run_backbone(m5, bd, monkeypatch, on=True)
    ref, _ = _run_backbone(m5, bd, monkeypatch, on=False)
    assert calls == [] and m5._chain_blocks() is None
    _assert_same_taps(got, ref, "own forward")
    assert torch.equal(got["x_conv3"].features, want["x_conv3"].features * 2.0)

    # the other way round: a downsample that was set and cleared again (torch keeps the slot registered as None) is no reason to stand down, and
    # must not trip the hook scan -- the chain runs and gives the module tree's bits
    m6 = build()
    m6.conv3[1].downsample = down
    m6.conv3[1].downsample = None
    assert "downsample" in m6.conv3[1]._modules and len(m6._chain_blocks()) == 21
    got, calls = _run_backbone(m6, bd, monkeypatch, on=True)
    ref, calls_off = _run_backbone(m6, bd, monkeypatch, on=False)
    assert calls == [22] and calls_off == []
    _assert_same_taps(got, ref, "downsample set and cleared")
    _assert_same_taps(got, want, "downsample set and cleared vs the untouched model")

    # SEEVCN_CHAIN=0
    monkeypatch.setattr(chain, "CHAIN_OFF", True)
    got, calls = _run_backbone(m, bd, monkeypatch, on=True)
    assert calls == []
    _assert_same_taps(got, want, "SEEVCN_CHAIN=0")


# ---------------------------------------------------------------------------------- 7. detectors
def _same_predictions(a, b, what):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert set(p) == set(q)
        for key in ("pred_boxes", "pred_scores", "pred_labels"):
            assert p[key].shape == q[key].shape and torch.equal(p[key], q[key]), (what, i, key)


def _detect(net, batch, monkeypatch, on):
    from seevcn_amd import _lib
    from seevcn_amd.spconv import chain
    with monkeypatch.context() as mp:
        mp.setattr(chain, "EVAL_CHAIN_OFF", not on)
        spy = _Spy(mp, _lib.load())
        np.random.seed(0)
        torch.manual_seed(0)
        with torch.no_grad():
            preds, recall = net(dict(batch))
    return preds, spy.calls


@pytest.mark.gpu
def test_hip_detectors_predict_the_same_with_the_eval_chain_on_and_off(cuda, hip_lib, monkeypatch):
    """SECONDNet, PV-RCNN (reads x_conv1..4 through multi_scale_3d_features: a mis-ordered tap would show) and CenterPoint in eval: boxes, scores and labels
    identical with the chain on and off."""
    import config_inputs as ci
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models import detectors
    from seevcn_amd.pcdet.ops import voxel_ops
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=100)
    batch = {"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda)}
    builds = [("SECONDNet", C.second_model_cfg(), 4, 13),
              ("PVRCNN", C.pvrcnn_model_cfg(num_keypoints=512, roi_per_image=32, nms_post_train=128, nms_pre_train=2048), 6, 13)]
    for name, cfg, seed, n_ops in builds:
        net = detectors.build_detector(cfg, num_class=3, dataset=C.SyntheticDatasetInfo())
        net.load_state_dict(seeded_state_dict(net, seed=seed))
        net = net.to(cuda).eval()
        on, calls = _detect(net, batch, monkeypatch, True)
        off, calls_off = _detect(net, batch, monkeypatch, False)
        assert calls == [n_ops] and calls_off == [], (name, calls, calls_off)
        assert len(on) == 2 and sum(len(p["pred_scores"]) for p in on) > 0, name
        _same_predictions(on, off, name)
        del net
    # CenterPoint on a small nuScenes-shaped scene (config-5 size is tests/test_configs.py's)
    pts, gt = ci.centerpoint_scene(n_az=240)
    pts = pts[np.random.default_rng(0).permutation(len(pts))]
    grid = np.round((np.array(ci.NUSC_RANGE[3:]) - np.array(ci.NUSC_RANGE[:3])) / np.array(ci.NUSC_VOXEL)).astype(np.int64)
    vox, crd, nmp, nv = voxel_ops.voxelize_hard(torch.from_numpy(pts).to(cuda), 0, 3, [len(pts)], ci.NUSC_RANGE, ci.NUSC_VOXEL, grid, 10, 120000)
    n = int(nv[0])
    coords = torch.cat([torch.zeros((n, 1), dtype=torch.int32, device=cuda), crd[0, :n]], dim=1)
    ds = C.SyntheticDatasetInfo(class_names=C.NUSC_CLASS_NAMES, point_cloud_range=ci.NUSC_RANGE, voxel_size=ci.NUSC_VOXEL, num_point_features=3)
    net = detectors.build_detector(C.centerpoint_model_cfg(), num_class=10, dataset=ds)
    net.load_state_dict(seeded_state_dict(net, seed=21))
    net = net.to(cuda).eval()
    gt10 = np.concatenate([gt[:, :7], np.zeros((len(gt), 2), np.float32), gt[:, 7:8]], axis=1)[None]
    batch = {"batch_size": 1, "voxels": vox[0, :n].contiguous(), "voxel_coords": coords, "voxel_num_points": nmp[0, :n].contiguous(),
             "gt_boxes": torch.from_numpy(gt10).to(cuda)}
    on, calls = _detect(net, batch, monkeypatch, True)
    off, calls_off = _detect(net, batch, monkeypatch, False)
    assert calls == [22] and calls_off == [], (calls, calls_off)
    assert len(on) == 1 and on[0]["pred_boxes"].shape[1] >= 7
    _same_predictions(on, off, "CenterPoint")


# ---------------------------------------------------------------------------------- 8. the store path at the size the product runs
@pytest.mark.gpu
def test_hip_epilogue_on_whole_rows_at_16_scenes(cuda, hip_lib):
    """All epilogue terms on the 64 -> 64 submanifold table (subm3) of a 16-scene KITTI-shaped batch: two tiles per wave go through the staging tile.
    Against float64, bit-equal to the plain entry (k_spconv_rs, per-accumulator conv_epilogue), and bit-equal with residual / bias / scale at
    addresses that are not 16-byte aligned (the launch then stores per accumulator).
    What this cannot see: WHICH of the two store forms a launch took -- they give the same bits by design, so a launch that wrongly chose the other
    form passes here.  The only witness of the form is its time (tools/spconv_micro.py --epilogue against SEEVCN_RS3_EPI_ROWS=0)."""
    import seevcn_amd.spconv as spconv
    from seevcn_amd.spconv import functional as Fsp
    bd = _kitti_batch(cuda, n_scenes=16, n_az=384)
    m = _backbone("VoxelBackBone8x").to(cuda).eval()
    x = spconv.SparseConvTensor(bd["voxel_features"], bd["voxel_coords"].int(), m.sparse_shape, 16)
    spconv.prebuild_rulebooks(m, x, with_backward=False)
    rb = x.indice_dict["subm3"]
    assert rb.subm and rb.n_in == rb.n_out and rb.n_out > 80_000, rb.n_out
    plan = rb.plan("fwd", 64, 64)
    assert plan is not None and plan[2] == hip_lib.sv_conv_tiles_per_wave(rb.n_out, 64, 64) == 2
    rng = np.random.default_rng(64)
    K = 27
    xh = rng.normal(size=(rb.n_in, 64)).astype(np.float32)
    wh = (rng.normal(size=(K, 64, 64)) * 1.5 / np.sqrt(0.4 * K * 64)).astype(np.float32)
    xd, wd = torch.from_numpy(xh).to(cuda), torch.from_numpy(wh).to(cuda)
    nbr = rb.nbr_out.cpu().numpy()
    conv64 = osp.conv_forward(xh, nbr, wh)
    t, dev = _epilogue_terms(rng, rb.n_out, 64, cuda)
    ff, _ = Fsp.fragment_cache.get(wd)
    wt = wd.permute(0, 2, 1).contiguous()
    for name in ("scale+shift+relu", "all"):
        kw = _epilogue_kwargs(dev, EPILOGUES[name])
        y = Fsp.gather_gemm_planned(xd, plan, ff, rb.n_out, K, 64, 64, **kw)
        assert _ok(y.cpu().numpy(), _epilogue_ref(conv64, t, EPILOGUES[name]), name=f"planned 64->64 at 16 scenes, epilogue {name}")
        assert torch.equal(y, Fsp.gather_gemm(xd, rb.nbr_out, wt, rb.n_out, **kw)), name
    # the same terms one float off 16-byte alignment: per-accumulator stores, the same bits
    off = {}
    for k, v in dev.items():
        buf = torch.empty((v.numel() + 4,), dtype=torch.float32, device=cuda)
        off[k] = buf[1:1 + v.numel()].view(v.shape)
        off[k].copy_(v)
        assert off[k].data_ptr() % 16 == 4
    assert torch.equal(Fsp.gather_gemm_planned(xd, plan, ff, rb.n_out, K, 64, 64, **_epilogue_kwargs(off, EPILOGUES["all"])), y)
