"""Voxel R-CNN's voxel RoI pooling: the dense cell -> row volume, the voxel query (bit-exact), the fused eval tail and the module tree of
NeighborVoxelSAModuleMSG against the CPU restatement in tests/voxel_pool_reference.py, and the registries / state_dict of the head and detector."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import voxel_pool_reference as R
from seeding import seeded_state_dict
from seevcn_amd.pcdet import model_cfgs as C

SHAPE = (5, 12, 9)                      # (Z, Y, X): no power of two, Z smaller than a range-4 window (clipped on both sides at once)
VOXEL = np.array([0.1, 0.1, 0.2], np.float32)                 # x, y, z
# (range, radius, nsample)
CASES = [([4, 4, 4], 0.4, 16), ([1, 2, 3], 0.25, 4), ([0, 0, 0], 1.0, 1), ([2, 2, 2], 10.0, 32), ([4, 4, 4], 0.12, 16)]
SEED = 31


@functools.lru_cache(maxsize=None)
def _scene(per_scene=160):
    """B = 2 scenes on SHAPE, about 35 % of the cells occupied, each scene's rows in a seeded random order; per_scene queries a scene drawn from
    the volume's box grown by 1.5 voxels a side, every 40th moved 3 m away."""
    rng = np.random.default_rng(SEED)
    Z, Y, X = SHAPE
    rows = []
    for b in range(2):
        occ = np.argwhere(rng.uniform(size=SHAPE) < 0.35)
        occ = occ[rng.permutation(len(occ))]
        rows.append(np.concatenate([np.full((len(occ), 1), b), occ], 1))
    indices = np.concatenate(rows).astype(np.int32)                                    # (N, 4) [b, z, y, x]
    xyz = ((indices[:, [3, 2, 1]].astype(np.float32) + np.float32(0.5)) * VOXEL).astype(np.float32)
    hi = np.array([X, Y, Z], np.float32) * VOXEL
    counts = [per_scene, per_scene] if isinstance(per_scene, int) else list(per_scene)
    new_xyz, bcol = [], []
    for b, n in enumerate(counts):
        q = rng.uniform(-1.5 * VOXEL, hi + 1.5 * VOXEL, size=(n, 3)).astype(np.float32)
        q[::40] += np.float32(3.0)
        new_xyz.append(q)
        bcol.append(np.full((n, 1), b, np.int32))
    new_xyz = np.concatenate(new_xyz)
    cell = np.floor(new_xyz / VOXEL).astype(np.int32)                                  # [x, y, z], negatives included
    new_coords = np.concatenate([np.concatenate(bcol), cell[:, [2, 1, 0]]], 1).astype(np.int32)   # [b, z, y, x]
    vol = R.voxel2pinds(indices, 2, SHAPE)
    return SimpleNamespace(indices=indices, xyz=xyz, new_xyz=new_xyz, new_coords=new_coords, vol=vol, counts=counts,
                           xyz_cnt=np.bincount(indices[:, 0], minlength=2).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _want(case, per_scene=160):
    s = _scene(per_scene)
    rng_, radius, ns = CASES[case]
    return R.voxel_query(rng_, radius, ns, s.xyz, s.new_xyz, s.new_coords, s.vol, return_counts=True)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_restatement_hand_case():
    """1 x 3 x 3 x 3 volume, one query at the centre cell, range [1, 1, 1], nsample 4: rows come back in visit order (z outermost, x innermost), a
    short query repeats its first hit, a far query gets -1 and keeps the caller's other slots."""
    # occupied cells [z, y, x] -> row: visit order from the centre is rows 2, 0, 3, 1, 4
    cells = [(0, 1, 1), (2, 0, 0), (0, 0, 2), (1, 1, 1), (2, 2, 2)]                    # rows 0..4
    indices = np.array([(0,) + c for c in cells], np.int32)
    vol = R.voxel2pinds(indices, 1, (3, 3, 3))
    assert vol[0, 1, 1, 1] == 3 and vol[0, 0, 0, 2] == 2 and (vol == -1).sum() == 27 - 5
    xyz = (indices[:, [3, 2, 1]] + 0.5).astype(np.float32)
    centre = np.array([[1.5, 1.5, 1.5]], np.float32)
    coords = np.array([[0, 1, 1, 1]], np.int32)
    assert R.voxel_query([1, 1, 1], 10.0, 4, xyz, centre, coords, vol).tolist() == [[2, 0, 3, 1]]
    assert R.voxel_query([1, 1, 1], 10.0, 8, xyz, centre, coords, vol).tolist() == [[2, 0, 3, 1, 4, 2, 2, 2]]
    # radius 1.0: only rows 0 (distance 1 exactly: kept, the test is `>`) and 3 (distance 0) survive
    assert R.voxel_query([1, 1, 1], 1.0, 4, xyz, centre, coords, vol).tolist() == [[0, 3, 0, 0]]
    # range [0, 1, 1] never leaves the z = 1 slab: row 3 only
    assert R.voxel_query([0, 1, 1], 10.0, 4, xyz, centre, coords, vol).tolist() == [[3, 3, 3, 3]]
    far = R.voxel_query([1, 1, 1], 10.0, 4, xyz, centre + 50, np.array([[0, 51, 51, 51]], np.int32), vol, idx=np.full((1, 4), 7, np.int32))
    assert far.tolist() == [[-1, 7, 7, 7]]
    idx, empty = R.post_process(np.array([[-1, 7, 7, 7], [2, 0, 3, 1]], np.int32))
    assert idx.tolist() == [[0, 0, 0, 0], [2, 0, 3, 1]] and empty.tolist() == [True, False]


def test_registries_resolve(hip_lib):
    from seevcn_amd.pcdet.models import detectors, roi_heads
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda, voxel_pool_modules, voxel_query_utils
    assert roi_heads.__all__['VoxelRCNNHead'].__name__ == 'VoxelRCNNHead' and detectors.__all__['VoxelRCNN'].__name__ == 'VoxelRCNN'
    assert callable(voxel_query_utils.voxel_query) and hasattr(voxel_pool_modules, 'NeighborVoxelSAModuleMSG')
    import seevcn_amd._lib as L
    with pytest.raises(L.SeevcnHipError):                           # bound to the kernel: refuses CPU tensors like its neighbours, no NotImplementedError
        z = torch.zeros((1, 4), dtype=torch.int32)
        pointnet2_stack_cuda.voxel_query_wrapper(1, 1, 1, 1, 4, 1.0, 0, 0, 0, torch.zeros(1, 3), torch.zeros(1, 3), z, torch.zeros((1, 1, 1, 1), dtype=torch.int32), z)
    with pytest.raises(NotImplementedError):
        pointnet2_stack_cuda.vector_pool_wrapper()
    with pytest.raises(NotImplementedError):
        voxel_pool_modules.NeighborVoxelSAModuleMSG(query_ranges=[[1, 1, 1]], radii=[1.0], nsamples=[4], mlps=[[16, 16, 16]], pool_method='sum_pool')(
            torch.zeros(1, 3), None, torch.zeros(1, 3), None, torch.zeros((1, 4), dtype=torch.int32), torch.zeros(1, 16), None)


def _head(cfg):
    from seevcn_amd.pcdet.models import roi_heads
    return roi_heads.__all__['VoxelRCNNHead'](backbone_channels={'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}, model_cfg=cfg,
                                              point_cloud_range=C.KITTI_RANGE, voxel_size=[0.05, 0.05, 0.1], num_class=1, input_channels=None)


def test_head_state_dict_keys_and_shapes():
    import copy
    cfg = C.voxelrcnn_cfg()
    before = copy.deepcopy(cfg)
    sd = {k: tuple(v.shape) for k, v in _head(cfg).state_dict().items()}
    assert sd['roi_grid_pool_layers.0.mlps_in.0.0.weight'] == (32, 32, 1) and sd['roi_grid_pool_layers.1.mlps_in.0.0.weight'] == (32, 64, 1)
    assert sd['roi_grid_pool_layers.0.mlps_pos.0.0.weight'] == (32, 3, 1, 1) and sd['roi_grid_pool_layers.2.mlps_pos.0.1.running_var'] == (32,)
    assert sd['roi_grid_pool_layers.2.mlps_out.0.0.weight'] == (32, 32, 1) and sd['roi_grid_pool_layers.2.mlps_out.0.1.weight'] == (32,)
    assert sd['shared_fc_layer.0.weight'] == (256, 216 * 96) and sd['shared_fc_layer.1.running_mean'] == (256,)
    assert sd['shared_fc_layer.4.weight'] == (256, 256)                                       # Dropout sits at index 3 (DP_RATIO 0.3)
    assert sd['cls_fc_layers.0.weight'] == (256, 256) and sd['cls_pred_layer.weight'] == (1, 256) and sd['cls_pred_layer.bias'] == (1,)
    assert sd['reg_fc_layers.4.weight'] == (256, 256) and sd['reg_pred_layer.weight'] == (7, 256) and sd['reg_pred_layer.bias'] == (7,)
    assert not any('groupers' in k for k in sd)
    # building twice from one config object: the same model, the config untouched (the reference prepends the backbone channel in place)
    sd2 = {k: tuple(v.shape) for k, v in _head(cfg).state_dict().items()}
    assert sd2 == sd and cfg == before


def test_detector_builds_from_registry():
    from seevcn_amd.pcdet.models import detectors
    cfg = C.voxelrcnn_model_cfg(roi_per_image=32, nms_post_train=64, nms_pre_train=512)
    net = detectors.build_detector(cfg, num_class=1, dataset=C.SyntheticDatasetInfo(class_names=C.VOXELRCNN_CLASS_NAMES, num_point_features=4))
    assert type(net).__name__ == 'VoxelRCNN' and net.LOSS_HEADS == ('dense_head', 'roi_head') and net.pfe is None and net.point_head is None
    assert type(net.roi_head).__name__ == 'VoxelRCNNHead' and net.roi_head.shared_fc_layer[0].weight.shape == (256, 216 * 96)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(s, cuda):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return SimpleNamespace(indices=t(s.indices), xyz=t(s.xyz), new_xyz=t(s.new_xyz), new_coords=t(s.new_coords), vol=t(s.vol), xyz_cnt=t(s.xyz_cnt),
                           new_cnt=t(np.array(s.counts, np.int32)))


@pytest.mark.gpu
def test_hip_generate_voxel2pinds_exact(cuda, hip_lib):
    from seevcn_amd.pcdet.utils import common_utils
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_query_utils
    s = _scene()
    tap = SimpleNamespace(indices=torch.from_numpy(s.indices).to(cuda), spatial_shape=list(SHAPE), batch_size=2)
    got = common_utils.generate_voxel2pinds(tap)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), s.vol)
    assert np.array_equal(common_utils.scatter_point_inds(tap.indices.long(), torch.arange(len(s.indices), dtype=torch.int32, device=cuda),
                                                          [2] + list(SHAPE)).cpu().numpy(), s.vol)
    for _ in range(2):                                              # the borrowed volume: the same cells inside the block, all -1 again behind it
        with voxel_query_utils.borrowed_voxel2pinds(tap) as vol:
            assert np.array_equal(vol.cpu().numpy(), s.vol)
        assert bool((vol == -1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
def test_hip_voxel_query_bit_exact(case, cuda, hip_lib):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda, voxel_query_utils
    s, (rng_, radius, ns) = _scene(), CASES[case]
    want, hits = _want(case)
    # conditions on the INPUT (the restatement's own hit counts), not on the kernel
    empty, partial, over = int((hits == 0).sum()), int(((hits >= 1) & (hits < ns)).sum()), int((hits > ns).sum())
    print(f"case {case + 1}: empty {empty} partial {partial} over {over} of {len(hits)}")
    assert empty >= 10
    if case in (0, 1, 3):
        assert over >= 10 and partial >= 10
    d = _dev(s, cuda)
    idx = torch.zeros((len(s.new_xyz), ns), dtype=torch.int32, device=cuda)
    assert pointnet2_stack_cuda.voxel_query_wrapper(len(s.new_xyz), *SHAPE, ns, radius, *rng_, d.new_xyz, d.xyz, d.new_coords, d.vol, idx) == 1
    assert np.array_equal(idx.cpu().numpy(), want)
    got_idx, got_empty = voxel_query_utils.voxel_query(rng_, radius, ns, d.xyz, d.new_xyz, d.new_coords, d.vol)
    want_idx, want_empty = R.post_process(want)
    assert np.array_equal(got_idx.cpu().numpy(), want_idx) and np.array_equal(got_empty.cpu().numpy(), want_empty)


@pytest.mark.gpu
def test_hip_voxel_query_radius_zero_finds_own_cell(cuda, hip_lib):
    """radius 0, range [0, 0, 0], queries copied from 50 voxel centres: dist2 = 0 is not > 0, every query finds exactly its own row."""
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda
    s = _scene()
    pick = np.random.default_rng(SEED + 1).choice(len(s.indices), 50, replace=False)
    new_xyz, new_coords = s.xyz[pick].copy(), s.indices[pick].copy()
    want = R.voxel_query([0, 0, 0], 0.0, 1, s.xyz, new_xyz, new_coords, s.vol)
    assert np.array_equal(want[:, 0], pick)
    d = _dev(s, cuda)
    idx = torch.zeros((50, 1), dtype=torch.int32, device=cuda)
    pointnet2_stack_cuda.voxel_query_wrapper(50, *SHAPE, 1, 0.0, 0, 0, 0, torch.from_numpy(new_xyz).to(cuda), d.xyz, torch.from_numpy(new_coords).to(cuda), d.vol, idx)
    assert np.array_equal(idx.cpu().numpy(), want)


POOL_QUERIES = (167, 166)               # M = 333: no multiple of 16 or 64


def _module(c, ns, pool_method, cuda=None):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules
    rng_, radius, _ = CASES[0]
    m = voxel_pool_modules.NeighborVoxelSAModuleMSG(query_ranges=[rng_], radii=[radius], nsamples=[ns], mlps=[[c, 32, 32]], pool_method=pool_method)
    m.load_state_dict(seeded_state_dict(m, seed=17))                # running statistics away from (0, 1)
    return m if cuda is None else m.to(cuda)


@functools.lru_cache(maxsize=None)
def _pool_case(c, ns):
    """the scene with 333 queries, case 1's range and radius at nsample ns, seeded features of c channels; idx from the restatement"""
    s = _scene(POOL_QUERIES)
    rng_, radius, _ = CASES[0]
    idx, hits = R.voxel_query(rng_, radius, ns, s.xyz, s.new_xyz, s.new_coords, s.vol, return_counts=True)
    assert (hits == 0).sum() >= 10 and ((hits >= 1) & (hits < ns)).sum() >= 10 and (ns == 32 or (hits > ns).sum() >= 10)
    feats = np.random.default_rng(SEED + c).normal(size=(len(s.xyz), c)).astype(np.float32)
    return s, idx, hits, feats


def _forward(m, s, feats, cuda):
    d = _dev(s, cuda)
    new_coords_xyz = d.new_coords[:, [0, 3, 2, 1]].contiguous()     # the module takes [b, x, y, z]
    return m(xyz=d.xyz, xyz_batch_cnt=d.xyz_cnt, new_xyz=d.new_xyz, new_xyz_batch_cnt=d.new_cnt, new_coords=new_coords_xyz, features=feats, voxel2point_indices=d.vol)


@pytest.mark.gpu
@pytest.mark.parametrize("c,ns", [(16, 16), (64, 16), (16, 32), (64, 32)])
def test_hip_voxel_pool_max_and_module_match_float64(c, ns, cuda, hip_lib, monkeypatch):
    import seevcn_amd._lib as L
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules
    from tolerances import assert_close_per_channel
    s, idx, hits, feats = _pool_case(c, ns)
    assert len(s.new_xyz) == 333
    m = _module(c, ns, 'max_pool', cuda).eval()
    sd = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
    want = R.neighbor_voxel_sa(sd, [idx], s.xyz, s.new_xyz, feats)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    # the kernel alone, on an f_in of its own
    lib = L.load()
    f_in = np.random.default_rng(SEED + 5).normal(size=(len(s.xyz), 32)).astype(np.float32)
    wp = np.random.default_rng(SEED + 6).normal(size=(32, 3)).astype(np.float32)
    bp = np.random.default_rng(SEED + 7).normal(size=(32,)).astype(np.float32)
    out = torch.empty((333, 32), dtype=torch.float32, device=cuda)
    args = [t(a) for a in (f_in, s.xyz, s.new_xyz, idx, wp, bp)]                               # kept alive across the launch
    L.check(lib.sv_voxel_pool_max(*[L.ptr(a) for a in args], 333, len(s.xyz), 32, ns, L.ptr(out), L.stream()), "sv_voxel_pool_max")
    want_k = R.voxel_pool_max(f_in, s.xyz, s.new_xyz, idx, wp, bp)
    assert_close_per_channel(out.cpu().numpy(), want_k, rtol=1e-3, atol_frac=1e-4, name="sv_voxel_pool_max")
    assert np.array_equal(out.cpu().numpy()[hits == 0], np.broadcast_to(np.maximum(bp, 0), (int((hits == 0).sum()), 32)))
    # the module: fused route, then the module tree
    with torch.no_grad():
        monkeypatch.setattr(voxel_pool_modules, "FUSED_VOXEL_POOL_OFF", False)
        assert m._fused_ok(0, t(s.xyz), t(feats))
        fused = _forward(m, s, t(feats), cuda).cpu().numpy()
        monkeypatch.setattr(voxel_pool_modules, "FUSED_VOXEL_POOL_OFF", True)
        assert not m._fused_ok(0, t(s.xyz), t(feats))
        tree = _forward(m, s, t(feats), cuda).cpu().numpy()
    assert_close_per_channel(fused, want, rtol=1e-3, atol_frac=1e-4, name="fused route")
    assert_close_per_channel(tree, want, rtol=1e-3, atol_frac=1e-4, name="module tree")
    # rows of empty queries = ReLU(BN(conv(0))) pushed through mlps_out: a kernel that reads row 0 instead fails only here
    f64 = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    pos0 = f64['mlps_pos.0.1.bias'] - f64['mlps_pos.0.1.running_mean'] * f64['mlps_pos.0.1.weight'] / np.sqrt(f64['mlps_pos.0.1.running_var'] + 1e-5)
    y = np.maximum(pos0, 0) @ f64['mlps_out.0.0.weight'][:, :, 0].T
    y = (y - f64['mlps_out.0.1.running_mean']) / np.sqrt(f64['mlps_out.0.1.running_var'] + 1e-5) * f64['mlps_out.0.1.weight'] + f64['mlps_out.0.1.bias']
    row = np.broadcast_to(np.maximum(y, 0), (int((hits == 0).sum()), 32))
    for name, got in (("fused", fused), ("tree", tree)):
        np.testing.assert_allclose(got[hits == 0], row, rtol=1e-3, atol=1e-4 * np.abs(want).max(), err_msg=name + ": rows of empty queries")


@pytest.mark.gpu
def test_hip_voxel_pool_avg_matches_float64(cuda, hip_lib):
    from tolerances import assert_close_per_channel
    s, idx, hits, feats = _pool_case(16, 16)
    m = _module(16, 16, 'avg_pool', cuda).eval()
    want = R.neighbor_voxel_sa({k: v.cpu().numpy() for k, v in m.state_dict().items()}, [idx], s.xyz, s.new_xyz, feats, pool_method='avg_pool')
    with torch.no_grad():
        assert not m._fused_ok(0, torch.from_numpy(s.xyz).to(cuda), torch.from_numpy(feats).to(cuda))
        got = _forward(m, s, torch.from_numpy(feats).to(cuda), cuda).cpu().numpy()
    assert_close_per_channel(got, want, rtol=1e-3, atol_frac=1e-4, name="avg_pool")


def _torch_f64(sd, idx, xyz, new_xyz, features):
    """the module in training mode as a float64 torch graph on the CPU (batch statistics), for the gradient with respect to `features`"""
    p = {k: v.double().cpu() for k, v in sd.items()}

    def bn(x, prefix):
        return (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + 1e-5) * p[prefix + '.weight'] + p[prefix + '.bias']

    empty = torch.from_numpy(idx[:, 0] < 0)
    j = torch.from_numpy(np.where(idx[:, :1] < 0, 0, idx).astype(np.int64))
    keep = (~empty).view(-1, 1, 1)
    f_in = bn(features @ p['mlps_in.0.0.weight'][:, :, 0].T, 'mlps_in.0.1')
    g_feat = torch.where(keep, f_in[j], 0.0)
    g_xyz = torch.where(keep, torch.from_numpy(xyz).double()[j] - torch.from_numpy(new_xyz).double()[:, None, :], 0.0)
    M, ns, _ = g_xyz.shape
    pos = bn(g_xyz.reshape(M * ns, 3) @ p['mlps_pos.0.0.weight'][:, :, 0, 0].T, 'mlps_pos.0.1').reshape(M, ns, -1)
    x = torch.relu(g_feat + pos).max(dim=1)[0]
    return torch.relu(bn(x @ p['mlps_out.0.0.weight'][:, :, 0].T, 'mlps_out.0.1'))


@pytest.mark.gpu
def test_hip_voxel_pool_training_route(cuda, hip_lib):
    """One forward / backward in train(): outputs against the restatement with batch statistics, the gradient with respect to `features` against
    torch.autograd over a float64 CPU graph of the same module; the same again with order-fixed gradients."""
    import seevcn_amd
    from tolerances import assert_close_per_channel
    s, idx, hits, feats = _pool_case(16, 16)
    m0 = _module(16, 16, 'max_pool')
    sd = {k: v.clone() for k, v in m0.state_dict().items()}
    want = R.neighbor_voxel_sa({k: v.numpy() for k, v in sd.items()}, [idx], s.xyz, s.new_xyz, feats, train=True)
    gout = np.random.default_rng(SEED + 9).normal(size=want.shape)
    f64 = torch.from_numpy(feats).double().requires_grad_(True)
    ref = _torch_f64(sd, idx, s.xyz, s.new_xyz, f64)
    np.testing.assert_allclose(ref.detach().numpy(), want, rtol=1e-9, atol=1e-9)              # the two float64 statements agree
    (ref * torch.from_numpy(gout)).sum().backward()
    want_grad = f64.grad.numpy()
    results = []
    for fixed in (False, True):
        m = _module(16, 16, 'max_pool', cuda).train()
        x = torch.from_numpy(feats).to(cuda).requires_grad_(True)
        calls = seevcn_amd.ordered_gradient_calls().get("group_points", 0)
        with seevcn_amd.set_ordered_gradients(fixed):
            out = _forward(m, s, x, cuda)
            (out * torch.from_numpy(gout).float().to(cuda)).sum().backward()
        assert (seevcn_amd.ordered_gradient_calls().get("group_points", 0) > calls) == fixed     # the grouping's gradient took the route asked for
        assert_close_per_channel(out.detach().cpu().numpy(), want, rtol=1e-3, atol_frac=1e-4, name=f"train output (ordered={fixed})")
        assert_close_per_channel(x.grad.cpu().numpy(), want_grad, rtol=1e-3, atol_frac=1e-4, name=f"d features (ordered={fixed})")
        assert torch.isfinite(m.mlps_pos[0][0].weight.grad).all() and int(m.mlps_in[0][1].num_batches_tracked) == 1
        results.append(x.grad.cpu().numpy())
    assert_close_per_channel(results[1], results[0], rtol=1e-3, atol_frac=1e-4, name="ordered vs atomic gradient")
