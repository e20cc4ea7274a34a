"""PV-RCNN++'s vector-pool aggregation on the GPU: the choice kernel, the local 3-NN, the stacked interpolation and their gradients against the numpy
restatement (tests/vector_pool_reference.py), the modules against the reference's own classes (tests/golden/vector_pool_modules.npz), and the way
PVRCNNHead / VoxelSetAbstraction reach them through build_local_aggregation_module.

Indices, counts, copied values, single subtractions, fp32 distances and the three-product interpolation are compared BIT FOR BIT: the restatement
rounds every fp32 operation where the kernels do (the library is built without fp contraction and with a correctly rounded divide), so it decides
every in-range and tie case itself and no case is left out.  Coordinates are multiples of 1/256 so that rows exactly on local == +-R, duplicate
points and distance ties all occur."""
import functools
import os

import numpy as np
import pytest
import torch

import vector_pool_inputs as I
import vector_pool_reference as VR

F = np.float32
R0 = 0.5                                           # exactly representable, like every planted offset
SCENES = {"ragged": ((67, 0, 130), (5, 3, 0)), "edges": ((1, 64, 65), (2, 2, 2))}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_bits(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    assert len(bad) == 0, f"{name}: {len(bad)} of {got.size} elements differ, first at {bad[:5]}: {got.ravel()[bad[:5]]} vs {want.ravel()[bad[:5]]}"


@functools.lru_cache(None)
def _scene(tag, c_in=4):
    """xyz, xyz_cnt, new_xyz, new_cnt, feats.  Per scene a cloud within +-1 of its centre on a 1/256 lattice, queries on a 1/64 lattice; planted in
    the first scene that has queries: rows exactly on +-R of query 0, a duplicate pair, and (scene of 67 rows only) the 8 cells of [2, 2, 2] around
    query 1 filled by row 17 and the 27 cells of [3, 3, 3] around query 2 filled by row 46."""
    sup, qry = SCENES[tag]
    rng = np.random.default_rng(7 if tag == "ragged" else 8)
    xyz, new_xyz = [], []
    for b, (n, m) in enumerate(zip(sup, qry)):
        centre = np.array([4.0 * b, -2.0 * b, 1.0], F)
        p = (centre + rng.integers(-256, 257, (n, 3)) / 256.0).astype(F)
        q = (centre + rng.integers(-32, 33, (m, 3)) / 64.0).astype(F)
        if m and n >= 64:
            p[3] = q[0] + np.array([R0, 0, 0], F)
            p[4] = q[0] + np.array([-R0, R0, -R0], F)
            p[5] = q[0] + np.array([0.25, -R0, 0.125], F)
            p[7] = p[6]
            if n == 67:
                p[10:18] = q[1] + np.array([[x, y, z] for x in (-0.25, 0.25) for y in (-0.25, 0.25) for z in (-0.25, 0.25)], F)
                p[20:47] = q[2] + np.array([[x, y, z] for x in (-0.375, 0, 0.375) for y in (-0.375, 0, 0.375) for z in (-0.375, 0, 0.375)], F)
        xyz.append(p)
        new_xyz.append(q)
    xyz, new_xyz = np.concatenate(xyz), np.concatenate(new_xyz)
    feats = rng.normal(0, 1, (len(xyz), c_in)).astype(F)
    return xyz, np.array(sup, np.int32), new_xyz, np.array(qry, np.int32), feats


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------------------------------------------- 4. choice
@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 2, 2), (3, 3, 3), (3, 2, 1)])
@pytest.mark.parametrize("tag", sorted(SCENES))
def test_choice_kernel_matches_the_restatement_bit_for_bit(cuda, hip_lib, tag, grid):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as ext
    for c_in, c_each in ((2, 2), (4, 2), (30, 30), (60, 30)):
        xyz, xyz_cnt, new_xyz, new_cnt, feats = _scene(tag, c_in)
        dev = [_t(a, cuda) for a in (xyz, xyz_cnt, feats, new_xyz, new_cnt)]
        for nsample in (-1, 1, 5, 32):
            for neighbor_type in (0, 1):
                want = VR.choice(xyz, xyz_cnt, feats, new_xyz, new_cnt, grid, R0, nsample, neighbor_type, c_each)
                got = ext.vector_pool_choice(dev[0], dev[1], dev[2], dev[3], dev[4], grid[0], grid[1], grid[2], R0, c_each, nsample, neighbor_type)
                for g, w, name in zip(got, want, ("choice", "point_cnt", "new_local_xyz", "new_features")):
                    _assert_bits(g.cpu().numpy(), w, f"{name} {tag} grid={grid} c={c_in}/{c_each} nsample={nsample} type={neighbor_type}")
    # what was planted is there: rows exactly on +-R are in range, and a query has every cell filled well before its scene ends
    xyz, xyz_cnt, new_xyz, new_cnt, feats = _scene(tag)
    first = 0 if tag == "ragged" else 1                                              # the first scene with at least 64 rows
    ps, qs = int(xyz_cnt[:first].sum()), int(new_cnt[:first].sum())
    loc = VR.local_xyz(xyz[ps + 3:ps + 6], new_xyz[qs])
    assert loc[0, 0] == R0 and loc[1].tolist() == [-R0, R0, -R0] and loc[2, 1] == -R0 and VR.in_range(loc, R0, 0).all()
    if tag == "ragged" and grid != (3, 2, 1):
        ch = VR.choice(xyz, xyz_cnt, feats, new_xyz, new_cnt, grid, R0, -1, 0, 2)[0]
        q = 1 if grid == (2, 2, 2) else 2
        assert (ch[q] >= 0).all() and ch[q].max() < 47 < xyz_cnt[0]


# ---------------------------------------------------------------------------------------------------------------- 5. three_nn
def _centres(new_xyz, R, grid):
    offs = [(-R + R / n + 2 * R / n * np.arange(n)).astype(F) for n in grid]
    off = np.stack(np.meshgrid(*offs, indexing="ij"), -1).reshape(-1, 3).astype(F)
    return (new_xyz[:, None, :] + off[None]).astype(F)


@functools.lru_cache(None)
def _list_scene():
    """One scene: query i at (8 i, 0, 0) has exactly LENS[i] rows within the cube of half-edge R0 (lists of length 0, 1, 2, 3, 63, 64, 65), rows
    shuffled, duplicates among them; a second scene of 1 100 rows: rows 0..999 on a shell 0.3..0.45 around its query 0, rows 1000..1049 around its
    query 1 (across the 1024-row tile edge), rows 1050..1099 within 0.05 of query 0 -- nearer than anything in its list, and beyond the cap."""
    lens = (0, 1, 2, 3, 63, 64, 65)
    rng = np.random.default_rng(11)
    q_a = np.array([[8.0 * i, 0, 0] for i in range(len(lens))], F)
    clusters = [q_a[i] + rng.integers(-100, 101, (n, 3)) / 256.0 for i, n in enumerate(lens)]
    for c in clusters:
        if len(c) >= 3:
            c[1] = c[0]                                                               # a duplicate pair inside the list
    rows = np.concatenate(clusters).astype(F)
    rows = rows[rng.permutation(len(rows))]
    q_b = np.array([[100, 0, 0], [110, 0, 0]], F)
    d = rng.normal(0, 1, (1000, 3))
    shell = q_b[0] + np.round(d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 0.45, (1000, 1)) * 256) / 256
    near1 = q_b[1] + rng.integers(-100, 101, (50, 3)) / 256.0
    near0 = q_b[0] + rng.integers(-8, 9, (50, 3)) / 256.0
    big = np.concatenate([shell, near1, near0]).astype(F)
    return (np.concatenate([rows, big]), np.array([len(rows), len(big)], np.int32), np.concatenate([q_a, q_b]), np.array([len(q_a), 2], np.int32), lens)


def _run_three_nn(cuda, xyz, xyz_cnt, new_xyz, new_cnt, grid, R, nsample, neighbor_type, name):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as ext
    cen = _centres(new_xyz, R0, grid)
    want_idx, want_d2 = VR.three_nn(xyz, xyz_cnt, new_xyz, cen, new_cnt, F(R), nsample, neighbor_type)
    idx, d2 = ext.vector_pool_three_nn(_t(xyz, cuda), _t(xyz_cnt, cuda), _t(new_xyz, cuda), _t(cen, cuda), _t(new_cnt, cuda), float(F(R)), nsample,
                                       neighbor_type)
    _assert_bits(idx.cpu().numpy(), want_idx, "idx " + name)
    _assert_bits(d2.cpu().numpy(), want_d2, "dist2 " + name)
    return want_idx, want_d2


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 2, 2), (3, 3, 3)])
def test_three_nn_kernel_matches_the_restatement_bit_for_bit(cuda, hip_lib, grid):
    for tag in sorted(SCENES):
        xyz, xyz_cnt, new_xyz, new_cnt, _ = _scene(tag)
        for nsample in (-1, 2, 5):
            for neighbor_type in (0, 1):
                _run_three_nn(cuda, xyz, xyz_cnt, new_xyz, new_cnt, grid, R0 * 2.0, nsample, neighbor_type, f"{tag} G={grid} nsample={nsample} type={neighbor_type}")
    xyz, xyz_cnt, new_xyz, new_cnt, lens = _list_scene()
    for nsample in (-1, 2, 5):
        idx, d2 = _run_three_nn(cuda, xyz, xyz_cnt, new_xyz, new_cnt, grid, R0, nsample, 0, f"lists G={grid} nsample={nsample}")
        if nsample == -1:
            for i, n in enumerate(lens):
                assert len(VR.neighbour_list(xyz[:xyz_cnt[0]], new_xyz[i], F(R0), -1, 0)) == n
                distinct = {len(set(r)) for r in idx[i].tolist()}
                assert distinct == ({1} if n <= 1 else {2} if n == 2 else distinct) and (n > 0 or np.all(idx[i] == -1) and np.all(np.isposinf(d2[i])))
            start = int(xyz_cnt[0])
            assert len(VR.neighbour_list(xyz[start:], new_xyz[len(lens)], F(R0), -1, 0)) == 1000           # 1 050 in range, cut at the cap
            assert idx[len(lens)].max() < start + 1000 and idx[len(lens) + 1].min() >= start + 1000       # rows past the cap ignored although nearer


# ---------------------------------------------------------------------------------------------------------------- 6. interpolate
def _interp_case(C, rows=130, n=50, seed=5):
    rng = np.random.default_rng(seed + C)
    feats = rng.normal(0, 1, (n, C)).astype(F)
    idx = rng.integers(0, n, (rows, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (rows, 3)).astype(F)
    idx[:70, 0] = 7                                   # feature row 7 is named by more than 64 keys ...
    idx[idx == 9] = 10                                # ... and row 9 by none
    idx[70] = 3                                       # three equal indices
    w[71] = 0                                         # a row of zero weights
    idx[72, 1] = -1                                   # a negative index contributes nothing
    idx[73, 2] = n                                    # nor does one past the end
    return feats, idx, w, rng.normal(0, 1, (rows, C)).astype(F)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 30, 32, 70])
def test_three_interpolate_forward_and_gradients(cuda, hip_lib, C):
    import seevcn_amd
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as ext
    feats, idx, w, grad_out = _interp_case(C)
    n = len(feats)
    d_feats, d_idx, d_w, d_go = (_t(a, cuda) for a in (feats, idx, w, grad_out))
    out = torch.full((len(idx), C), float("nan"), device=cuda)
    ext.three_interpolate_wrapper(d_feats, d_idx, d_w, out)
    _assert_bits(out.cpu().numpy(), VR.interpolate(feats, idx, w), f"three_interpolate C={C}")

    def grad():
        g = torch.full((n, C), float("nan"), device=cuda)
        ext.three_interpolate_grad_wrapper(d_go, d_idx, d_w, g)
        return g.cpu().numpy()

    terms = VR.interpolate_grad_terms(grad_out, idx, w, n)
    assert len(terms[7]) > 64 and len(terms[9]) == 0
    with seevcn_amd.set_ordered_gradients(True):
        a, b = grad(), grad()
    _assert_bits(a, VR.ordered_sum(terms, C), f"three_interpolate grad ordered C={C}")
    _assert_bits(b, a, f"three_interpolate grad ordered C={C}, second call")
    assert np.all(_bits(a)[9] == 0)
    ref, bound = VR.sum_f64_and_bound(VR.interpolate_grad_terms(grad_out, idx, w, n, exact=True), C)
    err = np.abs(grad().astype(np.float64) - ref)
    print(f"three_interpolate grad plain C={C}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound), f"plain gradient outside K * 2^-24 * sum|term|: {np.max(err - bound)}"


# ---------------------------------------------------------------------------------------------------------------- 7. choice gradient
@pytest.mark.gpu
@pytest.mark.parametrize("c_in,c_each", [(4, 2), (30, 30), (60, 30)])
def test_choice_gradient_ordered_and_plain(cuda, hip_lib, c_in, c_each):
    import seevcn_amd
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as ext
    rng = np.random.default_rng(c_in)
    M, G, N = 40, 8, 30
    ch = rng.integers(-1, N, (M, G)).astype(np.int32)
    ch.reshape(-1)[::4][:70] = 3                      # support row 3 is named by more than 64 keys ...
    ch[ch == 5] = -1                                  # ... and row 5 by none
    cnt = (ch >= 0).astype(np.int32)
    grad_new = rng.normal(0, 1, (M, G * c_each)).astype(F)
    d_ch, d_cnt, d_g = (_t(a, cuda) for a in (ch, cnt, grad_new))
    terms = VR.choice_grad_terms(grad_new, ch, cnt, N, c_in, c_each)
    assert len(terms[3]) > 64 and len(terms[5]) == 0
    with seevcn_amd.set_ordered_gradients(True):
        a, b = (ext.vector_pool_choice_grad(d_g, d_ch, d_cnt, N, c_in).cpu().numpy() for _ in range(2))
    _assert_bits(a, VR.ordered_sum(terms, c_in), f"vector_pool grad ordered {c_in}/{c_each}")
    _assert_bits(b, a, f"vector_pool grad ordered {c_in}/{c_each}, second call")
    assert np.all(_bits(a)[5] == 0)
    ref, bound = VR.sum_f64_and_bound(VR.choice_grad_terms(grad_new, ch, cnt, N, c_in, c_each, exact=True), c_in)
    err = np.abs(ext.vector_pool_choice_grad(d_g, d_ch, d_cnt, N, c_in).cpu().numpy().astype(np.float64) - ref)
    print(f"vector_pool grad plain {c_in}/{c_each}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound), f"plain gradient outside K * 2^-24 * sum|term|: {np.max(err - bound)}"


@pytest.mark.gpu
def test_gradients_through_autograd_follow_the_switch(cuda, hip_lib):
    """The switch is read when the backward runs; ordered_gradient_calls() moves only on the ordered route."""
    import seevcn_amd
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    C = 30
    feats, idx, w, grad_out = _interp_case(C)
    xyz, xyz_cnt, new_xyz, new_cnt, sf = _scene("ragged", 60)
    d = {k: _t(v, cuda) for k, v in dict(idx=idx, w=w, go=grad_out, xyz=xyz, xyz_cnt=xyz_cnt, new_xyz=new_xyz, new_cnt=new_cnt).items()}
    f1 = _t(feats, cuda).requires_grad_(True)
    f2 = _t(sf, cuda).requires_grad_(True)

    def interp():
        f1.grad = None
        pu.three_interpolate(f1, d["idx"], d["w"]).backward(d["go"])
        return f1.grad.cpu().numpy()

    def pool():
        f2.grad = None
        out = pu.vector_pool_with_voxel_query_op(d["xyz"], d["xyz_cnt"], f2, d["new_xyz"], d["new_cnt"], 3, 3, 3, R0, 30, 1, 20, 5, 0, 1)
        assert out[0].requires_grad and not out[1].requires_grad and out[2].tolist() == [20] and not out[3].requires_grad
        out[0].square().sum().backward()
        return f2.grad.cpu().numpy(), out

    for key, fn in (("three_interpolate", interp), ("vector_pool", pool)):
        calls = seevcn_amd.ordered_gradient_calls()[key]
        fn()
        assert seevcn_amd.ordered_gradient_calls()[key] == calls                       # off: the atomic entry
        with seevcn_amd.set_ordered_gradients(True):
            a, b = fn(), fn()
        assert seevcn_amd.ordered_gradient_calls()[key] == calls + 2
        if key == "three_interpolate":
            _assert_bits(a, VR.ordered_sum(VR.interpolate_grad_terms(grad_out, idx, w, len(feats)), C), "three_interpolate backward, ordered")
            _assert_bits(b, a, "three_interpolate backward, second call")
        else:
            ch, cnt, _, nf = VR.choice(xyz, xyz_cnt, sf, new_xyz, new_cnt, (3, 3, 3), R0, 5, 0, 30)
            _assert_bits(a[1][0].detach().cpu().numpy(), nf, "vector_pool_with_voxel_query_op new_features")
            _assert_bits(a[0], VR.ordered_sum(VR.choice_grad_terms((2 * nf).astype(F), ch, cnt, len(xyz), 60, 30), 60), "vector pool backward, ordered")
            _assert_bits(b[0], a[0], "vector pool backward, second call")
    with pytest.raises(NotImplementedError):
        pu.vector_pool_with_voxel_query_op(d["xyz"], d["xyz_cnt"], f2, d["new_xyz"], d["new_cnt"], 3, 3, 3, R0, 30, 1, 20, 5, 0, 0)


# ---------------------------------------------------------------------------------------------------------------- 8. modules vs the golden
def _layer(tag, cuda):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm
    from seevcn_amd.seeding import seeded_state_dict
    c = I.CONFIGS[tag]
    layer, _ = pm.build_local_aggregation_module(input_channels=c["input_channels"], config=c["cfg"])
    layer.load_state_dict(seeded_state_dict(layer, seed=I.WEIGHT_SEED))
    return layer.to(cuda)


def _gold_inputs(gold, tag, cuda):
    return {k: _t(gold[f"{tag}_{k}"], cuda) for k in ("xyz", "xyz_batch_cnt", "new_xyz", "new_xyz_batch_cnt", "features")}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(I.CONFIGS))
def test_modules_match_the_reference_golden(cuda, hip_lib, golden_dir, tag):
    import seevcn_amd
    from oracle.tolerances import assert_close_per_channel
    gold = np.load(os.path.join(golden_dir, "vector_pool_modules.npz"))
    for k, v in I.make_inputs(tag).items():
        assert np.array_equal(gold[f"{tag}_{k}"], v)
    layer = _layer(tag, cuda).eval()
    inp = _gold_inputs(gold, tag, cuda)
    with torch.no_grad():
        new_xyz, out = layer(**inp)
    assert new_xyz is inp["new_xyz"]
    assert_close_per_channel(out.cpu().numpy(), gold[tag + "_out"], rtol=1e-3, atol_frac=1e-4, name=f"VectorPoolAggregationModuleMSG {tag}")
    # train mode: backward reaches the features and every parameter; ordered: two runs give the same bits
    layer.train()

    def grads():
        layer.zero_grad(set_to_none=True)
        f = inp["features"].clone().requires_grad_(True)
        layer(**dict(inp, features=f))[1].square().sum().backward()
        return f.grad.cpu().numpy()

    g = grads()
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    for name, p in layer.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
    with seevcn_amd.set_ordered_gradients(True):
        a, b = grads(), grads()
    _assert_bits(b, a, f"features.grad of {tag}, ordered, second run")
    assert layer.layer_0.num_mean_points_per_grid == 20


# ---------------------------------------------------------------------------------------------------------------- 9. public builders
@pytest.mark.gpu
def test_pvrcnn_head_pools_through_the_vector_pool_layer(cuda, hip_lib):
    from oracle.tolerances import assert_close_per_channel
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models.roi_heads.pvrcnn_head import PVRCNNHead
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm, pointnet2_stack_cuda as ext
    from seevcn_amd.seeding import seeded_state_dict
    layer, c_out = pm.build_local_aggregation_module(input_channels=90, config=C.PVRCNNPP_ROI_GRID_POOL)
    assert isinstance(layer, pm.VectorPoolAggregationModuleMSG) and c_out == 128
    roi_cfg = dict(C.pvrcnn_cfg()[2], ROI_GRID_POOL=dict(C.PVRCNNPP_ROI_GRID_POOL, GRID_SIZE=2))
    head = PVRCNNHead(input_channels=90, model_cfg=roi_cfg, num_class=1)
    head.load_state_dict(seeded_state_dict(head, seed=41))
    head = head.to(cuda).eval()
    rng = np.random.default_rng(42)
    B, K, n_roi = 2, 64, 4
    rois = np.concatenate([rng.uniform(-1, 1, (B, n_roi, 3)), rng.uniform(1.5, 3.0, (B, n_roi, 3)), rng.uniform(-3, 3, (B, n_roi, 1))], -1).astype(F)
    pts = rng.uniform(-2.5, 2.5, (B * K, 3)).astype(F)
    coords = np.concatenate([np.repeat(np.arange(B), K)[:, None].astype(F), pts], 1)
    feats = rng.normal(0, 1, (B * K, 90)).astype(F)
    scores = rng.uniform(0.2, 1, (B * K,)).astype(F)
    bd = dict(batch_size=B, rois=_t(rois, cuda), point_coords=_t(coords, cuda), point_features=_t(feats, cuda), point_cls_scores=_t(scores, cuda))
    with torch.no_grad():
        pooled = head.roi_grid_pool(bd)
        assert pooled.shape == (B * n_roi, 8, 128)
        # the same layer fed by the restatement instead of the kernel: everything above the choice is torch either way
        glob, _ = head.get_global_grid_points_of_roi(bd["rois"], grid_size=2)
        new_xyz = glob.reshape(-1, 3).contiguous()
        f = (bd["point_features"] * bd["point_cls_scores"].view(-1, 1)).contiguous()
        cnt, qcnt = np.full(B, K, np.int32), np.full(B, n_roi * 8, np.int32)
        real = ext.vector_pool_choice

        def restated(sx, sc, sf, nx, nc, gx, gy, gz, dist, c_each, nsample, ntype):
            return tuple(_t(a, cuda) for a in VR.choice(sx.cpu().numpy(), cnt, sf.cpu().numpy(), nx.cpu().numpy(), qcnt, (gx, gy, gz), dist, nsample,
                                                         ntype, c_each))

        ext.vector_pool_choice = restated
        try:
            _, want = head.roi_grid_pool_layer(xyz=_t(pts, cuda), xyz_batch_cnt=_t(cnt, cuda), new_xyz=new_xyz, new_xyz_batch_cnt=_t(qcnt, cuda), features=f)
        finally:
            ext.vector_pool_choice = real
    assert_close_per_channel(pooled.reshape(-1, 128).cpu().numpy(), want.cpu().numpy(), rtol=1e-3, atol_frac=1e-4, name="PVRCNNHead.roi_grid_pool")
    with pytest.raises(NotImplementedError):
        ext.vector_pool_wrapper()                     # the pybind-shaped name stays the raising stub: its host-sized buffer + count is what went away


def test_voxel_set_abstraction_builds_the_vector_pool_sa_layers():
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.pcdet.models.backbones_3d.pfe import voxel_set_abstraction as vsa_mod
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm
    pfe = dict(NAME='VoxelSetAbstraction', POINT_SOURCE='raw_points', NUM_KEYPOINTS=4096, NUM_OUTPUT_FEATURES=90, SAMPLE_METHOD='FPS',
               FEATURES_SOURCE=['bev', 'x_conv3', 'x_conv4', 'raw_points'], SA_LAYER=C.PVRCNNPP_SA_LAYER)
    vsa = vsa_mod.VoxelSetAbstraction(pfe, voxel_size=[0.1, 0.1, 0.15], point_cloud_range=[-75.2, -75.2, -2, 75.2, 75.2, 4], num_bev_features=256,
                                      num_rawpoint_features=5)
    assert all(isinstance(m, pm.VectorPoolAggregationModuleMSG) for m in list(vsa.SA_layers) + [vsa.SA_rawpoints])
    assert vsa.num_point_features_before_fusion == 128 + 128 + 256 + 32 and vsa.num_point_features == 90
    sd = vsa.state_dict()
    for key, shape in (("SA_layers.0.layer_0.separate_local_aggregation_layer.0.weight", (27 * 32, 32 + 9, 1)),
                       ("SA_layers.1.layer_1.post_mlps.3.weight", (64, 64, 1)), ("SA_layers.0.msg_post_mlps.0.weight", (128, 131, 1)),
                       ("SA_rawpoints.layer_0.separate_local_aggregation_layer.0.weight", (8 * 32, 2 + 9, 1)),
                       ("SA_rawpoints.msg_post_mlps.1.running_mean", (32,)), ("vsa_point_feature_fusion.0.weight", (90, 544))):
        assert tuple(sd[key].shape) == shape, key
    assert not any("local_interpolate_module" in k for k in sd)                       # it has no parameters (mlp=None)
    with pytest.raises(NotImplementedError):
        vsa_mod.VoxelSetAbstraction(dict(pfe, SAMPLE_METHOD='SPC'), voxel_size=[0.1, 0.1, 0.15], point_cloud_range=[-75.2, -75.2, -2, 75.2, 75.2, 4],
                                    num_bev_features=256, num_rawpoint_features=5)._fps_inputs(
            dict(batch_size=1, points=torch.zeros((4, 5))))


# ---------------------------------------------------------------------------------------------------------------- 10. no host read
@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(I.CONFIGS))
def test_eval_forward_reads_nothing_back(cuda, hip_lib, golden_dir, tag):
    gold = np.load(os.path.join(golden_dir, "vector_pool_modules.npz"))
    layer = _layer(tag, cuda).eval()
    inp = _gold_inputs(gold, tag, cuda)
    with torch.no_grad():
        previous = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            _, out = layer(**inp)
        finally:
            torch.cuda.set_sync_debug_mode(previous)
    assert torch.isfinite(out).all()
