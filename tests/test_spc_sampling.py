"""SPC keypoint sampling and the RoI neighbour filter on the GPU, stage by stage against the numpy restatement (tests/spc_reference.py, pinned by
tests/test_spc_reference.py) and end to end against a golden made by the reference's own Python (tests/golden/make_spc_golden.py)."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import spc_inputs as I
import spc_reference as R

F = np.float32


@functools.lru_cache(maxsize=None)
def _case():
    """inputs + the restatement's results, computed once and shared (read-only) by the tests"""
    inp = I.make_inputs()
    rows, kp, sector, tab = R.sample_batch(inp["xyz"], inp["start"], inp["cnt"], inp["rois"], I.RADIUS, I.K, I.S)
    for v in list(inp.values()) + [rows, kp, sector] + list(tab.values()):
        v.setflags(write=False)
    return inp, rows, kp, sector, tab


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "spc_sampling.npz"))


def _ops():
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda
    return pointnet2_stack_cuda


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_seed_leaves_no_random_row_in_the_band():
    """CPU: the committed seed has no random row within 1e-5 of a sector edge (the GPU test may leave out at most 2)."""
    inp, _, _, _, _ = _case()
    q = R.sector_quotient(inp["xyz"], I.S)
    assert int(((np.abs(q - np.round(q)) <= I.BAND) & ~inp["planted"]).sum()) == 0
    assert int(inp["planted"].sum()) == 2 * len(I.planted_rows())


def test_restatement_equals_reference_golden(golden_dir):
    """CPU: on the band-free inputs the restatement equals what the reference's own functions gave: mask, sector and keypoints."""
    inp, rows, kp, sector, tab = _case()
    g = _golden(golden_dir)
    for k in ("xyz", "cnt", "rois", "feats", "bev"):
        assert np.array_equal(g[k].view(np.uint32) if g[k].dtype == F else g[k], inp[k].view(np.uint32) if inp[k].dtype == F else inp[k]), k
    assert np.array_equal(g["point_mask"], sector >= 0)
    # what the reference's sector_fps handed to its sampler: the selected points sector by sector in row order, their counts and quotas
    live = tab["seg_cnt"] > 0
    assert np.array_equal(g["seg_cnt"], tab["seg_cnt"][live]) and np.array_equal(g["seg_npoint"], tab["seg_m"][live])
    assert np.array_equal(g["seg_scene"], np.repeat(np.arange(2), I.S)[live])
    handed = np.concatenate([tab["order"][a:a + c] for a, c in zip(tab["seg_start"][live], tab["seg_cnt"][live])])
    assert np.array_equal(g["seg_xyz"].view(np.uint32), inp["xyz"][handed].view(np.uint32))
    assert np.array_equal(g["kp_cnt"], kp)
    assert np.array_equal(g["keypoints"].view(np.uint32), inp["xyz"][rows].view(np.uint32))
    for b, m in enumerate(g["filter_mask_cnt"]):
        s, n = inp["start"][b], inp["cnt"][b]
        assert int(R.select_mask(inp["xyz"][s:s + n], inp["rois"][b], I.FILTER_RADIUS).sum()) == m


@pytest.mark.gpu
def test_hip_spc_select_matches_restatement(cuda, hip_lib):
    inp, _, _, sector, _ = _case()
    got = _ops().spc_select(_t(inp["xyz"], cuda), _t(inp["cnt"], cuda), _t(inp["rois"], cuda), I.RADIUS, I.S, int(inp["cnt"].max())).cpu().numpy()
    assert np.array_equal(got >= 0, sector >= 0)                               # the mask: every row
    q = R.sector_quotient(inp["xyz"], I.S)
    band = (np.abs(q - np.round(q)) <= I.BAND) & ~inp["planted"]
    assert band.sum() <= 2
    diff = np.nonzero((got != sector) & ~band)[0]
    print("rows in the band:", int(band.sum()), "sector differences outside it:", len(diff),
          "nearest edge distance of a random selected row:", float(np.abs(q - np.round(q))[~inp["planted"] & (sector >= 0)].min()))
    assert len(diff) == 0, (diff[:8], got[diff[:8]], sector[diff[:8]])
    assert np.array_equal(got[inp["planted"]], sector[inp["planted"]])
    # a bound below the largest scene only sizes the grid: every row is still written
    low = _ops().spc_select(_t(inp["xyz"], cuda), _t(inp["cnt"], cuda), _t(inp["rois"], cuda), I.RADIUS, I.S, 300).cpu().numpy()
    assert np.array_equal(low, got)
    # the yaml's largest RoI block (TRAIN NMS_POST_MAXSIZE 512) and the entry's limit of 2048, the extra rows zero padding: 8 and 32 KB of LDS
    for m in (512, 2048):
        rois = np.zeros((2, m, 7), F)
        rois[:, :8] = inp["rois"]
        assert np.array_equal(_ops().spc_select(_t(inp["xyz"], cuda), _t(inp["cnt"], cuda), _t(rois, cuda), I.RADIUS, I.S).cpu().numpy(), got), m
    # mask mode, with N as the bound of a scene's size
    mask = _ops().spc_select(_t(inp["xyz"], cuda), _t(inp["cnt"], cuda), _t(inp["rois"], cuda), I.RADIUS, 0).cpu().numpy()
    assert np.array_equal(mask, np.where(sector >= 0, 0, -1))


def _partition_case():
    """the shared scenes + four more: nothing selected (row 0 in a sector), all selected rows in no sector, nothing selected with row 0 in no sector,
    an empty scene, and a last ordinary one behind it"""
    inp, _, _, sector, _ = _case()
    rng = np.random.default_rng(3)
    far = rng.uniform(5, 30, (40, 3)).astype(F)
    edge = np.array([[-1 - i, 0.0, 0] for i in range(5)], F)                    # sector S
    extra = [(far, np.full(40, -1)), (np.concatenate([edge, far[:7]]), np.array([I.S] * 5 + [-1] * 7)), (np.concatenate([edge[:1], far[:3]]), np.full(4, -1)),
             (np.zeros((0, 3), F), np.zeros(0)), (far[:9], R.sector_of(far[:9], I.S))]
    xyz = np.concatenate([inp["xyz"]] + [e[0] for e in extra])
    sec = np.concatenate([sector] + [e[1] for e in extra]).astype(np.int32)
    cnt = np.concatenate([inp["cnt"], [len(e[0]) for e in extra]]).astype(np.int32)
    return xyz, sec, cnt, (np.cumsum(cnt) - cnt).astype(np.int32)


@pytest.mark.gpu
def test_hip_spc_partition_matches_restatement(cuda, hip_lib):
    xyz, sec, cnt, start = _partition_case()
    want = R.partition(sec, xyz, start, cnt, I.K, I.S)
    assert want["kp_cnt"][2:].tolist() == [1, I.K, I.K, 0, 9]
    order, tables = _ops().spc_partition(_t(sec, cuda), _t(xyz, cuda), _t(cnt, cuda), I.K, I.S)
    tables, order = tables.cpu().numpy(), order.cpu().numpy()
    for i, k in enumerate(("seg_start", "seg_cnt", "seg_m", "seg_out_start")):
        assert np.array_equal(tables[i], want[k]), k
    assert np.array_equal(tables[4][:len(cnt)], want["kp_cnt"])
    defined = want["order"] >= 0
    assert np.array_equal(order[defined], want["order"][defined])
    # mask mode
    want = R.partition(np.where(sec >= 0, 0, -1).astype(np.int32), None, start, cnt, 0, 0)
    order, tables = _ops().spc_partition(_t(np.where(sec >= 0, 0, -1).astype(np.int32), cuda), None, _t(cnt, cuda), 0, 0)
    tables, order = tables.cpu().numpy(), order.cpu().numpy()
    assert np.array_equal(tables[0], want["seg_start"]) and np.array_equal(tables[1], want["seg_cnt"]) and np.array_equal(tables[4], want["kp_cnt"])
    assert np.array_equal(order[want["order"] >= 0], want["order"][want["order"] >= 0])


def _fps_case():
    """segments of every size at which the kernel changes its path, read through a shuffled row list"""
    rng = np.random.default_rng(11)
    sizes = [1, 2, 63, 64, 65, 1023, 1024, 1025, 3000, 6000, 12000, 25000, 100, 5, 5, 0, 40, 7, 17000]
    quota = [1, 2, 20, 20, 20, 24, 24, 24, 12, 8, 6, 8, 9, 12, 5, 4, 0, 7, 5]
    segs = []
    for i, n in enumerate(sizes):
        p = rng.normal(0, 4, (n, 3)).astype(F)
        if i % 2 == 0:
            p = np.round(p)                                                     # a lattice: rounds full of ties
        segs.append(p)
    segs[12] = np.tile(np.array([[1.5, -2, 0.25]], F), (100, 1))                # duplicated points: every pick is a tie
    segs[14] = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], F)     # the five-point tie
    pts = np.concatenate(segs)
    N = len(pts)
    perm = rng.permutation(N)                                                   # position in `order` -> row of xyz
    xyz = np.zeros((N, 3), F)
    xyz[perm] = pts
    seg_cnt = np.array(sizes, np.int32)
    seg_start = (np.cumsum(seg_cnt) - seg_cnt).astype(np.int32)
    seg_m = np.array(quota, np.int32)
    seg_out = (np.cumsum(seg_m + 2) - seg_m - 1).astype(np.int32)                # a guard word on either side of every segment's picks
    return xyz, perm.astype(np.int32), seg_start, seg_cnt, seg_m, seg_out, int(seg_out[-1] + seg_m[-1] + 1)


@functools.lru_cache(maxsize=None)
def _fps_want():
    xyz, order, seg_start, seg_cnt, seg_m, seg_out, total = _fps_case()
    full = R.fps_ragged(xyz, order, seg_start, seg_cnt, seg_m, seg_out, np.full(total, -7, np.int64))
    full.setflags(write=False)
    return full


@pytest.mark.gpu
@pytest.mark.parametrize("bound", [25000, 17000, 12000, 3000])
def test_hip_ragged_fps_matches_restatement(cuda, hip_lib, bound):
    """bound = the host's upper bound of a segment: the four instantiations of the kernel (streaming form carried, registers up to 48 points per
    thread, up to 32, up to 8); larger segments are taken out by a zero quota and, like the n == 0 / m == 0 ones, must leave their output untouched."""
    xyz, order, seg_start, seg_cnt, seg_m, seg_out, total = _fps_case()
    m = np.where(seg_cnt <= bound, seg_m, 0).astype(np.int32)
    want = np.array(_fps_want())
    for g in np.nonzero(m != seg_m)[0]:
        want[seg_out[g]:seg_out[g] + seg_m[g]] = -7
    idx = torch.full((total,), -7, dtype=torch.int32, device=cuda)
    _ops().stack_farthest_point_sampling_ragged(_t(xyz, cuda), _t(order, cuda), _t(seg_start, cuda), _t(seg_cnt, cuda), _t(m, cuda), _t(seg_out, cuda),
                                                idx, bound)
    got = idx.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    if bound == 25000:
        five = seg_out[14]
        assert order[seg_start[14] + 4] == got[five + 1]                        # the five-point case: second pick is its row 4


@pytest.mark.gpu
def test_hip_stack_farthest_point_sample_routes(cuda, hip_lib):
    from oracle import pointnet2 as op2
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    rng = np.random.default_rng(5)
    cnt = np.array([700, 1, 1300], np.int32)
    xyz = np.round(rng.normal(0, 3, (int(cnt.sum()), 3)) * 2).astype(F) / 2
    npoint = [33, 3, 64]
    want = R.stack_fps(xyz, cnt, npoint)
    x, c = _t(xyz, cuda), _t(cnt, cuda)
    for arg in (npoint, torch.tensor(npoint, dtype=torch.int32), torch.tensor(npoint, device=cuda)):
        got = U.stack_farthest_point_sample(x, c, arg)
        assert got.dtype == torch.int32 and got.shape == (sum(npoint),)
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(U.StackFarthestPointSampling.apply(x, c, 5).cpu().numpy(), R.stack_fps(xyz, cnt, 5))
    # an int npoint keeps the (batch, npoint) table of the existing route
    cnt2 = np.array([700, 601], np.int32)
    got = U.stack_farthest_point_sample(x[:1301].contiguous(), _t(cnt2, cuda), 48, 700)
    assert got.shape == (2, 48)
    assert torch.equal(U.stack_farthest_point_sample(x[:1301].contiguous(), _t(cnt2, cuda), np.int64(48), 700), got)      # a numpy integer is an int
    for b, (s, n) in enumerate(((0, 700), (700, 601))):
        assert np.array_equal(got[b].cpu().numpy(), s + np.asarray(op2.farthest_point_sampling(xyz[s:s + n], 48)))


def _vsa(cuda, sources=("raw_points",)):
    from seevcn_amd.pcdet.models.backbones_3d.pfe.voxel_set_abstraction import VoxelSetAbstraction
    from seeding import seeded_state_dict
    cfg = I.module_cfg()
    cfg["FEATURES_SOURCE"] = list(sources)
    vsa = VoxelSetAbstraction(cfg, voxel_size=I.VOXEL_SIZE, point_cloud_range=np.array(I.PC_RANGE, F), num_bev_features=16, num_rawpoint_features=7)
    vsa.load_state_dict(seeded_state_dict(vsa, seed=I.MODULE_SEED))
    return vsa.to(cuda)


def _batch(inp, cuda):
    return {"batch_size": len(inp["cnt"]), "points": _t(I.points_tensor(inp), cuda), "rois": _t(inp["rois"], cuda),
            "points_per_scene": [int(c) for c in inp["cnt"]], "spatial_features": _t(inp["bev"], cuda), "spatial_features_stride": I.BEV_STRIDE}


@pytest.mark.gpu
def test_hip_spc_keypoints_end_to_end(cuda, hip_lib, golden_dir):
    inp, rows, kp, _, _ = _case()
    g = _golden(golden_dir)
    vsa = _vsa(cuda)
    bd = _batch(inp, cuda)
    vsa.prefetch_keypoints(bd)                                                   # SPC: nothing to start early
    assert "_fps_prefetch" not in bd
    vsa.get_sampled_points(dict(bd))                                             # warm: library load, constant tensors
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            keypoints = vsa.get_sampled_points(bd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [str(x.message) for x in w if "synchroniz" in str(x.message).lower()]
    assert len(syncs) <= 1, syncs
    assert "point_coords_per_scene" not in bd
    got = keypoints.cpu().numpy()
    want = np.concatenate([np.repeat(np.arange(2), kp).astype(F)[:, None], inp["xyz"][rows]], 1)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bd["_keypoint_batch_cnt"].cpu().numpy(), kp)
    assert np.array_equal(got[:, 1:].view(np.uint32), g["keypoints"].view(np.uint32)) and np.array_equal(g["kp_cnt"], kp)


@pytest.mark.gpu
def test_hip_one_scene_functions(cuda, hip_lib):
    """sample_points_with_roi and sector_fps with the reference's arguments and returns, one scene each"""
    from seevcn_amd.pcdet.models.backbones_3d.pfe import voxel_set_abstraction as M
    inp, rows, kp, sector, _ = _case()
    s, n = int(inp["start"][1]), int(inp["cnt"][1])
    pts, rois = _t(inp["xyz"][s:s + n], cuda), _t(inp["rois"][1], cuda)
    sampled, mask = M.sample_points_with_roi(rois=rois, points=pts, sample_radius_with_roi=I.RADIUS, num_max_points_of_part=1000)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), sector[s:s + n] >= 0)
    assert torch.equal(sampled, pts[mask])
    out = M.sector_fps(points=sampled, num_sampled_points=I.K, num_sectors=I.S)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), inp["xyz"][rows[kp[0]:]].view(np.uint32))
    none, mask = M.sample_points_with_roi(rois=rois + 1000, points=pts, sample_radius_with_roi=I.RADIUS)
    assert not bool(mask.any()) and torch.equal(none, pts[:1])


@pytest.mark.gpu
def test_hip_roi_neighbour_filter(cuda, hip_lib):
    from seevcn_amd.pcdet.models.backbones_3d.pfe.voxel_set_abstraction import VoxelSetAbstraction
    inp, _, _, _, _ = _case()
    keep = np.concatenate([R.select_mask(inp["xyz"][s:s + n], inp["rois"][b], I.FILTER_RADIUS) for b, (s, n) in enumerate(zip(inp["start"], inp["cnt"]))])
    seen = {}

    def aggregate(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features):
        seen.update(xyz=xyz, cnt=xyz_batch_cnt, features=features)
        return new_xyz, (features * torch.arange(1, features.shape[0] + 1, device=features.device).view(-1, 1)).sum(0, keepdim=True)

    feats = _t(inp["feats"], cuda).requires_grad_(True)
    bs = _t(np.repeat(np.arange(2), inp["cnt"]).astype(F), cuda)
    new_xyz = torch.zeros((2, 3), device=cuda)
    out = VoxelSetAbstraction.aggregate_keypoint_features_from_one_source(
        2, aggregate, _t(inp["xyz"], cuda), feats, bs, new_xyz, torch.ones(2, dtype=torch.int32, device=cuda), filter_neighbors_with_roi=True,
        radius_of_neighbor=I.FILTER_RADIUS, num_max_points_of_part=1000, rois=_t(inp["rois"], cuda))
    assert np.array_equal(seen["xyz"].cpu().numpy().view(np.uint32), inp["xyz"][keep].view(np.uint32))
    assert np.array_equal(seen["features"].detach().cpu().numpy().view(np.uint32), inp["feats"][keep].view(np.uint32))
    assert seen["cnt"].cpu().tolist() == [int(keep[:inp["cnt"][0]].sum()), int(keep[inp["cnt"][0]:].sum())]
    out.sum().backward()
    grad = feats.grad.cpu().numpy()
    want = np.zeros_like(inp["feats"])
    want[keep] = np.arange(1, keep.sum() + 1, dtype=F)[:, None]
    assert np.array_equal(grad, want)                                            # the gradient reaches exactly the kept rows, each once


@pytest.mark.gpu
def test_hip_voxel_set_abstraction_spc_matches_reference_golden(cuda, hip_lib, golden_dir):
    from tolerances import assert_close_per_channel
    inp, _, kp, _, _ = _case()
    g = _golden(golden_dir)
    vsa = _vsa(cuda, ("bev", "raw_points")).eval()
    with torch.no_grad():
        bd = vsa(_batch(inp, cuda))
    assert np.array_equal(bd["point_coords"].cpu().numpy().view(np.uint32), g["point_coords"].view(np.uint32))
    assert_close_per_channel(bd["point_features_before_fusion"].cpu().numpy(), g["point_features_before_fusion"], rtol=1e-3, atol_frac=1e-4,
                             name="point_features_before_fusion")
    assert_close_per_channel(bd["point_features"].cpu().numpy(), g["point_features"], rtol=1e-3, atol_frac=1e-4, name="point_features")
