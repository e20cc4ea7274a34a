"""Deterministic inputs shared by make_spc_golden.py (reference side) and tests/test_spc_sampling.py: 2 scenes of 3 000 and 1 500 random points plus
planted rows, 8 RoIs per scene two of them zero rows, K = 256, S = 6.  The radius is 1.5 (the yaml's 1.6 is no fp32 number) so that the planted
threshold edge is exact.  Random points within 1e-5 (relative) of their selection threshold, or whose sector quotient is within 1e-5 of an
integer, are redrawn: there torch's CPU norm / division and a GPU's may legitimately differ in the last place."""
import numpy as np

K, S, RADIUS, BAND = 256, 6, 1.5, 1e-5
N_RANDOM = (3000, 1500)
FILTER_RADIUS = 2.5

F = np.float32


def _rois(rng, b):
    r = np.zeros((8, 7), F)
    # RoI 0: the threshold-edge box, max_dim = 5 exactly -> threshold 6.5; RoIs 1, 2: the equal-distance pair of the tie case (swapped in scene 1)
    r[0] = [0, -8, 0, 6, 8, 0, 0]
    pair = np.array([[30, 10, 0, 4, 4, 2, 0.5], [34, 10, 0, 0, 0, 0, 0]], F)         # thresholds 3 + 1.5 and 0 + 1.5, both 2 away from (32, 10, 0)
    r[1:3] = pair if b == 0 else pair[::-1]
    for j in (3, 4, 5):
        r[j] = np.concatenate([rng.uniform([8, -35, -1], [35, 0, 1]), rng.uniform([1.5, 0.6, 1.2], [5, 2.2, 2]), rng.uniform(-3, 3, 1)])
    return r                                                                          # rows 6, 7: zero padding; the random RoIs keep clear of the planted cases


def planted_rows():
    e = np.nextafter(F(6.5), F(0))
    return np.array([[6.5, -8, 0], [e, -8, 0], [0, -14.5, 0], [0, -8, e],            # threshold edge: out, in, out, in
                     [32, 10, 0],                                                              # nearest-RoI tie: scene 0 in, scene 1 out
                     [-1, 0.0, 0], [-1, -0.0, 0], [0.0, 0.0, 0], [-0.0, 0.0, 0], [0.0, -0.0, 0], [-0.0, -0.0, 0],
                     [1, 0.0, 0], [1, -0.0, 0], [0, 1, 0], [0, -1, 0],                            # sector edges, selected by the zero rows
                     [1.25, 0.5, 0.25]], F)


def make_inputs():
    import spc_reference as R
    rng = np.random.default_rng(2026)
    xyz, cnt, rois = [], [], []
    for b, n in enumerate(N_RANDOM):
        r = _rois(rng, b)
        pts = np.zeros((0, 3), F)
        while len(pts) < n:
            m = n - len(pts)
            near = r[rng.integers(0, 8, m), 0:3] + rng.normal(0, 2.5, (m, 3)) * np.array([1, 1, 0.3])
            far = rng.uniform([-40, -40, -2], [40, 40, 2], (m, 3))
            cand = np.where(rng.uniform(size=(m, 1)) < 0.6, near, far).astype(F)
            _, d, thr = R.select_mask(cand, r, RADIUS, return_parts=True)
            q = R.sector_quotient(cand, S)
            ok = (np.abs(d.astype(np.float64) - thr) > BAND * thr) & (np.abs(q - np.round(q)) > BAND)
            for rad in (FILTER_RADIUS,):                                              # the neighbour filter's threshold as well
                _, d2, thr2 = R.select_mask(cand, r, rad, return_parts=True)
                ok &= np.abs(d2.astype(np.float64) - thr2) > BAND * thr2
            pts = np.concatenate([pts, cand[ok]])
        plant = planted_rows()
        at = np.sort(rng.choice(n, len(plant), replace=False)) + np.arange(len(plant))    # planted rows spread through the scene, in order
        full = np.insert(pts, at - np.arange(len(plant)), plant, axis=0)
        xyz.append(full.astype(F))
        cnt.append(len(full))
        rois.append(r)
    xyz = np.concatenate(xyz)
    cnt = np.array(cnt, np.int32)
    feats = rng.normal(size=(len(xyz), 4)).astype(F)
    planted = np.zeros(len(xyz), bool)
    plant = planted_rows()
    start = 0
    for n in cnt:                                                                     # mark planted rows by value (bit pattern)
        blk = xyz[start:start + n]
        for p in plant:
            planted[start:start + n] |= (blk.view(np.uint32) == p.view(np.uint32)).all(1)
        start += n
    bev = rng.normal(size=(len(cnt), 16, 50, 50)).astype(F)
    return dict(bev=bev, xyz=xyz, cnt=cnt, start=(np.cumsum(cnt) - cnt).astype(np.int32), rois=np.stack(rois).astype(F), feats=feats, planted=planted)


# the module case: VoxelSetAbstraction with SPC keypoints and the RoI neighbour filter over two sources, the vector-pool layer shrunk
PC_RANGE, VOXEL_SIZE, BEV_STRIDE = [-40, -40, -3, 40, 40, 1], [0.2, 0.2, 0.4], 8
MODULE_SEED = 17


def module_cfg():
    from seevcn_amd.pcdet import model_cfgs as C
    pfe, _, _ = C.pvrcnnpp_cfg(num_keypoints=K, features_source=('bev', 'raw_points'))
    pfe['SPC_SAMPLING'] = dict(NUM_SECTORS=S, SAMPLE_RADIUS_WITH_ROI=RADIUS)
    pfe['NUM_OUTPUT_FEATURES'] = 32
    pfe['SA_LAYER'] = dict(raw_points=C._vector_pool('local_interpolation', 2, 16, [((2, 2, 2), 0.4, -1, 16), ((3, 3, 3), 0.8, -1, 16)],
                                                     FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=FILTER_RADIUS))
    return pfe


def points_tensor(inp):
    """(N, 1 + 3 + 4) [bs_idx, x, y, z, features]"""
    b = np.repeat(np.arange(len(inp['cnt'])), inp['cnt']).astype(F)
    return np.concatenate([b[:, None], inp['xyz'], inp['feats']], 1)
