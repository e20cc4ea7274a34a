"""Hand cases that pin the numpy restatement of SPC keypoint sampling (tests/spc_reference.py): the GPU tests hold the kernels to it."""
import math

import numpy as np

import spc_reference as R

F = np.float32
S6 = 6


def _roi(x, y, z, l, w, h):
    return np.array([x, y, z, l, w, h, 0], F)


def test_threshold_edge_is_strict():
    rois = np.stack([_roi(0, 0, 0, 6, 8, 0)])                      # max_dim = 5 exactly, + 1.5 = 6.5
    assert R.roi_threshold(rois, 1.5)[0] == F(6.5)
    pts = np.array([[6.5, 0, 0], [np.nextafter(F(6.5), F(0)), 0, 0], [0, -6.5, 0], [0, 0, np.nextafter(F(6.5), F(0))]], F)
    assert R.select_mask(pts, rois, 1.5).tolist() == [False, True, False, True]


def test_nearest_roi_tie_takes_the_lower_index():
    big, small = _roi(2, 0, 0, 2, 2, 2), _roi(-2, 0, 0, 0, 0, 0)  # thresholds sqrt(3) + 0.5 > 2 and 0.5 < 2
    pts = np.zeros((1, 3), F)
    assert R.select_mask(pts, np.stack([big, small]), 0.5).tolist() == [True]
    assert R.select_mask(pts, np.stack([small, big]), 0.5).tolist() == [False]


def test_tie_is_judged_on_the_rooted_distance():
    # squared distances 1 + 2^-23 (RoI 0) and 1 (RoI 1) both root to 1.0: a tie, so RoI 0 decides although RoI 1 is nearer by the squares
    far, near = _roi(1, 3e-4, 0, 2, 2, 2), _roi(1, 0, 0, 0, 0, 0)
    d2 = F(1) + F(3e-4) * F(3e-4)
    assert d2 == np.nextafter(F(1), F(2)) and np.sqrt(d2) == F(1)
    pts = np.zeros((1, 3), F)
    assert R.select_mask(pts, np.stack([far, near]), 0.5).tolist() == [True]
    assert R.select_mask(pts, np.stack([near, far]), 0.5).tolist() == [False]


def test_zero_padding_rows_select_around_the_origin():
    rois = np.stack([_roi(50, 50, 0, 4, 2, 2), np.zeros(7, F), np.zeros(7, F)])
    pts = np.array([[1.5, 0, 0], [0, 1.7, 0], [1, 1, 0.5], [50, 51, 0], [30, 30, 0]], F)
    assert R.select_mask(pts, rois, 1.6).tolist() == [True, False, True, True, False]


def test_sector_edges():
    pts = np.array([[-1, 0.0, 0], [-1, -0.0, 0], [0.0, 0.0, 0], [-0.0, 0.0, 0], [0.0, -0.0, 0], [-0.0, -0.0, 0],
                    [1, 0.0, 0], [1, -0.0, 0], [0, 1, 0], [0, -1, 0]], F)
    ang = R.angle(pts[:, 0], pts[:, 1])
    pi, hp = F(np.pi), F(np.pi / 2)
    assert ang.tolist() == [pi, -pi, 0.0, pi, 0.0, -pi, 0.0, 0.0, hp, -hp]
    assert np.signbit(ang).tolist() == [False, True, False, False, True, True, False, True, False, True]
    # what the fp32 expressions give, statement by statement
    size = F(np.pi * 2 / S6)
    want = [int(min(max(math.floor(F(F(a) + pi) / size), 0), S6)) for a in ang]
    got = R.sector_of(pts, S6).tolist()
    assert got == want
    assert got[0] == S6 and got[1] == 0                           # (-1, +0): 2 pi / (2 pi / 6) lands on S itself; (-1, -0): angle 0
    assert got == [6, 0, 3, 6, 3, 0, 3, 3, 4, 1]


def _scene(sectors_of_rows):
    """points on the unit circle in the middle of the wanted sector (S: the (-1, +0) point), one per row"""
    pts = []
    for i, s in enumerate(sectors_of_rows):
        if s == S6:
            pts.append([-1 - i, 0.0, 0])
        else:
            a = -np.pi + (s + 0.5) * 2 * np.pi / S6
            pts.append([(1 + i) * np.cos(a), (1 + i) * np.sin(a), 0])
    return np.array(pts, F)


def test_partition_quotas_and_order():
    secs = [0] * 7 + [2] * 5 + [5] * 3 + [S6] * 2 + [2] * 4 + [0] * 2
    xyz = _scene(secs)
    assert R.sector_of(xyz, S6).tolist() == secs
    sector = np.array(secs, np.int32)
    sector[3] = -1                                                 # one row not selected
    K = 10
    t = R.partition(sector, xyz, [0], [len(secs)], K, S6)
    n_sel = len(secs) - 1                                          # 22, the two rows of sector S counted
    cnts = [8, 0, 9, 0, 0, 3]
    assert t["seg_cnt"].tolist() == cnts
    quota = [min(c, math.ceil(c / n_sel * K)) for c in cnts]
    assert quota == [4, 0, 5, 0, 0, 2] and t["seg_m"].tolist() == quota
    assert t["kp_cnt"].tolist() == [11] and K < 11 <= K + S6       # the ceilings add up to K + (something <= S)
    assert t["seg_out_start"].tolist() == [0, 4, 4, 9, 9, 9]
    assert t["seg_start"].tolist() == [0, 8, 8, 17, 17, 17]
    assert t["order"][:8].tolist() == [0, 1, 2, 4, 5, 6, 21, 22] and t["order"][8:17].tolist() == [7, 8, 9, 10, 11, 17, 18, 19, 20]
    assert t["order"][17:20].tolist() == [12, 13, 14] and t["order"][20:22].tolist() == [15, 16] and t["order"][22] == -1
    # min(cnt, .) binding: a large K gives every sector all of its rows
    t = R.partition(sector, xyz, [0], [len(secs)], 1000, S6)
    assert t["seg_m"].tolist() == cnts and t["kp_cnt"].tolist() == [20]


def test_partition_fallbacks():
    K = 7
    # scene 0: nothing selected -> its row 0 alone; scene 1: all selected rows in no sector -> one segment, quota K; scene 2: row 0 in no sector
    xyz = np.concatenate([_scene([4, 1, 2]), _scene([S6, 0, S6, S6]), _scene([S6, 3])])
    sector = np.array([-1, -1, -1, S6, -1, S6, S6, -1, -1], np.int32)
    t = R.partition(sector, xyz, [0, 3, 7], [3, 4, 2], K, S6)
    assert t["kp_cnt"].tolist() == [1, K, K]
    assert t["seg_cnt"].reshape(3, S6).tolist() == [[0, 0, 0, 0, 1, 0], [3, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]]
    assert t["seg_m"].reshape(3, S6).tolist() == [[0, 0, 0, 0, 1, 0], [K, 0, 0, 0, 0, 0], [K, 0, 0, 0, 0, 0]]
    assert t["seg_start"].reshape(3, S6)[:, 0].tolist() == [0, 3, 7] and t["seg_start"][4] == 0
    assert t["order"][0] == 0 and t["order"][3:6].tolist() == [3, 5, 6] and t["order"][7] == 7
    assert t["seg_out_start"].reshape(3, S6)[:, 0].tolist() == [0, K + S6, 2 * (K + S6)]
    rows, kp, _, _ = R.sample_batch(xyz, [0, 3, 7], [3, 4, 2], np.zeros((3, 1, 7), F) + F(1e6), 0.1, K, S6)    # RoIs far away: nothing selected
    assert kp.tolist() == [1, K, K] and rows.tolist() == [0] + [3] * K + [7] * K    # rows 3 and 7 lie in no sector: the whole quota


def test_mask_mode():
    sector = np.array([0, -1, 0, -1, -1, 0, 0], np.int32)
    t = R.partition(sector, None, [0, 4], [4, 3], 0, 0)
    assert t["seg_start"].tolist() == [0, 4] and t["seg_cnt"].tolist() == [2, 2] and t["kp_cnt"].tolist() == [2, 2]
    assert t["order"].tolist() == [0, 2, -1, -1, 5, 6, -1]


def test_fps_five_point_tie():
    """Row 0 at the origin, rows 1-4 at distance 1.  Slot 0 of the kernel's tree first meets slot 4 (0 < 1: row 4 moves to slot 0) and from then on
    wins every equal comparison as the lower slot, so the second pick is row 4.  The batch kernel (T = 2^floor(log2 n) = 4 threads, thread 0 scanning
    rows 0 and 4) picks row 4 as well: below 2 T rows the two rules order ties identically (bit reversal of k mod T, then k div T, is the bit
    reversal over one more bit), and n < 2 T always holds for T by n."""
    pts = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], F)
    assert R.fps_segment(pts, 2).tolist() == [0, 4]
    assert R.fps_segment(pts, 5).tolist() == [0, 4, 2, 1, 3]
    from oracle import pointnet2 as op2
    assert np.asarray(op2.farthest_point_sampling(pts, 5)).tolist() == [0, 4, 2, 1, 3]


def _key_form(pts, m, log2t=10):
    """argmax of (distance, then smallest (bitreverse(k mod 2^log2t), k div 2^log2t)): the closed form the kernels use"""
    n = len(pts)
    k = np.arange(n)
    lo = k & ((1 << log2t) - 1)
    rev = np.array([int(format(int(v), f"0{log2t}b")[::-1], 2) for v in lo])
    tie = rev * (1 << 21) + (k >> log2t)
    temp = np.full(n, 1e10, F)
    out, old = [0], 0
    for _ in range(1, m):
        d = (pts - pts[old]).astype(F)
        s = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
        s = (s + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        temp = np.minimum(s, temp)
        cand = np.nonzero(temp == temp.max())[0]
        old = int(cand[np.argmin(tie[cand])])
        out.append(old)
    return out


def test_fps_tree_equals_key_form_on_ties():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 5, 63, 64, 65, 700, 1023, 1024, 1025, 2500):
        pts = rng.integers(-2, 3, size=(n, 3)).astype(F)          # a coarse lattice: every round is full of ties
        m = min(n, 24)
        assert R.fps_segment(pts, m).tolist() == _key_form(pts, m), n


def test_fps_more_samples_than_points():
    pts = np.array([[0, 0, 0], [3, 0, 0], [1, 0, 0]], F)
    assert R.fps_segment(pts, 6).tolist() == [0, 1, 2, 0, 0, 0]    # all running distances 0: slot 0 holds row 0 and is the lowest slot
    assert R.fps_segment(pts[:1], 3).tolist() == [0, 0, 0]
    dup = np.ones((70, 3), F)
    assert R.fps_segment(dup, 4).tolist() == [0, 0, 0, 0]


def test_stack_fps_offsets():
    rng = np.random.default_rng(9)
    xyz = rng.normal(size=(40, 3)).astype(F)
    got = R.stack_fps(xyz, [10, 0, 30], [4, 0, 6])
    assert got[:4].tolist() == R.fps_segment(xyz[:10], 4).tolist()
    assert got[4:].tolist() == (10 + R.fps_segment(xyz[10:], 6)).tolist()
