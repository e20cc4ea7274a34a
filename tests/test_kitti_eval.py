"""GPU checks of the KITTI evaluation kernels (csrc/kitti_eval.hip) and the package above them against the float64 restatement
(tests/kitti_eval_reference.py) and the golden produced by the reference's own eval.py (tests/golden/kitti_eval.npz)."""
import os

import numpy as np
import pytest

import kitti_eval_inputs as I
import kitti_eval_reference as K

pytestmark = pytest.mark.gpu

SEGMENTS = [(0, 0), (0, 3), (3, 0), (1, 1), (63, 5), (64, 64), (65, 3), (150, 70)]          # (n_dt, n_gt): rows, columns of one launch
CRITERIA = (-1, 0, 1, 2)
PI = float(np.float32(np.pi))


def special_pairs():
    """(row box, column box, kind) as (x, y, z, l, h, w, ry) pairs, every pair around its own centre, 40 m from the next so that only the pair itself
    overlaps.  kind "exact": the pair sits ON a test of the algorithm (identical, touching, a corner on an edge) with binary-exact coordinates and
    angle 0, so fp32 and float64 both compute without rounding and take the same branches.  kind "fragile": identical ROTATED boxes -- every corner
    lies on the other box's edges and whether `adap >= 0` holds for it hangs on the rounding of a dot product that is zero in exact arithmetic, in
    fp32 and in float64 alike (the float64 restatement returns 0 for this pair, an fp32 evaluation 1 / 3); it presents more than 8 candidates, so it
    is kept for the capacity rule and held to "finite, within [0, 1]" only."""
    pairs = []

    def add(a, b, kind="generic", centre=None):
        n = len(pairs)
        c = np.array([70.0 + 40.0 * (n % 3), 1.5, 80.0 + 40.0 * (n // 3)] if centre is None else centre)          # the first at (70, 80)
        row, col = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
        row[:3] += c
        col[:3] += c
        pairs.append((row, col, kind))

    car = [3.9, 1.5, 1.6]
    add([0, 0, 0, 4, 1.5, 2, 0.0], [0, 0, 0, 4, 1.5, 2, 0.0], "exact")                           # identical, at (70, 80)
    add([0, 0, 0, 4, 1.5, 4, 0.0], [0, 0, 0, 4, 1.5, 4, PI / 4])                                 # concentric squares at 45 degrees: an octagon
    add([0, 0, 0, 4, 1.5, 2, 0.0], [0.25, 0, 0.125, 2, 1.0, 1, 0.0], "exact")                    # contained, axis aligned
    add([0, 0, 0] + car + [0.4], [0.2, 0.1, -0.1, 1.5, 1.2, 0.7, 1.1])                           # contained, rotated
    add([0, 0, 0, 4, 1.5, 2, 0.0], [4, 0, 0, 4, 1.5, 2, 0.0], "exact")                           # edge touching (shared short edge)
    add([0, 0, 0, 4, 1.5, 2, 0.0], [0, 0, 2, 4, 1.5, 2, 0.0], "exact")                           # edge touching (shared long edge)
    add([0, 0, 0, 4, 1.5, 2, 0.0], [2, 0, -0.5, 2, 1.5, 1, 0.0], "exact")                        # a corner of one on an edge of the other
    add([0, 0, 0] + car + [0.2], [6.0, 0, 3.0] + car + [-0.5])                                   # disjoint, close
    add([0, 0, 0] + car + [0.0], [0.5, 0.1, 0.3] + car + [PI / 2])                               # angles at multiples of pi / 2
    add([0, 0, 0] + car + [PI], [0.4, 0.0, -0.2, 3.5, 1.4, 1.5, 0.35])
    add([0, 0, 0] + car + [-PI / 2], [0.3, 0.2, 0.2, 4.2, 1.6, 1.7, 3 * PI / 2 + 0.4])
    add([0, 0, 0, 0.05, 0.04, 0.03, 0.3], [0.01, 0.0, 0.005, 0.06, 0.05, 0.04, 1.0], centre=[1.0, 1.5, 2.0])      # sub-decimetre boxes
    add([0, 0, 0, 0.08, 0.06, 0.05, -0.7], [0.0, 0.01, 0.0, 0.04, 0.05, 0.09, 0.2], centre=[-3.0, 1.5, 4.0])
    add([0, 0, 0, 0.8, 1.75, 0.6, 0.5], [0.1, 0.05, -0.1, 0.75, 1.7, 0.65, 0.9])                 # pedestrians
    add([0, 0, 0, 10.0, 3.2, 2.6, 1.3], [1.0, 0.3, 0.8, 9.0, 3.0, 2.5, 1.05])                    # trucks, a shallow crossing
    add([0, 0, 0] + car + [0.3], [0.3, -1.0, 0.2] + car + [0.5])                                 # BEV overlap, partial height overlap
    add([0, 0, 0] + car + [0.3], [0.3, -2.0, 0.2] + car + [0.5])                                 # BEV overlap, no height overlap
    add([0, 0, 0] + car + [0.3], [0, 0, 0] + car + [0.3], "fragile")                             # identical and rotated: more than 8 candidates
    return pairs


def overlap_problem():
    """Row / column boxes (7 floats) for SEGMENTS.  The special pairs sit on the diagonal of the (64, 64) segment; everything else is seeded random
    boxes over a 200 m field, so that each segment holds overlapping, touching-distance and far pairs."""
    rng = np.random.RandomState(7)
    pairs = special_pairs()

    def random_boxes(n, near=None):
        out = np.zeros((n, 7))
        out[:, 0], out[:, 1], out[:, 2] = rng.uniform(-60, 140, n), rng.uniform(1.0, 2.0, n), rng.uniform(0, 200, n)
        if near is not None and len(near):
            pick = rng.randint(len(near), size=n)
            close = rng.rand(n) < 0.6
            out[close, :3] = near[pick[close], :3] + rng.randn(close.sum(), 3) * [1.0, 0.3, 1.0]
        out[:, 3], out[:, 4], out[:, 5] = rng.uniform(0.5, 5, n), rng.uniform(1.0, 2.5, n), rng.uniform(0.4, 2.5, n)
        out[:, 6] = rng.uniform(-np.pi, np.pi, n)
        return out

    rows, cols = [], []
    for n_dt, n_gt in SEGMENTS:
        c = random_boxes(n_gt)
        r = random_boxes(n_dt, c)
        if (n_dt, n_gt) == (64, 64):
            c[:, 2] += 1000.0                                # the random part of this segment stays clear of the special pairs...
            r[:, 2] += 1000.0
            for i, (a, b, _) in enumerate(pairs):            # ...which take the head of its diagonal
                r[i], c[i] = a, b
            assert len(pairs) <= 64
        rows.append(r), cols.append(c)
    f32 = lambda a: np.concatenate(a, 0).astype(np.float32).astype(np.float64)          # what both sides start from
    return f32(rows), f32(cols), np.array([s[0] for s in SEGMENTS]), np.array([s[1] for s in SEGMENTS])


def image_boxes(b7):
    """An image box for every 3-D box of the overlap problem (quarter pixels: exact in fp32)."""
    u, v = 600 + 4 * (b7[:, 0] - 40), 180 + 0.5 * (b7[:, 2] % 40)
    w, h = 12 * b7[:, 3], 20 * b7[:, 4]
    return np.round(np.stack([u - w / 2, v - h / 2, u + w / 2, v + h / 2], 1) * 4) / 4


@pytest.fixture(scope="module")
def pkg(cuda, hip_lib):
    from seevcn_amd.pcdet.datasets.kitti.kitti_object_eval_python import eval as E, rotate_iou as R
    return E, R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "kitti_eval.npz"))


@pytest.fixture(scope="module")
def annos(golden):
    gt, dt = I.unpack(golden, "gt"), I.unpack(golden, "dt")
    return gt, {"alpha": dt, "noalpha": [dict(a, alpha=np.full_like(a["alpha"], -10.0)) for a in dt]}


@pytest.fixture(scope="module")
def problem():
    return overlap_problem()


def _segments(counts_r, counts_c):
    ro, co = np.concatenate([[0], np.cumsum(counts_r)]), np.concatenate([[0], np.cumsum(counts_c)])
    return [(slice(ro[s], ro[s + 1]), slice(co[s], co[s + 1])) for s in range(len(counts_r))]


@pytest.mark.parametrize("metric", [1, 2])
def test_rotated_overlaps_within_the_derived_bound(pkg, problem, metric):
    """Every pair of every segment, criteria -1, 0, 1, 2, one launch per criterion, against the float64 restatement within the PAIR's bound."""
    E, R = pkg
    rows, cols, nr, nc = problem
    cut = (lambda b: b[:, [0, 2, 3, 5, 6]]) if metric == 1 else (lambda b: b)
    worst = 0.0
    for criterion in CRITERIA:
        R.reset_counters()
        blocks = R.ragged_overlaps(cut(rows), cut(cols), nr, nc, metric, criterion)
        assert R.COUNTERS == {"library_calls": 1, "host_reads": 1}
        assert [b.shape for b in blocks] == SEGMENTS
        for (rs, cs), got in zip(_segments(nr, nc), blocks):
            r, c = rows[rs], cols[cs]
            want = K.bev_box_overlap(cut(r), cut(c), criterion) if metric == 1 else K.d3_box_overlap(r, c, criterion)
            assert np.isfinite(got).all()
            fragile = [n for n, p in enumerate(special_pairs()) if p[2] == "fragile"] if got.shape == (64, 64) else []
            for i, j in zip(*np.nonzero((want != 0) | (got != 0))):
                if i == j and i in fragile:                        # see special_pairs(): held to "finite, a ratio within [0, 1]"
                    assert criterion == 2 or 0 <= got[i, j] <= 1 + 1e-5
                    continue
                if metric == 1:
                    bound = K.rotated_overlap_bound(c[j][[0, 2, 3, 5, 6]], r[i][[0, 2, 3, 5, 6]], criterion)
                else:
                    bound = K.d3_overlap_bound(r[i], c[j], criterion)
                diff = abs(float(got[i, j]) - want[i, j])
                scale = max(1.0, abs(want[i, j]))                  # criterion 2 of metric 1 is an area, not a ratio
                assert diff <= bound * scale + 2 * K.U32 * scale, (metric, criterion, i, j, r[i], c[j], got[i, j], want[i, j], bound)
                if criterion == -1:
                    worst = max(worst, diff)
    print("metric %d: largest |kernel - float64 restatement| at criterion -1: %.3e" % (metric, worst))


def test_special_pairs_values(pkg):
    """The named geometric cases, against closed-form values where there is one."""
    E, R = pkg
    pairs = special_pairs()
    rows, cols = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    bev = R.rotate_iou_gpu_eval(rows[:, [0, 2, 3, 5, 6]], cols[:, [0, 2, 3, 5, 6]], -1)
    assert bev.dtype == np.float32 and bev.shape == (len(pairs), len(pairs))
    d = np.diag(bev)
    assert d[0] == 1.0                                                             # identical, exact arithmetic
    octagon = 16 * 2 * (np.sqrt(2) - 1)                                            # two concentric 4 x 4 squares at 45 degrees
    assert abs(d[1] - octagon / (32 - octagon)) < 1e-4
    assert d[2] == np.float32(2.0 / 8.0)                                           # contained, exact arithmetic
    assert d[4] == 0 and d[5] == 0                                                 # touching edges share no area
    assert d[6] == np.float32(1.0) / np.float32(9.0)                               # the 1 x 1 piece of the 2 x 1 box inside the 4 x 2 box
    assert d[7] == 0 and 0 <= d[-1] <= 1 + 1e-5
    off = bev - np.diag(d)
    assert (off == 0).all()                                                        # the pairs are 40 m apart
    d3 = np.diag(E.d3_box_overlap(rows, cols))
    assert d3[0] == 1.0 and d3[-2] == 0 and 0 < d3[-3] < d[-3]
    area = R.rotate_iou_gpu_eval(rows[:1, [0, 2, 3, 5, 6]], cols[:1, [0, 2, 3, 5, 6]], 2)
    assert area[0, 0] == 8.0


def test_image_overlaps(pkg, problem):
    E, R = pkg
    rows, cols, nr, nc = problem
    br, bc = image_boxes(rows), image_boxes(cols)
    for criterion in (-1, 0, 1):
        blocks = R.ragged_overlaps(br, bc, nr, nc, 0, criterion)
        n = 0
        for (rs, cs), got in zip(_segments(nr, nc), blocks):
            want = K.image_box_overlap(br[rs], bc[cs], criterion)
            assert np.array_equal(want > 0, got > 0)
            for i, j in zip(*np.nonzero(want > 0)):
                assert abs(got[i, j] - want[i, j]) <= K.image_overlap_bound(br[rs][i], bc[cs][j]) + 2 * K.U32
                n += 1
        assert n > 50
    with pytest.raises(ValueError):
        R.ragged_overlaps(br, bc, nr, nc, 0, 2)
    dense = E.image_box_overlap(br[:7], bc[:5])
    assert dense.dtype == br.dtype and dense.shape == (7, 5)
    assert E.image_box_overlap(br[:0], bc[:5]).shape == (0, 5) and E.bev_box_overlap(np.zeros((0, 5)), np.zeros((3, 5))).shape == (0, 3)


def test_overlaps_against_the_reference_fp32(pkg, golden, annos):
    """The kernel against the golden's overlaps (the reference's own statements on float32 arrays): twice the pair's bound, since both sides round."""
    E, R = pkg
    gt, dts = annos
    for metric in (0, 1, 2):
        blocks, parted, total_dt_num, total_gt_num = E.calculate_iou_partly(dts["alpha"], gt, metric)
        assert parted is None and total_dt_num.tolist() == [len(a["name"]) for a in dts["alpha"]]
        ref, pos, worst = golden["overlaps_%d" % metric], 0, 0.0
        for g, d, block in zip(gt, dts["alpha"], blocks):
            assert block.shape == (len(d["name"]), len(g["name"]))
            want = ref[pos:pos + block.size].reshape(block.shape)
            pos += block.size
            assert np.array_equal(want > 0, block > 0)
            d3, g3 = K.metric_boxes(d, 2), K.metric_boxes(g, 2)
            for i, j in zip(*np.nonzero(want > 0)):
                bound = (K.image_overlap_bound(d["bbox"][i], g["bbox"][j]) if metric == 0 else
                         K.rotated_overlap_bound(g3[j][[0, 2, 3, 5, 6]], d3[i][[0, 2, 3, 5, 6]]) if metric == 1 else K.d3_overlap_bound(d3[i], g3[j]))
                diff = abs(block[i, j] - want[i, j])
                assert diff <= 2 * bound, (metric, i, j, diff, bound)
                worst = max(worst, diff)
        assert pos == len(ref)
        print("metric %d: largest |kernel - reference on float32 arrays| over the fixture: %.3e" % (metric, worst))


def _compare_detail(detail, loop, combos):
    for c, key in enumerate(combos):
        want = loop[key]
        n = int(detail["tp_count"][c])
        assert n == len(want["tp_scores"]), key
        assert np.array_equal(detail["tp_scores"][c, :n], np.sort(want["tp_scores"])[::-1]), key          # bits
        nt = int(detail["num_thresholds"][c])
        assert nt == len(want["thresholds"]), key
        assert np.array_equal(detail["thresholds"][c, :nt], want["thresholds"]), key                       # bits
        assert np.array_equal(detail["table"][c, :nt, :3], want["pr"][:, :3]), key                         # tp, fp, fn: integers
        np.testing.assert_allclose(detail["table"][c, :nt, 3], want["pr"][:, 3], rtol=1e-12, atol=0, err_msg=str(key))
        assert (detail["table"][c, nt:] == 0).all()


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_matching_equals_the_sequential_loop(pkg, annos, metric):
    """Both passes on the kernel's OWN overlaps against the sequential restatement on the same values: every (frame, combination, threshold) of the
    fixture, metric 0 with DontCare and AOS.  Integers and bits equal; the similarity sums to 1e-12; two runs give equal bits."""
    E, R = pkg
    gt, dts = annos
    min_overlaps = E.official_min_overlaps()[:, :, [0, 1, 2]]
    detail = {}
    ret = E.eval_class(gt, dts["alpha"], [0, 1, 2], [0, 1, 2], metric, min_overlaps, compute_aos=metric == 0, detail=detail)
    off = detail["ov_off"]
    blocks = [detail["overlaps"][off[f]:off[f + 1]].reshape(len(dts["alpha"][f]["name"]), len(gt[f]["name"])) for f in range(len(gt))]
    loop = {}
    want = K.eval_class(gt, dts["alpha"], [0, 1, 2], [0, 1, 2], metric, min_overlaps, compute_aos=metric == 0, overlaps=blocks, detail=loop)
    combos = [(m, l, k) for m in range(3) for l in range(3) for k in range(2)]
    _compare_detail(detail, loop, combos)
    assert sum(len(v["thresholds"]) for v in loop.values()) > 100
    for k in ("precision", "recall", "orientation"):
        np.testing.assert_allclose(ret[k], want[k], rtol=1e-12, atol=0)
    again = {}
    E.eval_class(gt, dts["alpha"], [0, 1, 2], [0, 1, 2], metric, min_overlaps, compute_aos=metric == 0, detail=again)
    for k in ("overlaps", "tp_scores", "tp_count", "thresholds", "num_thresholds", "table"):
        assert np.array_equal(detail[k], again[k]), k


def _loop_on_matrices(frames, min_overlap, num_valid, metric=1):
    """The sequential reference on bare overlap matrices: frames = [(overlap (n_dt, n_gt), scores, ignored_det, ignored_gt)]."""
    tp_scores, datas = [], []
    for ov, sc, igd, igg in frames:
        gt_datas, dt_datas = np.zeros((ov.shape[1], 5)), np.zeros((ov.shape[0], 6))
        dt_datas[:, -1] = sc
        datas.append((gt_datas, dt_datas))
        tp_scores += K.compute_statistics_jit(ov, gt_datas, dt_datas, igg, igd, np.zeros((0, 4)), metric, min_overlap, 0.0, False)[4].tolist()
    thresholds = np.array(K.get_thresholds(np.array(tp_scores), num_valid))
    pr = np.zeros((len(thresholds), 4))
    for (ov, sc, igd, igg), (gt_datas, dt_datas) in zip(frames, datas):
        for t, th in enumerate(thresholds):
            pr[t, :3] += K.compute_statistics_jit(ov, gt_datas, dt_datas, igg, igd, np.zeros((0, 4)), metric, min_overlap, th, True)[:3]
    return dict(tp_scores=np.array(tp_scores), thresholds=thresholds, pr=pr)


def adversarial_frames():
    """Overlap matrices given directly, so that ties are exact.  The named cases first, then seeded frames whose overlaps and scores are drawn from a few
    values (ties everywhere) with every mix of ignored flags, up to 150 detections (three strides of a wave) a frame."""
    f32 = lambda a: np.array(a, dtype=np.float32)
    frames = [
        (f32([[0.6], [0.6], [0.6]]), [0.5, 0.9, 0.9], [0, 0, 0], [0]),                          # equal overlaps, equal scores: the lowest index of the best
        (f32([[0.8], [0.6]]), [0.3, 0.9], [0, 0], [0]),                                         # pass 1 takes the score, pass 2 the overlap
        (f32([[0.6], [0.9]]), [0.5, 0.4], [1, 0], [0]),                                         # an ignored detection in front of a better unignored one
        (f32([[0.9], [0.6]]), [0.5, 0.4], [0, 1], [0]),                                         # ...and behind it
        (f32([[0.9], [0.6]]), [0.5, 0.4], [1, 1], [0]),                                         # only ignored ones: the first
        (f32([[0.9, 0.7], [0.2, 0.8]]), [0.8, 0.6], [0, 0], [1, 0]),                            # an ignored ground truth absorbs the detection the next one wants
        (f32([[0.9, 0.8], [0.7, 0.1]]), [0.2, 0.9], [0, 0], [0, 0]),                            # a threshold cuts the best candidate of ground truth 0
        (f32([[0.0, 0.3], [0.0, 0.0]]), [0.7, 0.6], [0, 0], [0, 0]),                            # zero overlaps: not above min_overlap = 0
        (f32([[0.5, 0.5, 0.5]] * 4), [0.4, 0.4, 0.3, 0.9], [0, -1, 0, 1], [0, 1, 0]),
        (f32(np.zeros((0, 2))), [], [], [0, 0]),                                                # no detection: two misses
        (f32(np.zeros((2, 0))), [0.5, 0.6], [0, 0], []),                                        # no ground truth: two false positives
    ]
    rng = np.random.RandomState(11)
    for n_dt, n_gt in [(5, 3), (64, 4), (65, 5), (130, 6), (150, 9), (7, 70)] * 4:
        ov = rng.choice(f32([0.0, 0.25, 0.5, 0.5, 0.75, 1.0]), size=(n_dt, n_gt)) * (rng.rand(n_dt, n_gt) < 0.3)
        frames.append((f32(ov), rng.choice([0.1, 0.3, 0.5, 0.7, 0.9], size=n_dt).tolist(), rng.choice([-1, 0, 0, 1], size=n_dt).tolist(),
                       rng.choice([-1, 0, 0, 1], size=n_gt).tolist()))
    return [(ov, np.array(sc, dtype=np.float64), np.array(igd, dtype=np.int64), np.array(igg, dtype=np.int64)) for ov, sc, igd, igg in frames]


def test_adversarial_matching(pkg, cuda):
    import torch
    E, R = pkg
    frames = adversarial_frames()
    min_overlaps = [0.0, 0.25, 0.5, 0.7]
    n_dt, n_gt = np.array([f[0].shape[0] for f in frames]), np.array([f[0].shape[1] for f in frames])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    igg = np.concatenate([f[3] for f in frames]).astype(np.int8)
    num_valid = int((igg == 0).sum())
    out = E.match_on_device(
        up(np.concatenate([f[0].reshape(-1) for f in frames])), up(R.offsets(n_dt)), up(R.offsets(n_gt)), up(R.offsets(n_dt * n_gt)),
        up(np.concatenate([f[1] for f in frames])), up(np.concatenate([f[2] for f in frames]).astype(np.int8)[None]), up(igg[None]),
        up(np.zeros(len(min_overlaps), dtype=np.int32)), up(np.array(min_overlaps)), up(np.full(len(min_overlaps), num_valid, dtype=np.int32)),
        metric=1, detail=True)
    table, num_thresholds, tp_scores, tp_count, thresholds = [t.cpu().numpy() for t in out]
    detail = dict(table=table, num_thresholds=num_thresholds, tp_scores=tp_scores, tp_count=tp_count, thresholds=thresholds)
    loop = {c: _loop_on_matrices(frames, mo, num_valid) for c, mo in enumerate(min_overlaps)}
    _compare_detail(detail, loop, list(range(len(min_overlaps))))
    assert all(len(loop[c]["thresholds"]) > 2 for c in loop)
    assert loop[0]["pr"][:, :3].sum() != loop[1]["pr"][:, :3].sum()                       # min_overlap = 0 really differs from 0.25


def _check_official(E, golden, gt, dets, classes, tag):
    detail = {}
    result, ret_dict = E.get_official_eval_result(gt, dets, classes, PR_detail_dict=detail)
    assert result == str(golden[tag + "_result"])
    assert list(ret_dict.keys()) == golden[tag + "_ret_keys"].tolist()
    np.testing.assert_allclose([float(v) for v in ret_dict.values()], golden[tag + "_ret_values"], rtol=0, atol=1e-9)
    names = {"bbox": (0, "precision"), "bev": (1, "precision"), "3d": (2, "precision"), "aos": (0, "orientation")}
    assert set(detail) == (set(names) if tag.startswith("alpha") else set(names) - {"aos"})
    for k, v in detail.items():
        np.testing.assert_allclose(v, golden["%s_m%d_%s" % ((tag,) + names[k])], rtol=0, atol=1e-9)


@pytest.mark.parametrize("set_name", ["alpha", "noalpha"])
def test_official_result_equals_the_reference(pkg, golden, annos, set_name):
    """get_official_eval_result on the fixture: the reference's strings character for character, ret_dict and the PR arrays to 1e-9."""
    E, R = pkg
    gt, dts = annos
    _check_official(E, golden, gt, dts[set_name], ["Car", "Pedestrian", "Cyclist"], set_name + "_cpc")
    _check_official(E, golden, gt, dts[set_name], ["Car"], set_name + "_car")
    _check_official(E, golden, gt, dts[set_name], [0, 1, 2], set_name + "_cpc")
    _check_official(E, golden, gt, dts[set_name], 0, set_name + "_car")


def test_calls_and_reads_do_not_depend_on_the_number_of_frames(pkg, annos):
    E, R = pkg
    gt, dts = annos
    counts = []
    for sel in (slice(3, 6), slice(None)):
        R.reset_counters()
        E.get_official_eval_result(gt[sel], dts["alpha"][sel], ["Car", "Pedestrian", "Cyclist"])
        counts.append(dict(R.COUNTERS))
    assert counts[0] == counts[1] == {"library_calls": 3 * 4, "host_reads": 3}
    R.reset_counters()
    E.eval_class(gt, dts["alpha"], [0], [0, 1, 2], 2, E.official_min_overlaps()[:, :, [0]])
    assert R.COUNTERS == {"library_calls": 4, "host_reads": 1}


def test_empty_inputs_launch_nothing(pkg, annos):
    """An empty dataset, frames with nothing, only ground truth, only detections, and a class with no valid ground truth anywhere."""
    E, R = pkg
    gt, dts = annos
    mo = E.official_min_overlaps()
    R.reset_counters()
    for g, d in (([], []), (gt[:1], dts["alpha"][:1]), (gt[1:2], dts["alpha"][1:2]), (gt[2:3], dts["alpha"][2:3]), (gt[:3], dts["alpha"][:3])):
        for metric in (0, 1, 2):
            ret = E.eval_class(g, d, [0, 1], [0, 1, 2], metric, mo[:, :, [0, 1]], compute_aos=metric == 0)
            assert all(v.shape == (2, 3, 2, 41) and (v == 0).all() for v in ret.values())
    assert R.COUNTERS == {"library_calls": 0, "host_reads": 0}
    result, ret_dict = E.get_official_eval_result(gt[:3], dts["alpha"][:3], ["Car"])
    assert "bbox AP:0.0000, 0.0000, 0.0000" in result and ret_dict["Car_3d/moderate_R40"] == 0
    no_truck_gt = [dict(g, name=np.where(g["name"] == "Truck", "Van", g["name"])) for g in gt]
    ret = E.eval_class(no_truck_gt, dts["alpha"], [5, 0], [0, 1, 2], 1, mo[:, :, [5, 0]])
    assert (ret["precision"][0] == 0).all() and (ret["recall"][0] == 0).all() and (ret["precision"][1] > 0).any()
    assert E.get_thresholds(np.zeros(0), 5) == []
    scores = np.random.RandomState(3).rand(300)
    assert E.get_thresholds(scores.copy(), 320) == K.get_thresholds(scores.copy(), 320)


def test_refusals(pkg, annos):
    import torch
    import seevcn_amd._lib as L
    E, R = pkg
    gt, dts = annos
    off = torch.tensor([0, 1], dtype=torch.int64)
    with pytest.raises(L.SeevcnHipError):
        R.ragged_overlaps_device(torch.zeros(1, 5), torch.zeros(1, 5), off, off, off, 1, 1, -1)
    with pytest.raises(L.SeevcnHipError):
        E.match_on_device(torch.zeros(1), off, off, off, torch.zeros(1, dtype=torch.float64), torch.zeros(1, 1, dtype=torch.int8),
                          torch.zeros(1, 1, dtype=torch.int8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.float64),
                          torch.ones(1, dtype=torch.int32))
    R.reset_counters()
    bad = E.official_min_overlaps()[:, :, [0]].copy()
    bad[0, 2, 0] = -1e-3
    with pytest.raises(ValueError):
        E.eval_class(gt, dts["alpha"], [0], [0, 1, 2], 2, bad)
    n = E.max_detections_per_frame() + 1
    big = dict(name=np.array(["Car"] * n), bbox=np.tile([0.0, 0, 10, 50], (n, 1)), alpha=np.zeros(n), score=np.linspace(0, 1, n),
               dimensions=np.ones((n, 3)), location=np.zeros((n, 3)), rotation_y=np.zeros(n))
    with pytest.raises(ValueError):
        E.get_official_eval_result([gt[4]], [big], ["Car"])
    assert R.COUNTERS == {"library_calls": 0, "host_reads": 0}
