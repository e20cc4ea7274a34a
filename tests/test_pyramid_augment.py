"""csrc/augment_pyramid.hip and random_local_pyramid_aug in seevcn_amd.pcdet.datasets.augmentor on the GPU against the numpy restatement
(tests/pyramid_augment_reference.py, itself held to the reference's own functions in tests/test_pyramid_augment_reference.py).

Every point of every case is at least 1e-6 m from every face plane (the generator rejects the others; the CPU test shows it), so membership is
decided alike by any float64 evaluation: keep flags, counts and every copied row must equal the restatement exactly.  Swapped rows are float32
with one rounding per operation on both sides (the library is built with contraction off and IEEE division): equal bits are asked for there too.
The restatement's results are computed once per case and shared."""
import numpy as np
import pytest

import pyramid_augment_reference as PR

F = np.float32
CLASSES = ["Car", "Pedestrian"]
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _with_cfg(case, cfg):
    return dict(case, cfg=dict(cfg))


def _want(name, cfg=None):
    """(points, draws, next uniform) of the restatement for a case, optionally under another case's settings; computed once."""
    def make():
        case = PR.cases()[name] if cfg is None else _with_cfg(PR.cases()[name], cfg)
        pts, draws, rng = PR.run_case(case)
        return pts, draws, rng.uniform()
    return _cached(("want", name, None if cfg is None else tuple(sorted(cfg.items()))), make)


def _batch(cases, dev, point_slots=None, box_slots=None):
    """A DeviceBatch of the cases as they are: rows with cls == -2 stay in place (they do not exist), dead points get keep = 0."""
    from seevcn_amd.pcdet.datasets.augmentor import DeviceBatch
    batch = DeviceBatch.from_scenes([_t(c["points"], dev) for c in cases], [_t(c["boxes"], dev) for c in cases], [c["cls"] for c in cases],
                                    point_slots, box_slots)
    keep = batch.keep.cpu().numpy()
    for b, c in enumerate(cases):
        first = batch.pt_offsets[b] + batch.point_slots[b]
        keep[first:first + len(c["points"])] = ~c["dead"]
    batch.keep.copy_(_t(keep, dev))
    return batch


def _rows(batch, cases):
    return [batch.box_offsets[b] + np.nonzero(c["cls"] != -2)[0] for b, c in enumerate(cases)]


def _compare_scenes(out, wants):
    """The compacted batch against the restatement: per scene the same rows in the same order with equal bits."""
    pts = out["points"].cpu().numpy()
    assert out["points_per_scene"].tolist() == [len(w) for w in wants]
    at = 0
    for b, w in enumerate(wants):
        got = pts[at:at + len(w)]
        assert (got[:, 0] == b).all()
        assert np.array_equal(_bits(got[:, 1:]), _bits(w)), f"scene {b}"
        at += len(w)


def _same_draws(got, want):
    assert [n for n, _ in got] == [n for n, _ in want] == list(PR.DRAW_NAMES)
    for (name, a), (_, b) in zip(got, want):
        if name == "pyramid_sparsify_choice":
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), name
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b)), name


# ---------------------------------------------------------------------------------------------------------- the kernels, by name
@pytest.mark.gpu
def test_pyramids_are_the_restatements_bit_for_bit(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    rs = np.random.RandomState(5)
    boxes = np.concatenate([c["boxes"] for c in PR.cases().values()] + [np.zeros((300, 7), F)])
    n = len(boxes) - 300                                         # 300 more with any heading at all: the device and the restatement round alike
    boxes[n:, 0:2], boxes[n:, 2] = rs.uniform(-70, 70, (300, 2)), rs.uniform(-2, 1, 300)
    boxes[n:, 3:6], boxes[n:, 6] = rs.uniform(0.4, 10, (300, 3)), rs.uniform(-3.2, 3.2, 300)
    wide = np.concatenate([boxes, rs.uniform(-1, 1, (len(boxes), 2)).astype(F)], axis=1)      # velocity columns are not read
    for b in (boxes, wide):
        got = A.get_pyramids(_t(b, cuda)).cpu().numpy()
        assert got.shape == (len(b), 6, 15) and np.array_equal(_bits(got), _bits(PR.get_pyramids(b[:, :7])))


@pytest.mark.gpu
def test_counts_and_membership_of_every_pyramid(cuda):
    """Three scenes at once, the 3 000-row one first: per pyramid the live members, and per point the faces that hold it; rows with cls == -2 and
    dead points do not count, spare rows in front neither."""
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    cases = [PR.cases()[k] for k in ("large", "classes", "no_boxes", "overlap")]
    batch = _batch(cases, cuda, point_slots=[5, 0, 3, 0], box_slots=[2, 1, 0, 0])
    A.reset_counters()
    counts, member = A.points_in_pyramids_mask(batch, member=True)
    assert A.COUNTERS == {"library_calls": 1, "host_reads": 0}
    counts, member = counts.cpu().numpy(), member.cpu().numpy()
    some = np.zeros(batch.total_boxes, np.int64)
    some[batch.box_offsets[0]:batch.box_offsets[0] + 6] = [1, 2, 4, 0, 63, 40]
    part = A.points_in_pyramids_mask(batch, some).cpu().numpy()
    for b, c in enumerate(cases):
        exists = c["cls"] != -2
        masks = PR.points_in_pyramids_mask(c["points"], PR.get_pyramids(c["boxes"])).reshape(len(c["points"]), -1, 6)
        masks = masks & exists[None, :, None] & ~c["dead"][:, None, None]
        b0, p0 = batch.box_offsets[b], batch.pt_offsets[b] + batch.point_slots[b]
        assert np.array_equal(counts[b0:b0 + len(exists)], masks.sum(0))
        assert (counts[b0 + len(exists):(list(batch.box_offsets) + [batch.total_boxes])[b + 1]] == 0).all()      # the spare box rows
        packed = (masks * (1 << np.arange(6))[None, None, :]).sum(-1)
        got = member[p0:p0 + len(c["points"]), :len(exists)]
        assert np.array_equal(got, packed) and (member[batch.pt_offsets[b]:p0] == 0).all()
        if b == 0:
            asked = np.array([[(m >> f) & 1 for f in range(6)] for m in some[b0:b0 + 6]])
            assert np.array_equal(part[b0:b0 + 6], masks.sum(0) * asked) and part[b0 + 6:].sum() == 0
    assert (counts[batch.box_offsets[3]:] .sum() > 0) and ((member[batch.pt_offsets[3]:] != 0).sum(1) >= 2).sum() >= 3   # points in two boxes' pyramids


@pytest.mark.gpu
def test_dropout_by_name(cuda):
    """Rows with cls == -2 get NaN draws; rows of another class (-1) take part."""
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    cases = [PR.cases()[k] for k in ("classes", "large", "small")]
    rs = np.random.RandomState(9)
    for trial in range(2):
        removed = 0
        batch = _batch(cases, cuda, point_slots=[4, 0, 0], box_slots=[1, 0, 2])
        faces, u = np.full(batch.total_boxes, np.nan), np.full(batch.total_boxes, np.nan)
        for b, r in enumerate(_rows(batch, cases)):
            faces[r], u[r] = rs.randint(0, 6, len(r)), rs.uniform(0, 1, len(r))
        before = batch.keep.cpu().numpy().copy()
        A.reset_counters()
        dropped = A.local_pyramid_dropout(batch, faces, u, 0.6)
        assert A.COUNTERS == {"library_calls": 1, "host_reads": 0}
        assert np.array_equal(dropped, np.nan_to_num(u, nan=2.0) <= 0.6) and dropped.sum() >= 3
        keep = batch.keep.cpu().numpy()
        for b, c in enumerate(cases):
            r = batch.box_offsets[b] + np.arange(len(c["boxes"]))
            hit = np.zeros(len(c["points"]), bool)
            for i in np.nonzero(dropped[r])[0]:
                hit |= PR.member(c["points"], PR.get_pyramids(c["boxes"][i:i + 1])[0, int(faces[r[i]])])
            p0 = batch.pt_offsets[b] + batch.point_slots[b]
            assert np.array_equal(keep[p0:p0 + len(hit)].astype(bool), ~c["dead"] & ~hit)
            removed += int((hit & ~c["dead"]).sum())
            assert np.array_equal(keep[batch.pt_offsets[b]:p0], before[batch.pt_offsets[b]:p0])
        assert removed >= 20


@pytest.mark.gpu
def test_a_count_that_differs_from_the_plan_is_an_error(cuda):
    from seevcn_amd import _lib as L
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    case = PR.cases()["sparsify_max5"]
    for wrong in (-1, 1):
        batch = _batch([case], cuda)
        counts = A.read_checked(batch, A.points_in_pyramids_mask(batch)).copy()
        assert counts[0, 1] == 6
        counts[0, 1] += wrong                                    # face 1 of box 0 holds 6 points; the plan is told 5 and 7
        plan = A.plan_pyramid_sparsify(counts, [(np.array([0]), np.array([1]))], 3, [np.random.RandomState(0)])
        assert len(plan["pyr"]) == 1
        A.local_pyramid_sparsify(batch, plan)
        with pytest.raises(L.SeevcnHipError, match="another number of points"):
            A.compact(batch)
    batch = _batch([PR.cases()["swap_max5"]], cuda)
    counts = A.read_checked(batch, A.points_in_pyramids_mask(batch)).copy()
    plan = A.plan_pyramid_swap(counts + 1, [np.arange(3)], [np.ones(3, bool)], 5, [np.random.RandomState(0)])
    assert len(plan["pairs"]) == 3
    before = batch.keep.cpu().numpy()[:batch.total_points]
    A.local_pyramid_swap(batch, plan)
    with pytest.raises(L.SeevcnHipError, match="another number of points"):
        A.read_checked(batch, batch.box_cls[:3])
    after = batch.keep.cpu().numpy()
    assert np.array_equal(after[:len(before)], before) and (after[len(before):batch.total_points] == 0).all()   # nothing is written on a mismatch


# ---------------------------------------------------------------------------------------------------------- the entry on a batch built by hand
def _augmentor(cfg, **kw):
    from seevcn_amd.pcdet.datasets.augmentor import BatchDataAugmentor
    return BatchDataAugmentor(None, [dict(cfg, NAME="random_local_pyramid_aug")], CLASSES, **kw)


GROUPS = {
    # the 3 000-row scene (ranks cross a dozen chunks), the 70-row one, rows of other classes and rows that do not exist, dead points everywhere
    "mixed": (("large", "small", "classes", "no_boxes"), None, ([6, 0, 2, 0], [1, 0, 3, 0])),
    "max0": (("sparsify_max0", "swap_max0", "small"), {"DROP_PROB": 0.0, "SPARSIFY_PROB": 0.5, "SPARSIFY_MAX_NUM": 0, "SWAP_PROB": 1.0, "SWAP_MAX_NUM": 0}, None),
    "max5": (("sparsify_max5", "swap_max5", "all_sparsified", "self_swap", "shared_partner", "overlap"),
             {"DROP_PROB": 0.0, "SPARSIFY_PROB": 0.5, "SPARSIFY_MAX_NUM": 5, "SWAP_PROB": 1.0, "SWAP_MAX_NUM": 5}, None),
    "max50": (("sparsify_max50", "swap_max50", "large"), {"DROP_PROB": 0.1, "SPARSIFY_PROB": 0.5, "SPARSIFY_MAX_NUM": 50, "SWAP_PROB": 1.0, "SWAP_MAX_NUM": 50},
              ([0, 9, 0], [0, 0, 2])),
    "columns3": (("columns3", "columns3_swap"), {"DROP_PROB": 0.4, "SPARSIFY_PROB": 0.7, "SPARSIFY_MAX_NUM": 5, "SWAP_PROB": 0.0, "SWAP_MAX_NUM": 5}, None),
    "columns5": (("columns5",), None, ([3], [1])),
    # every box drops a face: sparsify and swap draw nothing; sparsify takes every box: the swap's uniform draws nothing
    "all_dropped": (("all_dropped", "no_boxes"), None, None),
    "all_sparsified": (("all_sparsified", "small"), None, ([0, 2], [1, 0])),
}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_entry_on_a_hand_built_batch(cuda, group):
    """_run_pyramid on a DeviceBatch with dead points, spare rows in front and rows that do not exist, then the one compaction: rows, order, draws
    and the stream's position equal the restatement's; boxes never change."""
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    names, cfg, slots = GROUPS[group]
    cfg = PR.cases()[names[0]]["cfg"] if cfg is None else cfg
    cases = [_with_cfg(PR.cases()[k], cfg) for k in names]
    wants = [_want(k, cfg) for k in names]
    batch = _batch(cases, cuda, *(slots or (None, None)))
    boxes_before = batch.boxes.clone()
    rngs = [np.random.RandomState(c["seed"]) for c in cases]
    A.reset_counters()
    draws = _augmentor(cfg)._run_pyramid(batch, dict(cfg), _rows(batch, cases), rngs, None)
    assert A.COUNTERS["host_reads"] <= 2 and A.COUNTERS["library_calls"] <= 5
    out = A.compact(batch)
    _compare_scenes(out, [w[0] for w in wants])
    for d, w, rng in zip(draws, wants, rngs):
        _same_draws(d, w[1])
        assert rng.uniform() == w[2]
    assert (batch.boxes == boxes_before).all()
    if group == "mixed":
        assert len(wants[0][0]) != int((~cases[0]["dead"]).sum())
    first = dict(draws[0])
    if group == "all_dropped":
        assert len(first["pyramid_drop_u"]) == 3 and len(first["pyramid_sparsify_u"]) == 0 == len(first["pyramid_swap_u"])
        assert A.COUNTERS["host_reads"] == 1                     # no counts were needed: the compaction's read alone
    if group == "all_sparsified":
        assert len(first["pyramid_sparsify_u"]) == 3 and len(first["pyramid_sparsify_choice"]) >= 1 and len(first["pyramid_swap_u"]) == 0


# ---------------------------------------------------------------------------------------------------------- the queue
def _scene(case, dev):
    """A case as a dataset sample: dead points are left out; a row with cls == -2 holds too few points for MIN_POINTS_OF_GT, one with -1 is of a
    class the detector does not train on."""
    names = np.array([CLASSES[c] if c >= 0 else "Van" for c in case["cls"]])
    return dict(points=_t(case["points"][~case["dead"]], dev), gt_boxes=_t(case["boxes"], dev), gt_names=names,
                num_points_in_gt=np.where(case["cls"] == -2, 0, 99))


SETTINGS = {"DROP_PROB": 0.3, "SPARSIFY_PROB": 0.5, "SPARSIFY_MAX_NUM": 5, "SWAP_PROB": 0.6, "SWAP_MAX_NUM": 5}


@pytest.mark.gpu
@pytest.mark.parametrize("names", [("classes",), ("classes", "small", "overlap")], ids=["B1", "B3"])
def test_queue_forward_replay_and_counters(cuda, names):
    import torch
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, reset_counters
    cases = [_with_cfg(PR.cases()[k], SETTINGS) for k in names]
    wants = [_want(k, SETTINGS) for k in names]
    aug = _augmentor(SETTINGS)
    rngs = [np.random.RandomState(c["seed"]) for c in cases]
    reset_counters()
    out = aug.forward([_scene(c, cuda) for c in cases], rng=rngs)
    counters = dict(COUNTERS)
    assert counters["host_reads"] == 3                           # the sparsify counts, the swap counts, the final counts
    _compare_scenes(out, [w[0] for w in wants])
    for d, w, rng, c in zip(out["draws"], wants, rngs, cases):
        _same_draws(d, w[1])
        assert rng.uniform() == w[2]
    gt = out["gt_boxes"].cpu().numpy()
    for b, c in enumerate(cases):
        kept = c["cls"] >= 0
        assert np.array_equal(_bits(gt[b, :kept.sum(), :7]), _bits(c["boxes"][kept])) and (gt[b, :kept.sum(), 7] == c["cls"][kept] + 1).all()
    reset_counters()
    again = aug.forward([_scene(c, cuda) for c in cases], draws=out["draws"])
    assert torch.equal(again["points"], out["points"]) and dict(COUNTERS) == counters
    _CACHE[("counters", len(names))] = counters
    if ("counters", 1) in _CACHE and ("counters", 3) in _CACHE:
        assert _CACHE[("counters", 1)] == _CACHE[("counters", 3)]
    with pytest.raises(ValueError, match="one numpy RandomState per scene"):
        aug.forward([_scene(c, cuda) for c in cases], rng=np.random.RandomState(0))
    short = [list(d) for d in out["draws"]]
    short[0][0] = ("pyramid_drop_face", short[0][0][1][:-1])
    with pytest.raises(ValueError, match="pyramid_drop_face"):
        aug.forward([_scene(c, cuda) for c in cases], draws=short)


@pytest.mark.gpu
def test_queue_behind_a_world_dropout_and_before_world_transforms(cuda):
    """The pyramid's per-box draws behind random_world_frustum_dropout use that boundary's read; the entries behind it go on from the same streams.
    Checked against the pieces: the dropout's survivors through the restatement, then the flip on the result."""
    from seevcn_amd.pcdet.datasets.augmentor import BatchDataAugmentor, COUNTERS, reset_counters
    case = _with_cfg(PR.cases()["classes"], SETTINGS)
    queue = [{"NAME": "random_world_frustum_dropout", "INTENSITY_RANGE": [0.0, 0.0], "DIRECTION": ["top"]},
             dict(SETTINGS, NAME="random_local_pyramid_aug"), {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]}]
    aug = BatchDataAugmentor(None, queue, CLASSES)
    assert [len(s) for s in aug.stages] == [1, 1, 1]
    rng, replay = np.random.RandomState(77), np.random.RandomState(77)
    reset_counters()
    out = aug.forward([_scene(case, cuda)], rng=[rng])
    reads = COUNTERS["host_reads"]
    assert replay.uniform(0.0, 0.0) == 0.0                      # intensity 0: the threshold is the maximum itself, the strict < drops the topmost
    pts = case["points"][~case["dead"]]
    assert (case["boxes"][:, 2] < pts[:, 2].max()).all()         # no box centre is up there: every box stays
    pts = pts[pts[:, 2] < pts[:, 2].max()]
    want, draws = PR.random_local_pyramid_aug(case["boxes"][case["cls"] != -2], pts, SETTINGS, replay)
    want = want.copy()
    if bool(replay.choice([False, True], replace=False, p=[0.5, 0.5])):
        want[:, 1] = -want[:, 1]
    assert rng.uniform() == replay.uniform()
    assert np.array_equal(_bits(out["points"].cpu().numpy()[:, 1:]), _bits(want))
    assert [n for n, _ in out["draws"][0]] == ["world_dropout_top"] + list(PR.DRAW_NAMES) + ["flip_x"]
    _same_draws(out["draws"][0][1:-1], draws)
    d = dict(draws)
    # the dropout's boundary and the final counts; a pyramid read only where the host cannot know that no scene needs it
    assert reads == 2 + int((d["pyramid_sparsify_u"] <= SETTINGS["SPARSIFY_PROB"]).any()) + int((d["pyramid_swap_u"] <= SETTINGS["SWAP_PROB"]).any())
    assert reads >= 3


@pytest.mark.gpu
def test_swap_needs_four_columns_when_the_batch_is_formed(cuda):
    case = PR.cases()["columns3_swap"]
    with pytest.raises(ValueError, match="exactly 4 columns"):
        _augmentor(case["cfg"]).forward([_scene(case, cuda)], rng=[np.random.RandomState(0)])
    for name in ("columns3", "columns5"):                       # dropout and sparsify alone: any C >= 3
        c = PR.cases()[name]
        out = _augmentor(c["cfg"]).forward([_scene(c, cuda)], rng=[np.random.RandomState(c["seed"])])
        _compare_scenes(out, [_want(name)[0]])
