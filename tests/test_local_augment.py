"""csrc/augment_local.hip and the local / frustum half of seevcn_amd.pcdet.datasets.augmentor on the GPU against the numpy restatement
(tests/local_augment_reference.py, itself held to the reference's own functions in tests/test_local_augment_reference.py).

Every case is shown robust on the CPU when it is built (every tested point at least 1e-3 m from every comparison it meets, every box centre
from the world thresholds), so keep flags and class codes must equal the restatement exactly; moved coordinates are held to its per-element
bound (derived in its header, not fitted), unmoved ones to equal bits."""
import numpy as np
import pytest

import augment_reference as R
import local_augment_reference as LR

F = np.float32
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _batch(scenes, dev):
    """scenes: dicts with boxes, points and optionally cls (default 0) and dead (rows with keep = 0 on entry)."""
    from seevcn_amd.pcdet.datasets.augmentor import DeviceBatch
    batch = DeviceBatch.from_scenes([_t(s["points"], dev) for s in scenes], [_t(s["boxes"], dev) for s in scenes],
                                    [s.get("cls", np.zeros(len(s["boxes"]), np.int32)) for s in scenes])
    dead = np.concatenate([s.get("dead", np.zeros(len(s["points"]), bool)) for s in scenes])
    if dead.any():
        batch.keep[:len(dead)] = _t((~dead).astype(np.int32), dev)
    return batch


def _apply(batch, scenes, poison=np.nan):
    """The scenes' ops (the same names in every scene) on the device: runs of local steps fused, runs of world dropouts fused.  Rows of boxes
    that do not exist get a NaN draw: a kernel that read it would show."""
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    names = [n for n, _ in scenes[0]["ops"]]
    assert all([n for n, _ in s["ops"]] == names for s in scenes)
    i = 0
    while i < len(names):
        local = names[i] in LR.LOCAL_NAMES
        j = i
        while j < len(names) and (names[j] in LR.LOCAL_NAMES) == local:
            j += 1
        if local:
            cols = []
            for t in range(i, j):
                col = []
                for s in scenes:
                    exists = s.get("cls", np.zeros(len(s["boxes"]), np.int32)) != -2
                    full = np.full(len(s["boxes"]), poison)
                    full[exists] = np.asarray(s["ops"][t][1], np.float64)
                    col.append(full)
                cols.append(np.concatenate(col))
            A.local_transform(batch, names[i:j], np.stack(cols, axis=1).reshape(batch.total_boxes, j - i))
        else:
            A.world_frustum_dropout(batch, names[i:j], np.array([[float(s["ops"][t][1]) for t in range(i, j)] for s in scenes]))
        i = j


def _reference(s):
    exists = s.get("cls", np.zeros(len(s["boxes"]), np.int32)) != -2
    alive = ~s["dead"] if "dead" in s else None
    ref = LR.run_ops(s["boxes"], s["points"], s["ops"], alive=alive, exists=exists)
    live = ref.gap[np.ones(len(s["points"]), bool) if alive is None else alive]
    assert (live.min() if len(live) else np.inf) >= R.ROBUST and ref.box_gap >= R.ROBUST       # the case is robust
    return ref


def _compare(batch, scenes):
    pts, boxes = batch.points.cpu().numpy(), batch.boxes.cpu().numpy()
    keep, codes = batch.keep.cpu().numpy().astype(bool), batch.box_cls.cpu().numpy()
    p0 = b0 = 0
    for s in scenes:
        ref = s["ref"] if "ref" in s else _reference(s)
        n, m = len(s["points"]), len(s["boxes"])
        cls = s.get("cls", np.zeros(m, np.int32))
        alive = ref.alive
        assert np.array_equal(keep[p0:p0 + n], alive)                                             # decisions: exactly
        assert np.array_equal(codes[b0:b0 + m], np.where(ref.exists, cls, -2))
        got = pts[p0:p0 + n]
        assert np.array_equal(got[:, 3:], s["points"][:, 3:])
        assert (np.abs(got[alive, :3].astype(np.float64) - ref.pts[alive, :3]) <= ref.err[alive]).all()   # values: within the derived bound
        still = alive & (ref.err.max(axis=1) == 0)
        assert np.array_equal(got[still], s["points"][still])                                     # unmoved points: equal bits
        if "dead" in s:
            assert np.array_equal(got[s["dead"]], s["points"][s["dead"]])                          # dead on entry: never touched
        gone = cls == -2
        assert np.array_equal(boxes[b0:b0 + m][gone], s["boxes"][gone])                           # rows that do not exist: never touched
        ex = ~gone
        assert (np.abs(boxes[b0:b0 + m][ex].astype(np.float64) - ref.boxes[ex]) <= ref.berr[ex]).all()
        p0, b0 = p0 + n, b0 + m


# ---------------------------------------------------------------------------------------------------------- every op alone; the sequential cases
@pytest.mark.gpu
@pytest.mark.parametrize("name", LR.LOCAL_NAMES + LR.WORLD_NAMES)
def test_each_op_on_one_box_and_on_six(cuda, name):
    cases = LR.golden_cases()
    scenes = [cases[name + "_one_box"], cases[name]]
    batch = _batch(scenes, cuda)
    _apply(batch, scenes)
    _compare(batch, scenes)
    if "dropout" in name:
        assert not cases[name]["final"].alive.all()
    else:
        assert (cases[name]["final"].err.max(axis=1) > 0).sum() >= 40


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LR.SEQUENTIAL))
def test_a_moved_point_meets_the_next_box_where_it_now_is(cuda, name):
    """Pairs of parallel boxes 0.12 .. 0.18 m apart: the generator asserts that at least 8 decisions of a later box differ between the moved and
    the unmoved position, so a walk over the original points fails."""
    case = LR.golden_cases()["seq_" + name]
    assert case["final"].moved_decisions >= 8
    batch = _batch([case], cuda)
    _apply(batch, [case])
    _compare(batch, [case])


@pytest.mark.gpu
def test_translation_over_xyz_is_three_passes_in_one_call(cuda):
    """The y pass tests against the centres the x pass moved; the generator asserts that with the original centres at least 8 points end elsewhere."""
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, reset_counters
    case = LR.golden_cases()["translation_xyz"]
    assert case["differ"] >= 8
    batch = _batch([case], cuda)
    reset_counters()
    _apply(batch, [case])
    assert COUNTERS == {"library_calls": 2, "host_reads": 0}      # one plan, one walk
    _compare(batch, [case])


# ---------------------------------------------------------------------------------------------------------- sizes
MIXED = [("local_rotation", -0.3, 0.3), ("local_translation_y", -0.4, 0.4), ("local_scaling", 0.85, 1.2), ("local_dropout_top", 0.0, 0.4),
         ("local_dropout_left", 0.0, 0.4), ("world_dropout_right", 0.0, 0.2)]   # (the world dropout last: the per-box draws before it are sized at entry)


def _mixed_scene(seed, num_boxes, num_points, per_box=None, extent=40.0, cls=None):
    rng = np.random.RandomState(seed)
    boxes = R.make_boxes(rng, num_boxes, extent=extent)
    per_box = per_box if per_box is not None else (num_points // (2 * num_boxes) if num_boxes else 0)
    pts = R.make_points(rng, boxes, num_points + max(24, num_points // 20) - per_box * num_boxes, per_box, C=4)
    exists = None if cls is None else cls != -2
    ops = LR.replay(seed + 1000, MIXED, num_boxes if exists is None else int(exists.sum()))
    run = lambda p: LR.run_ops(boxes, p, ops, exists=exists).gap
    spare = R.robust_scene(pts, run)
    pts, spare = spare[:num_points], spare[num_points:]
    for _ in range(8):                                           # a subset changes the world extremes: top up until it is robust as it stands
        bad = run(pts) < R.ROBUST
        if not bad.any():
            break
        pts, spare = np.concatenate([pts[~bad], spare[:bad.sum()]]), spare[bad.sum():]
    s = dict(boxes=boxes, points=pts, ops=ops)
    if cls is not None:
        s["cls"] = cls
    assert len(pts) == num_points
    return s


@pytest.mark.gpu
def test_scenes_on_either_side_of_a_workgroup(cuda):
    scenes = _cached("sizes", lambda: [_mixed_scene(400 + n, 3, n) for n in (0, 1, 255, 256, 257)])
    batch = _batch(scenes, cuda)
    _apply(batch, scenes)
    _compare(batch, scenes)


@pytest.mark.gpu
def test_box_counts_none_the_cap_and_beyond(cuda):
    import torch
    from seevcn_amd.pcdet.datasets.augmentor import DeviceBatch
    scenes = _cached("caps", lambda: [_mixed_scene(420, 0, 300), _mixed_scene(421, 256, 2600, per_box=8, extent=60.0), _mixed_scene(422, 2, 100)])
    assert [len(s["boxes"]) for s in scenes] == [0, 256, 2]
    batch = _batch(scenes, cuda)
    _apply(batch, scenes)
    _compare(batch, scenes)
    with pytest.raises(ValueError, match="256"):
        DeviceBatch(torch.zeros(4, 4, device=cuda), torch.zeros(257, 7, device=cuda), np.zeros(257, np.int32), [4], [257])
    none = _batch([dict(boxes=np.zeros((0, 7), F), points=scenes[2]["points"])], cuda)            # a batch without any box
    _apply(none, [dict(boxes=np.zeros((0, 7), F), points=scenes[2]["points"], ops=LR.replay(1, MIXED, 0))])
    want = LR.run_ops(np.zeros((0, 7), F), scenes[2]["points"], LR.replay(1, MIXED, 0))
    assert np.array_equal(none.keep.cpu().numpy()[:100].astype(bool), want.alive) and np.array_equal(none.points.cpu().numpy(), scenes[2]["points"])


@pytest.mark.gpu
def test_rows_that_do_not_exist_are_skipped_and_other_classes_move(cuda):
    """box_cls == -2 interleaved with live rows: skipped, no draw consumed (their rows of the draw array hold NaN); -1 rows move like the rest."""
    cls = np.array([0, -2, -1, 1, -2, 0, -1, -2], np.int32)
    s = _cached("skip", lambda: _mixed_scene(430, 8, 700, cls=cls))
    assert len(s["ops"][0][1]) == 5
    batch = _batch([s], cuda)
    _apply(batch, [s])
    _compare(batch, [s])
    ref = _reference(s)
    assert (ref.boxes[2] != s["boxes"][2]).any() and (ref.boxes[6] != s["boxes"][6]).any()         # the -1 rows moved


@pytest.mark.gpu
def test_points_dead_on_entry_are_not_moved_and_not_counted(cuda):
    """keep == 0 on entry: left alone by the local steps and left out of the world dropout's minimum / maximum (they hold the scene's extremes)."""
    def make():
        s = _mixed_scene(440, 5, 600)
        rng = np.random.RandomState(441)
        inside = R.make_points(rng, s["boxes"], 0, 20, C=4, spread=0.4)                          # inside the boxes: a kernel that moved them would show
        far = np.concatenate([rng.uniform(-40, 40, (40, 1)), rng.uniform(-90, -60, (40, 1)), rng.uniform(-2, 1, (40, 2))], axis=1).astype(F)
        dead = np.concatenate([inside, far])                      # and beyond every live point on the dropout's side (right: minimum y)
        pts = np.concatenate([dead[:70], s["points"], dead[70:]])
        flags = np.concatenate([np.ones(70, bool), np.zeros(600, bool), np.ones(len(dead) - 70, bool)])
        return dict(boxes=s["boxes"], points=pts, ops=s["ops"], dead=flags)
    s = _cached("dead", make)
    batch = _batch([s], cuda)
    _apply(batch, [s])
    _compare(batch, [s])
    alone = LR.run_ops(s["boxes"], s["points"][~s["dead"]], s["ops"])
    assert np.array_equal(alone.alive, _reference(s).alive[~s["dead"]])                           # as if the dead points were not there


# ---------------------------------------------------------------------------------------------------------- world dropout
@pytest.mark.gpu
def test_world_dropout_all_directions_in_one_op_takes_boxes_with_their_class(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, reset_counters
    case = dict(LR.golden_cases()["world_all"])
    case["cls"] = np.arange(12, dtype=np.int32) % 3 - 1           # classes -1, 0, 1
    batch = _batch([case], cuda)
    reset_counters()
    _apply(batch, [case])
    assert COUNTERS == {"library_calls": 1, "host_reads": 0}
    _compare(batch, [case])
    ref = case["final"]
    assert 0 < ref.exists.sum() < 12 and np.array_equal(batch.boxes.cpu().numpy(), case["boxes"])  # dropped with their class, rows untouched


@pytest.mark.gpu
def test_world_dropout_intensity_zero_ties_and_empty_scenes(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    boxes = np.zeros((2, 7), F)
    boxes[:, 1], boxes[:, 2] = [3.0, -1.0], [0.5, 2.0]
    pts = np.zeros((6, 4), F)
    pts[:, 2] = [2.0, 1.0, 2.0, -1.0, 0.0, 2.0]                   # the maximum three times over
    pts[:, 1] = [-1.0, 3.0, 0.0, 3.0, -1.0, 0.5]
    empty = dict(boxes=boxes, points=pts[:0])
    all_dead = dict(boxes=boxes, points=pts, dead=np.ones(6, bool))
    for name, fn in (("world_dropout_top", A.global_frustum_dropout_top), ("world_dropout_bottom", A.global_frustum_dropout_bottom),
                     ("world_dropout_left", A.global_frustum_dropout_left), ("world_dropout_right", A.global_frustum_dropout_right)):
        scenes = [dict(boxes=boxes, points=pts), empty, all_dead, dict(boxes=boxes, points=pts, dead=np.array([1, 0, 1, 0, 0, 1], bool))]
        batch = _batch(scenes, cuda)
        fn(batch, np.zeros(4))                                    # intensity exactly 0: the extreme points go, ties included
        keep, codes = batch.keep.cpu().numpy().astype(bool), batch.box_cls.cpu().numpy()[:8]
        p0 = 0
        for i, s in enumerate(scenes):
            ref = LR.run_ops(s["boxes"], s["points"], [(name, 0.0)], alive=~s["dead"] if "dead" in s else None)
            assert np.array_equal(keep[p0:p0 + len(s["points"])], ref.alive) and np.array_equal(codes[2 * i:2 * i + 2], np.where(ref.exists, 0, -2))
            p0 += len(s["points"])
        assert codes[2:6].tolist() == [0, 0, 0, 0]                # a scene without live points passes through, boxes included
    first = LR.run_ops(boxes, pts, [("world_dropout_top", 0.0)])
    assert first.alive.tolist() == [False, True, False, True, True, False] and first.exists.tolist() == [True, False]


# ---------------------------------------------------------------------------------------------------------- refusals, equal bits
@pytest.mark.gpu
def test_wide_boxes_refuse_local_rotation_and_runs_repeat_bit_for_bit(cuda):
    import torch
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    rng = np.random.RandomState(450)
    boxes9 = R.make_boxes(rng, 4, width=9)
    s9 = dict(boxes=boxes9, points=R.make_points(rng, boxes9, 100, 20, C=4))
    batch = _batch([s9], cuda)
    with pytest.raises(NotImplementedError, match="465-468"):
        A.local_rotation(batch, np.full(4, 0.1))
    A.local_scaling(batch, np.full(4, 1.1))                       # the other local functions take the velocity columns along untouched
    assert np.array_equal(batch.boxes.cpu().numpy()[:, 6:], boxes9[:, 6:]) and not np.array_equal(batch.boxes.cpu().numpy()[:, 3:6], boxes9[:, 3:6])
    scenes = [_mixed_scene(400 + n, 3, n) for n in (255, 257)] if "sizes" not in _CACHE else _CACHE["sizes"][2:5:2]
    runs = []
    for _ in range(2):
        b = _batch(scenes, cuda)
        _apply(b, scenes)
        runs.append((b.points.clone(), b.boxes.clone(), b.keep.clone(), b.box_cls.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ---------------------------------------------------------------------------------------------------------- end to end
CLASSES = ["Car", "Pedestrian", "Cyclist"]
E2E_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
PROCESSOR = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True}]
ALL_NAMES = np.array(CLASSES + ["Van"])


def _cfg():
    """pointpillar_newaugs.yaml's augmentor block with nothing disabled; the world translation gets the key the code reads."""
    from seevcn_amd.pcdet.model_cfgs import pointpillar_newaugs_augmentor_cfg
    cfg = pointpillar_newaugs_augmentor_cfg()
    cfg["DISABLE_AUG_LIST"] = []
    for entry in cfg["AUG_CONFIG_LIST"]:
        if entry["NAME"] == "random_world_translation":
            entry["NOISE_TRANSLATE_STD"] = 0.2
    return cfg


def _database():
    """8 objects per class inside a radius of 25 m, their points well inside their boxes (a pasted point cannot be replaced when it comes near a face)."""
    def make():
        rng = np.random.RandomState(500)
        boxes = R.make_boxes(rng, 24, extent=18.0, min_gap=0.5)
        infos = {n: [] for n in CLASSES}
        for k, bx in enumerate(boxes):
            n = 6 + k
            pts = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)), rng.uniform(0, 1, (n, 1))], axis=1).astype(F)
            name = CLASSES[k % 3]
            infos[name].append(dict(name=name, box3d_lidar=bx, points=pts, db_index=k, class_index=k % 3, num_points_in_gt=n, difficulty=0))
        return infos, boxes
    return _cached("db", make)


def _sampler(database=None):
    from seevcn_amd.pcdet.datasets.augmentor.database_sampler import DataBaseSampler
    return DataBaseSampler(None, _cfg()["AUG_CONFIG_LIST"][0], CLASSES, _database()[0], database)


def _e2e_case(num_scenes, num_boxes, seed):
    """Per scene its own RandomState(seed + b).  The expected draws follow the reference sample by sample: each stage's per-box draws are sized by
    the boxes the restatement holds at that point.  A point that ends within 1e-3 m of a comparison or a range limit is replaced by a fresh one
    below every box, inside the scene's z extent (the world dropout's threshold stays), until the case is robust."""
    from seevcn_amd.pcdet.datasets.augmentor import BatchDataAugmentor, data_augmentor as D

    def make():
        stages = BatchDataAugmentor(None, _cfg(), CLASSES, db_infos=_database()[0]).stages
        assert len(stages) == 3                                  # cut behind gt_sampling and behind the world dropout
        scenes = []
        for b in range(num_scenes):
            rng = np.random.RandomState(seed + b)
            boxes = R.make_boxes(rng, num_boxes, extent=44.0)
            scenes.append(dict(points=R.make_points(rng, boxes, 400, max(240 // num_boxes, 4), C=4, spread=0.6), gt_boxes=boxes,
                               gt_names=ALL_NAMES[rng.randint(0, 4, num_boxes)], rng=rng, num_points_in_gt=np.full(num_boxes, 99)))
        for _ in range(12):
            sampler, clean, draws, want = _sampler(), True, [], []
            for b, s in enumerate(scenes):
                rs, cls = np.random.RandomState(1000 + seed + b), np.array([CLASSES.index(n) if n in CLASSES else -1 for n in s["gt_names"]])
                d, n = [], num_boxes
                for st in stages:
                    d += D._draw_scene(rs, st, n, sampler, s["gt_names"])
                    n = LR.prepare_scene(s["points"], s["gt_boxes"], cls, d, num_points_in_gt=s["num_points_in_gt"], check=False, count_boxes=True)
                pts, _, err, _, (gap, ok), origin = LR.prepare_scene(s["points"], s["gt_boxes"], cls, d, num_points_in_gt=s["num_points_in_gt"])
                assert ok and err.max() < 5e-4
                near = (np.abs(np.abs(pts[:, :2].astype(np.float64)) - 51.2) < 1e-3).any(axis=1)
                assert not near[origin < 0].any()
                bad = gap < R.ROBUST
                bad[origin[near & (origin >= 0)]] = True
                if bad.any():
                    clean = False
                    k = int(bad.sum())
                    s["points"][bad] = np.concatenate([s["rng"].uniform(-50, 50, (k, 2)), s["rng"].uniform(-2.45, -2.2, (k, 1)), s["rng"].uniform(0, 1, (k, 1))],
                                                      axis=1).astype(F)
                draws.append(d)
                want.append((cls, d))
            if clean:
                return scenes, draws, [LR.prepare_scene(s["points"], s["gt_boxes"], cls, d, 1, E2E_RANGE, 1, num_points_in_gt=s["num_points_in_gt"], check=False)
                                       for s, (cls, d) in zip(scenes, want)]
        raise AssertionError("the end-to-end case does not become robust")
    return _cached(("e2e", num_scenes, num_boxes, seed), make)


def _augmentor(dev):
    from seevcn_amd.pcdet.datasets.augmentor import BatchDataAugmentor
    from seevcn_amd.pcdet.datasets.augmentor.database_sampler import GtDatabase
    from seevcn_amd.pcdet.datasets.processor import DataProcessor
    infos, db_boxes = _database()
    flat = sorted((i for v in infos.values() for i in v), key=lambda i: i["db_index"])
    db = GtDatabase.from_arrays([i["points"] for i in flat], db_boxes, [i["class_index"] for i in flat], dev)
    dp = DataProcessor(PROCESSOR, np.array(E2E_RANGE, F), training=True, num_point_features=4)
    return BatchDataAugmentor(None, _cfg(), CLASSES, data_processor=dp, db_infos=infos, database=db)


def _device_scenes(scenes, dev):
    return [dict(points=_t(s["points"], dev), gt_boxes=_t(s["gt_boxes"], dev), gt_names=s["gt_names"], num_points_in_gt=s["num_points_in_gt"]) for s in scenes]


def test_end_to_end_case_exercises_every_stage():
    scenes, draws, want = _e2e_case(4, 10, 640)
    for d, w in zip(draws, want):
        names = [n for n, _ in d]
        assert names == ["gt_sampling", "local_rotation", "local_scaling", "flip_x", "rotation", "scaling", "translation_x", "translation_y",
                         "translation_z", "local_translation_x", "local_translation_y", "local_translation_z", "world_dropout_top", "local_dropout_top"]
        assert (w[5] < 0).sum() > 0                              # boxes were accepted and their points pasted
    assert any(len(d[1][1]) != 10 for d in draws)                 # the per-box draws behind gt_sampling are sized by what it left
    assert any(len(d[13][1]) < len(d[1][1]) for d in draws)       # and those behind the world dropout by the boxes it dropped


@pytest.mark.gpu
@pytest.mark.parametrize("num_scenes", [1, 4])
def test_newaugs_queue_end_to_end(cuda, num_scenes):
    import torch
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, reset_counters
    scenes, draws, want = _e2e_case(num_scenes, 10, 640)
    rngs = lambda: [np.random.RandomState(1000 + 640 + b) for b in range(num_scenes)]
    reset_counters()
    out = _augmentor(cuda).forward(_device_scenes(scenes, cuda), rng=rngs())
    counters = dict(COUNTERS)
    assert counters["host_reads"] == 3                           # the two boundaries and the final counts
    ref_pts, ref_gt = R.collate([(w[0], w[1]) for w in want])
    err = np.concatenate([w[2] for w in want])
    berr = np.zeros(ref_gt.shape)
    for b, w in enumerate(want):
        berr[b, :len(w[3])] = w[3]
    pts, gt = out["points"].cpu().numpy(), out["gt_boxes"].cpu().numpy()
    assert pts.shape == ref_pts.shape and gt.shape == ref_gt.shape
    assert np.array_equal(pts[:, 0], ref_pts[:, 0]) and np.array_equal(pts[:, 4:], ref_pts[:, 4:])
    assert (np.abs(pts[:, 1:4].astype(np.float64) - ref_pts[:, 1:4]) <= err).all()
    assert (np.abs(gt.astype(np.float64) - ref_gt) <= berr).all() and np.array_equal(gt[:, :, -1], ref_gt[:, :, -1])
    assert out["points_per_scene"].tolist() == [len(w[0]) for w in want] and out["boxes_per_scene"].tolist() == [len(w[1]) for w in want]
    for d, e in zip(out["draws"], draws):                         # every draw per scene, in order
        assert [n for n, _ in d] == [n for n, _ in e]
        assert [(g, i["db_index"]) for g, i in d[0][1]] == [(g, i["db_index"]) for g, i in e[0][1]]
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for (_, a), (_, b) in zip(d[1:], e[1:]))
    # equal bits run to run; the given draws give the same result with the same boundary reads; wrong per-box sizes are refused
    again = _augmentor(cuda).forward(_device_scenes(scenes, cuda), rng=rngs())
    assert torch.equal(again["points"], out["points"]) and torch.equal(again["gt_boxes"], out["gt_boxes"])
    reset_counters()
    given = _augmentor(cuda).forward(_device_scenes(scenes, cuda), draws=draws)
    assert torch.equal(given["points"], out["points"]) and torch.equal(given["gt_boxes"], out["gt_boxes"]) and dict(COUNTERS) == counters
    short = [list(d) for d in draws]
    short[0][13] = ("local_dropout_top", short[0][13][1][:-1])
    with pytest.raises(ValueError, match="local_dropout_top"):
        _augmentor(cuda).forward(_device_scenes(scenes, cuda), draws=short)
    with pytest.raises(ValueError, match="one numpy RandomState per scene"):
        _augmentor(cuda).forward(_device_scenes(scenes, cuda), rng=np.random.RandomState(0))
    _CACHE[("counters", num_scenes)] = counters
    if ("counters", 1) in _CACHE and ("counters", 4) in _CACHE:
        assert _CACHE[("counters", 1)] == _CACHE[("counters", 4)]


@pytest.mark.gpu
def test_newaugs_counters_depend_on_the_queue_only(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, reset_counters
    aug, seen = _augmentor(cuda), []
    for num_scenes, num_boxes in ((1, 2), (4, 2), (1, 40), (4, 40)):
        scenes = []
        for b in range(num_scenes):
            rng = np.random.RandomState(700 + b)
            boxes = R.make_boxes(rng, num_boxes, extent=46.0)
            scenes.append(dict(points=R.make_points(rng, boxes, 300, 5, C=4), gt_boxes=boxes, gt_names=ALL_NAMES[rng.randint(0, 4, num_boxes)],
                               num_points_in_gt=np.full(num_boxes, 99)))
        reset_counters()
        aug.forward(_device_scenes(scenes, cuda), rng=[np.random.RandomState(b) for b in range(num_scenes)])
        seen.append(dict(COUNTERS))
    assert all(c == seen[0] for c in seen) and seen[0]["host_reads"] == 3
