"""The numpy restatement of the training augmentation (tests/augment_reference.py) against hand-worked cases, and the host half of
seevcn_amd.pcdet.datasets.augmentor: draw_params against a replay of the reference's np.random calls, the sampler's pointer / permutation walk,
the PREPARE filters, LIMIT_WHOLE_SCENE, the refusals, and GtDatabase.from_infos on files it writes itself.  No GPU."""
import numpy as np
import pytest

import augment_reference as R

F = np.float32


# ---------------------------------------------------------------------------------------------------------- the restatement, by hand
def test_in_box_is_the_oracles_matrix_test():
    from oracle.pool_ops import points_in_boxes_cpu
    rng = np.random.RandomState(0)
    boxes = R.make_boxes(rng, 4)
    pts = R.make_points(rng, boxes, 40, 25)
    mine = np.stack([R.in_box(pts[:, :3], b)[0] for b in boxes])
    assert np.array_equal(mine, points_in_boxes_cpu(pts[:, :3], boxes).astype(bool)) and mine.sum() > 10
    # margin 1e-2 in x / y, none in z
    box = np.array([0, 0, 0, 2, 2, 2, 0], F)
    probe = np.array([[1.005, 0, 0], [1.015, 0, 0], [0, -1.005, 0], [0, 0, 1.0], [0, 0, 1.005]], F)
    assert R.in_box(probe, box)[0].tolist() == [True, False, True, True, False]


def test_scale_pre_object_by_hand():
    """One box 4 x 2 x 2 at the origin, heading pi / 2, scale 1.5: a point at (0, 1, 0.5) -- 1 m along the box's length -- goes to 1.5 m along it and
    is lifted by (3 - 2) / 2 on top of its scaled height; a point 2.5 m along the length is outside before, inside after: dropped; one far away stays."""
    box = np.array([[0, 0, 0, 4, 2, 2, np.pi / 2]], F)
    pts = np.array([[0, 1, 0.5, 0.7], [0, 2.5, 0, 0.1], [9, 9, 0, 0.2]], F)
    out, boxes, alive, plan, err, (gap, ok) = R.scale_pre_object(box, pts, np.ones(1), np.full((1, 50), 1.5))
    assert plan.tolist() == [1.5] and alive.tolist() == [True, False, True] and ok
    np.testing.assert_allclose(boxes[0], [0, 0, 0.5, 6, 3, 3, np.pi / 2], atol=1e-6)
    np.testing.assert_allclose(out[0], [0, 1.5, 0.75 + 0.5, 0.7], atol=1e-6)
    assert np.array_equal(out[2], pts[2]) and err[2].max() == 0 and 0 < err[0].max() < 1e-5
    # scale < 1: nobody is dropped; mask 0: nothing happens
    assert R.scale_pre_object(box, pts, np.ones(1), np.full((1, 50), 0.5))[2].all()
    untouched = R.scale_pre_object(box, pts, np.zeros(1), np.full((1, 50), 1.5))
    assert np.array_equal(untouched[0], pts) and np.array_equal(untouched[1], box) and untouched[3].tolist() == [0.0]


def test_scale_pre_object_conflicts_by_hand():
    """Two boxes 0.4 m apart along x: tries that bridge the gap are blocked, the first that does not is taken; a masked-out neighbour blocks as well;
    with every try blocked box and points stay."""
    boxes = np.zeros((2, 7), F)
    boxes[:, 3:6], boxes[1, 0] = [4, 2, 2], 4.4
    pts = np.array([[1.9, 0, 0, 0]], F)
    noises = np.full((2, 50), 1.0)
    noises[0, :3] = [1.3, 1.25, 1.1]
    out, nb, alive, plan, _, (_, ok) = R.scale_pre_object(boxes, pts, [1, 0], noises)
    assert plan.tolist() == [1.1, 0.0] and ok and np.array_equal(nb[1], boxes[1])
    np.testing.assert_allclose(out[0, :3], [1.9 * 1.1, 0, 0.1], atol=1e-6)
    blocked = R.scale_pre_object(boxes, pts, [1, 1], np.full((2, 50), 1.3))
    assert blocked[3].tolist() == [0.0, 0.0] and np.array_equal(blocked[0], pts) and np.array_equal(blocked[1], boxes)


def test_float64_geometry_of_the_robustness_check():
    a, b = np.array([0, 0, 0, 4, 2, 1, 0.0]), np.array([3, 0, 0, 4, 2, 1, 0.0])
    assert abs(R.overlap64(a, b) - 2.0) < 1e-12 and abs(R.separation64(a, b) + 1.0) < 1e-12
    b[0] = 4.5
    assert R.overlap64(a, b) == 0.0 and abs(R.separation64(a, b) - 0.5) < 1e-12
    assert R.pair_is_robust(a, b) == (False, True)
    b[0] = 4.0 + 1e-4
    assert R.pair_is_robust(a, b) == (True, False)               # closer than the IoU's corner margin, no real overlap: not a robust pair
    c = np.array([0, 0, 0, 2, 2, 1, np.pi / 4])
    assert abs(R.overlap64(c, c) - 4.0) < 1e-12


def test_world_transforms_by_hand():
    boxes = np.array([[1, 2, 0, 4, 2, 1, 0.5, 3, -1]], F)
    pts = np.array([[1, 2, 3, 0.5]], F)
    b, p, _, _ = R.world_transform(boxes, pts, [("flip_x", True)])
    assert p[0].tolist() == [1, -2, 3, 0.5] and b[0].tolist() == [1, -2, 0, 4, 2, 1, -0.5, 3, 1]
    b, p, _, _ = R.world_transform(boxes, pts, [("flip_y", True)])
    assert p[0].tolist() == [-1, 2, 3, 0.5] and b[0, 7] == -3 and abs(b[0, 6] + 0.5 + np.pi) < 1e-6
    b, p, e, be = R.world_transform(boxes, pts, [("rotation", np.pi / 2)])
    np.testing.assert_allclose(p[0], [-2, 1, 3, 0.5], atol=1e-6)
    np.testing.assert_allclose(b[0], [-2, 1, 0, 4, 2, 1, 0.5 + np.pi / 2, 1, 3], atol=1e-6)
    assert 0 < e.max() < 1e-5
    b, p, _, _ = R.world_transform(boxes, pts, [("scaling", 2.0), ("translation_z", 0.25)])
    assert p[0].tolist() == [2, 4, 6.25, 0.5] and b[0].tolist() == [2, 4, 0.25, 8, 4, 2, 0.5, 3, -1]
    h, _ = R.limit_period(np.array([3.5, -3.5, 0.1], F))
    np.testing.assert_allclose(h, [3.5 - 2 * np.pi, 2 * np.pi - 3.5, 0.1], atol=1e-6)


def test_tail_by_hand():
    pts = np.array([[44.8, 0, 9], [44.9, 0, 0], [0, -44.8, 0]], F)
    assert R.mask_points_by_range(pts, [-44.8, -44.8, -5, 44.8, 44.8, 3]).tolist() == [True, False, True]
    boxes = np.array([[0, 0, 0, 2, 2, 2, 0], [1, 0, 0, 2, 2, 2, 0]], F)
    assert R.mask_boxes_outside_range(boxes, [-1, -1, -1, 1, 1, 1], 8).tolist() == [True, False]
    assert R.mask_boxes_outside_range(boxes, [-1, -1, -1, 1, 1, 1], 1).tolist() == [True, True]
    corners = R.boxes_to_corners_3d(boxes[:1])[0]
    assert corners[0].tolist() == [1, 1, -1] and corners[6].tolist() == [-1, -1, 1]


# ---------------------------------------------------------------------------------------------------------- draw_params
FULL = [{"NAME": "random_object_scaling", "SCALE_UNIFORM_NOISE": [0.75, 1.0]},
        {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x", "y"]},
        {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.3925, 0.3925]},
        {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]},
        {"NAME": "random_world_translation", "NOISE_TRANSLATE_STD": 0.5, "ALONG_AXIS_LIST": ["x", "y", "z"]}]


def test_draw_params_replays_the_reference_call_sequence():
    from seevcn_amd.pcdet.datasets.augmentor import draw_params
    got = draw_params(np.random.RandomState(7), FULL, [3, 0, 5])
    rs = np.random.RandomState(7)
    for n, d in zip([3, 0, 5], got):
        want = [("object_scaling", rs.uniform(0.75, 1.0, size=[n, 50])), ("flip_x", rs.choice([False, True], replace=False, p=[0.5, 0.5])),
                ("flip_y", rs.choice([False, True], replace=False, p=[0.5, 0.5])), ("rotation", rs.uniform(-0.3925, 0.3925)),
                ("scaling", rs.uniform(0.95, 1.05))] + [("translation_" + a, rs.normal(0, 0.5, 1)[0]) for a in "xyz"]
        assert [k for k, _ in d] == [k for k, _ in want]
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for (_, a), (_, b) in zip(d, want))
    assert got[1][0][1].shape == (0, 50)


def test_draw_params_early_returns_consume_nothing():
    from seevcn_amd.pcdet.datasets.augmentor import draw_params
    cfg = [{"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [1.0, 1.0005]},
           {"NAME": "random_world_translation", "NOISE_TRANSLATE_STD": 0, "ALONG_AXIS_LIST": ["x", "y", "z"]},
           {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": 0.3}]
    got = draw_params(np.random.RandomState(3), cfg, [2])
    assert got == [[("rotation", np.random.RandomState(3).uniform(-0.3, 0.3))]]
    # DISABLE_AUG_LIST, and a scalar SCALE_UNIFORM_NOISE is [-s, s]
    cfg = {"DISABLE_AUG_LIST": ["random_world_flip"], "AUG_CONFIG_LIST": [FULL[1], {"NAME": "random_object_scaling", "SCALE_UNIFORM_NOISE": 0.1}]}
    got = draw_params(np.random.RandomState(4), cfg, [1])
    assert [k for k, _ in got[0]] == ["object_scaling"] and np.array_equal(got[0][0][1], np.random.RandomState(4).uniform(-0.1, 0.1, size=[1, 50]))


def test_names_that_are_not_built_are_refused_by_name():
    from seevcn_amd.pcdet.datasets.augmentor import BatchDataAugmentor, draw_params
    from seevcn_amd.pcdet.datasets.processor import DataProcessor
    for name in ("random_local_rotation", "random_image_flip", "random_local_pyramid_aug", "random_world_frustum_dropout"):
        with pytest.raises(NotImplementedError, match=name):
            BatchDataAugmentor(None, [{"NAME": name}], ["car"])
        with pytest.raises(NotImplementedError, match=name):
            draw_params(np.random.RandomState(0), [{"NAME": name}], [1])
    with pytest.raises(NotImplementedError, match="random_object_scaling after gt_sampling"):
        BatchDataAugmentor(None, [dict(_sampler_cfg()), FULL[0]], ["car"], db_infos=_infos())
    with pytest.raises(NotImplementedError, match="sample_points"):
        DataProcessor([{"NAME": "sample_points"}], np.zeros(6), True)


# ---------------------------------------------------------------------------------------------------------- the sampler's host logic
def _infos(n_car=7, n_ped=5):
    infos = {"car": [], "pedestrian": [], "bus": []}
    for name, n in (("car", n_car), ("pedestrian", n_ped)):
        for k in range(n):
            infos[name].append(dict(name=name, path=f"gt_database/{name}_{k}.bin", box3d_lidar=np.arange(7, dtype=F) + k, num_points_in_gt=3 * k,
                                    difficulty=k % 3 - 1, db_index=len(infos["car"]) + len(infos["pedestrian"]), class_index=0))
    return infos


def _sampler_cfg(**kw):
    cfg = {"NAME": "gt_sampling", "PREPARE": {"filter_by_min_points": ["car:5", "pedestrian:0"], "filter_by_difficulty": [-1]},
           "SAMPLE_GROUPS": ["car:3", "bus:4", "pedestrian:2", "truck:9"], "NUM_POINT_FEATURES": 4, "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0],
           "LIMIT_WHOLE_SCENE": False}
    cfg.update(kw)
    return cfg


def _sampler(**kw):
    from seevcn_amd.pcdet.datasets.augmentor.database_sampler import DataBaseSampler
    return DataBaseSampler(None, _sampler_cfg(**kw), ["car", "pedestrian", "bus"], _infos(), None)


def test_prepare_filters():
    s = _sampler()
    # cars: num_points_in_gt >= 5 keeps k = 2..6, difficulty != -1 drops k = 3, 6; pedestrians: min 0 filters nothing, difficulty drops k = 0, 3
    assert [i["num_points_in_gt"] // 3 for i in s.db_infos["car"]] == [2, 4, 5]
    assert [i["num_points_in_gt"] // 3 for i in s.db_infos["pedestrian"]] == [1, 2, 4]
    assert list(s.sample_groups) == ["car", "bus", "pedestrian"]  # SAMPLE_GROUPS order, classes outside class_names left out


def test_pointer_and_permutation_walk():
    s = _sampler(PREPARE={})
    rs, replay = np.random.RandomState(5), np.random.RandomState(5)
    group = s.sample_groups["car"]
    assert group["pointer"] == 7                                  # starts past the end: the first call draws a permutation
    perm = replay.permutation(7)
    got = [i["db_index"] for i in s.sample_with_fixed_number("car", group, rs)]
    assert got == perm[:3].tolist() and group["pointer"] == 3
    assert [i["db_index"] for i in s.sample_with_fixed_number("car", group, rs)] == perm[3:6].tolist()
    assert [i["db_index"] for i in s.sample_with_fixed_number("car", group, rs)] == perm[6:].tolist() and group["pointer"] == 9      # a short slice, no draw
    perm2 = replay.permutation(7)
    assert [i["db_index"] for i in s.sample_with_fixed_number("car", group, rs)] == perm2[:3].tolist()
    assert rs.uniform() == replay.uniform()                      # exactly the reference's draws were consumed


def test_draw_visits_groups_in_order_and_limits_the_whole_scene():
    s = _sampler(PREPARE={}, LIMIT_WHOLE_SCENE=True)
    rs, replay = np.random.RandomState(6), np.random.RandomState(6)
    got = s.draw(np.array(["car", "car", "pedestrian", "pedestrian", "truck"]), rs)
    # car: 3 - 2 = 1 wanted; bus: 4 wanted, none in the database (a permutation of 0 is still drawn); pedestrian: 2 - 2 = 0 -> no call, no draw
    car_perm = replay.permutation(7)
    replay.permutation(0)
    assert [(g, i["db_index"]) for g, i in got] == [(0, int(car_perm[0]))]
    assert rs.uniform() == replay.uniform()
    from seevcn_amd.pcdet.datasets.augmentor import draw_params
    cfg = [_sampler_cfg(PREPARE={}), FULL[1]]
    s2 = _sampler(PREPARE={})
    d = draw_params(np.random.RandomState(8), cfg, [2], s2, [np.array(["car", "bus"])])
    replay = np.random.RandomState(8)
    car, _, ped = replay.permutation(7), replay.permutation(0), replay.permutation(5)
    assert [(g, i["db_index"]) for g, i in d[0][0][1]] == [(0, int(c)) for c in car[:3]] + [(2, 7 + int(p)) for p in ped[:2]]
    assert d[0][1] == ("flip_x", bool(replay.choice([False, True], replace=False, p=[0.5, 0.5])))


def test_road_planes_and_image_paste_are_refused_by_key():
    with pytest.raises(NotImplementedError, match="USE_ROAD_PLANE"):
        _sampler(USE_ROAD_PLANE=True)
    with pytest.raises(NotImplementedError, match="IMG_AUG_TYPE"):
        _sampler(IMG_AUG_TYPE="kitti")
    _sampler(USE_ROAD_PLANE=False, IMG_AUG_TYPE=None)


def test_database_from_infos_reads_the_bin_files(tmp_path):
    """from_infos with np.fromfile on files written here; the device is the CPU only to look at the tensors (the sampler itself runs on the GPU)."""
    import torch
    from seevcn_amd.pcdet.datasets.augmentor import database_sampler as D
    infos = _infos(3, 2)
    (tmp_path / "gt_database").mkdir()
    rng = np.random.RandomState(9)
    written = {}
    for name in ("car", "pedestrian"):
        for k, info in enumerate(infos[name]):
            written[info["path"]] = rng.rand(4 + k, 4).astype(F)
            written[info["path"]].tofile(str(tmp_path / info["path"]))
    orig = D.L.require_cuda
    D.L.require_cuda = lambda *t: None
    try:
        db = D.GtDatabase.from_infos(infos, tmp_path, 4, ["car", "pedestrian", "bus"], torch.device("cpu"))
    finally:
        D.L.require_cuda = orig
    assert db.offsets.tolist() == [0, 4, 9, 15, 19, 24] and db.counts.tolist() == [4, 5, 6, 4, 5]
    assert db.class_ids.tolist() == [0, 0, 0, 1, 1] and db.boxes.shape == (5, 7)
    for name in ("car", "pedestrian"):
        for info in infos[name]:
            k = info["db_index"]
            assert np.array_equal(db.points[db.offsets[k]:db.offsets[k + 1]].numpy(), written[info["path"]])
            assert np.array_equal(db.boxes[k].numpy(), info["box3d_lidar"])
