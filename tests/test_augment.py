"""csrc/augment.hip and seevcn_amd.pcdet.datasets.augmentor on the GPU against the numpy restatement (tests/augment_reference.py).

Every generated case is shown robust on the CPU when it is built (augment_reference: box pairs apart or overlapping by a margin, points at
least 1e-3 m from every face they are tested against), so plans, keep flags, counts and output order must equal the restatement exactly; moved
coordinates are held to the restatement's per-element bound k * 2**-24 * sum|terms| (derived in its header, not fitted).  The range-limit cases
sit exactly on the limits on purpose."""
import numpy as np
import pytest

import augment_reference as R

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
    from seevcn_amd.pcdet.datasets.augmentor import DeviceBatch
    return DeviceBatch.from_scenes([_t(s["points"], dev) for s in scenes], [_t(s["boxes"], dev) for s in scenes], [s["cls"] for s in scenes])


def _robust_points(points, boxes, mask, noises):
    """Drop the input points that come within ROBUST of a face they are tested against; the boxes' plan does not depend on the points."""
    def run(p):
        return R.scale_pre_object(boxes, p, mask, noises, check=False)[5][0]
    return R.robust_scene(points, run)


# ---------------------------------------------------------------------------------------------------------- object scaling: the cases
def _fill(rows, n, value=1.0):
    out = np.full((n, 50), value)
    for i, r in rows.items():
        out[i, :len(r)] = r
    return out


def _scene_five():
    """5 boxes (headings 0, sizes 4 x 2 x 1.6), scale range [0.9, 1.3]:
      box 0 at (0, 0): tries 1.28 and 1.25 reach into box 1 (left face at 2.4), 1.1 is the first free try -- not try 0 -- and > 1
      box 1 at (4.4, 0): try 1.15 (left face 2.1) is free of box 0 as it was (right face 2.0) and blocked by box 0 as it is now (2.2); 1.05 is free
      box 2 at (0, 3): another class (masked out), never scaled, still an obstacle
      box 3 at (0, 5.15): try 1.25 (lower face 3.9) runs into the masked box 2 (upper face 4.0); 1.05 is free and > 1 (upper face 6.2)
      box 4 at (0, 7.215): lower face 6.215, 0.015 above the new box 3 -- beyond the IoU's 1e-2 corner margin, inside twice the point margin
    and one point at (0, 6.2075): outside box 3 before, inside it after (margin 1e-2) -> dropped by box 3, although box 4 holds it too."""
    boxes = np.zeros((5, 7), F)
    boxes[:, 3:6] = [4.0, 2.0, 1.6]
    boxes[:, 2] = -1.0
    boxes[:, :2] = [[0, 0], [4.4, 0], [0, 3.0], [0, 5.15], [0, 7.215]]
    cls = np.array([0, 1, -1, 0, 2], np.int32)
    noises = _fill({0: [1.28, 1.25, 1.1], 1: [1.15, 1.05], 2: [1.0], 3: [1.25, 1.05], 4: [0.95]}, 5)
    rng = np.random.RandomState(11)
    pts = R.make_points(rng, boxes, 380, 50)
    special = np.array([[0.0, 6.2075, -1.0, 0.5, 0.5]], F)
    pts = np.concatenate([_robust_points(pts, boxes, cls >= 0, noises)[:599], special])
    return dict(points=pts, boxes=boxes, cls=cls, noises=noises)


def _scene_seventy():
    """70 boxes over more than one wave of boxes and of (try, other) pairs, scale range [0.9, 1.9] so that neighbours do collide; boxes 68 and 69
    overlap each other: all 50 tries of both are blocked."""
    rng = np.random.RandomState(12)
    boxes = R.make_boxes(rng, 70, extent=30.0, min_gap=1.0)
    boxes[69] = boxes[68]
    boxes[69, 0] += F(1.0)
    cls = rng.randint(-1, 3, 70).astype(np.int32)
    cls[68:] = [0, 1]
    noises = rng.uniform(0.9, 1.9, (70, 50))
    pts = _robust_points(R.make_points(rng, boxes, 200, 8), boxes, cls >= 0, noises)
    return dict(points=pts, boxes=boxes, cls=cls, noises=noises)


def _scene_empty():
    rng = np.random.RandomState(13)
    return dict(points=R.make_points(rng, np.zeros((0, 7), F), 100, 0), boxes=np.zeros((0, 7), F), cls=np.zeros(0, np.int32), noises=np.zeros((0, 50)))


def _scene_single():
    rng = np.random.RandomState(14)
    boxes = R.make_boxes(rng, 1)
    noises = _fill({0: [1.2, 0.9]}, 1)
    pts = _robust_points(R.make_points(rng, boxes, 100, 60), boxes, np.ones(1), noises)
    return dict(points=pts, boxes=boxes, cls=np.zeros(1, np.int32), noises=noises)


def _scale_cases():
    def make():
        scenes = [_scene_five(), _scene_seventy(), _scene_empty(), _scene_single()]
        for s in scenes:
            s["ref"] = R.scale_pre_object(s["boxes"], s["points"], s["cls"] >= 0, s["noises"])
        return scenes
    return _cached("scale", make)


def test_scale_cases_are_robust_and_hit_their_edges():
    five, seventy, empty, single = _scale_cases()
    for s in (five, seventy, single):
        pts, boxes, alive, plan, err, (gap, pairs_ok) = s["ref"]
        assert pairs_ok and gap.min() >= R.ROBUST
    pts, boxes, alive, plan, err, _ = five["ref"]
    assert len(five["points"]) == 600
    assert plan.tolist() == [1.1, 1.05, 0.0, 1.05, 0.95]
    # with box 0 at its old size box 1 would have taken its first try
    assert R.scale_pre_object(five["boxes"][1:], five["points"], np.ones(4), five["noises"][1:], check=False)[3][0] == 1.15
    assert not alive[-1] and R.in_box(five["points"][-1:, :3], five["boxes"][4])[0][0]           # dropped by box 3, inside box 4
    assert (~alive).sum() > 5 and np.array_equal(boxes[2], five["boxes"][2])
    pts, boxes, alive, plan, err, _ = seventy["ref"]
    assert plan[68] == 0 and plan[69] == 0 and (plan[seventy["cls"] < 0] == 0).all()
    tries = [int(np.nonzero(seventy["noises"][k] == plan[k])[0][0]) for k in range(68) if plan[k] != 0]
    assert max(tries) >= 2 and min(tries) == 0 and (~alive).sum() > 0
    assert single["ref"][3][0] == 1.2


@pytest.mark.gpu
def test_scale_pre_object_matches_the_restatement(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    scenes = _scale_cases()
    batch = _batch(scenes, cuda)
    plan = A.scale_pre_object(batch, np.concatenate([s["noises"] for s in scenes])).cpu().numpy()
    pts, boxes, keep = batch.points.cpu().numpy(), batch.boxes.cpu().numpy(), batch.keep.cpu().numpy().astype(bool)
    p0 = b0 = 0
    for s in scenes:
        rp, rb, alive, rplan, err, _ = s["ref"]
        n, m = len(rp), len(rb)
        assert np.array_equal(plan[b0:b0 + m], rplan)
        assert np.array_equal(boxes[b0:b0 + m], rb)
        assert np.array_equal(keep[p0:p0 + n], alive)
        got = pts[p0:p0 + n][alive]
        assert np.array_equal(got[:, 3:], s["points"][alive][:, 3:])                               # intensity and further columns untouched
        assert (np.abs(got[:, :3].astype(np.float64) - rp[alive][:, :3]) <= err[alive]).all()
        still = err[alive].max(axis=1) == 0
        assert np.array_equal(got[still], s["points"][alive][still])                              # unmoved points: bit-identical
        p0, b0 = p0 + n, b0 + m
    # all 50 tries blocked: boxes 68 / 69 of the 70-box scene and their points are the input's bits
    s, b0, p0 = scenes[1], len(scenes[0]["boxes"]), len(scenes[0]["points"])
    assert np.array_equal(boxes[b0 + 68:b0 + 70], s["boxes"][68:70])
    inside = R.in_box(s["points"][:, :3], s["boxes"][68])[0] | R.in_box(s["points"][:, :3], s["boxes"][69])[0]
    assert inside.sum() > 0 and np.array_equal(pts[p0:p0 + len(inside)][inside], s["points"][inside]) and keep[p0:p0 + len(inside)][inside].all()


@pytest.mark.gpu
def test_points_in_boxes_count_and_min_points_filter(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    scenes = _scale_cases()
    batch = _batch(scenes, cuda)
    want = np.concatenate([R.points_in_boxes_count(s["points"], s["boxes"])[0] for s in scenes])
    got = A.points_in_boxes_count(batch).cpu().numpy()
    assert np.array_equal(got, want) and want.max() >= 8 > want.min()
    A.filter_boxes_by_min_points(batch, 8)
    cls = np.concatenate([s["cls"] for s in scenes])
    assert np.array_equal(batch.box_cls[:len(cls)].cpu().numpy(), np.where(want >= 8, cls, -2))


@pytest.mark.gpu
def test_filtered_boxes_do_not_block(cuda):
    """A box removed by MIN_POINTS_OF_GT does not exist for the others: box 1 of the 5-box scene gone, box 0 takes its first try."""
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    s = dict(_scale_cases()[0])
    s["cls"] = s["cls"].copy()
    s["cls"][1] = -2
    batch = _batch([s], cuda)
    plan = A.scale_pre_object(batch, s["noises"]).cpu().numpy()
    keep = np.array([0, 2, 3, 4])
    ref = R.scale_pre_object(s["boxes"][keep], s["points"], s["cls"][keep] >= 0, s["noises"][keep], check=False)
    assert plan[0] == 1.28 and np.array_equal(plan[keep], ref[3]) and plan[1] == 0
    assert np.array_equal(batch.boxes.cpu().numpy()[keep], ref[1]) and np.array_equal(batch.keep.cpu().numpy().astype(bool), ref[2])


@pytest.mark.gpu
def test_limits_are_refused_on_the_host(cuda):
    import torch
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    dev = cuda
    with pytest.raises(ValueError, match="256"):
        A.DeviceBatch(torch.zeros(4, 4, device=dev), torch.zeros(257, 7, device=dev), np.zeros(257, np.int32), [4], [257])
    batch = A.DeviceBatch(torch.zeros(4, 4, device=dev), torch.ones(2, 7, device=dev), np.zeros(2, np.int32), [4], [2])
    with pytest.raises(ValueError, match="num_try"):
        A.scale_pre_object(batch, np.ones((2, 65)))


# ---------------------------------------------------------------------------------------------------------- GT sampling
GT_CLASSES = ["car", "truck"]
GT_CFG = {"NAME": "gt_sampling", "PREPARE": {}, "SAMPLE_GROUPS": ["car:6", "truck:4"], "NUM_POINT_FEATURES": 5, "REMOVE_EXTRA_WIDTH": [0.2, 0.2, 0.2],
          "LIMIT_WHOLE_SCENE": False}


def _gt_database():
    """cars c0..c5 (rows 0-5), trucks d0..d4 (rows 6-10), all 4 x 2 x 1.6:
      c0 (1, 0.5) overlaps the existing box at (0, 0); c1 (0, 10) and c2 (1.5, 10.5) overlap each other; c3 (0, 20), c4 (10, 20), c5 (20, 20) are free;
      d0 (1, 20.5) overlaps c3; d1 (0.5, 10.2) overlaps only c1 / c2, which were not accepted; d2 (20, 0.8) overlaps the existing box of another
      class at (20, 0); d3 (30, 30) is free; d4 (10.5, 0.2) overlaps the existing box at (10, 0)."""
    def make():
        rng = np.random.RandomState(60)
        xy = [(1, 0.5), (0, 10), (1.5, 10.5), (0, 20), (10, 20), (20, 20), (1, 20.5), (0.5, 10.2), (20, 0.8), (30, 30), (10.5, 0.2)]
        boxes = np.zeros((11, 7), F)
        boxes[:, :2], boxes[:, 2], boxes[:, 3:6] = xy, -1.0, [4.0, 2.0, 1.6]
        boxes[4, 6] = 0.7
        infos = {"car": [], "truck": []}
        for k in range(11):
            pts = np.concatenate([rng.uniform(-0.9, 0.9, (7 + 3 * k, 3)), rng.uniform(0, 1, (7 + 3 * k, 2))], axis=1).astype(F)
            name = "car" if k < 6 else "truck"
            infos[name].append(dict(name=name, box3d_lidar=boxes[k], points=pts, db_index=k, class_index=GT_CLASSES.index(name), num_points_in_gt=len(pts),
                                    difficulty=0))
        return infos, boxes
    return _cached("gtdb", make)


def _gt_scenes():
    def make():
        infos, db_boxes = _gt_database()
        car, truck = infos["car"], infos["truck"]
        existing = np.zeros((3, 7), F)
        existing[:, :2], existing[:, 2], existing[:, 3:6] = [(0, 0), (10, 0), (20, 0)], -1.0, [4.0, 2.0, 1.6]
        all_cands = [(0, i) for i in car] + [(1, i) for i in truck[:4]]
        layouts = [(existing, np.array([0, 1, -1], np.int32), all_cands),
                   (existing[:0], np.zeros(0, np.int32), all_cands),                            # no existing boxes: iou1 := iou2
                   (existing[:2], np.array([0, 1], np.int32), [(0, car[0]), (1, truck[4])])]    # nothing accepted: unchanged
        scenes = []
        for b, (boxes, cls, cands) in enumerate(layouts):
            rng = np.random.RandomState(61 + b)
            pts = np.concatenate([R.make_points(rng, db_boxes, 300, 30, extent=36.0), R.make_points(rng, boxes, 0, 20)])

            def run(p, boxes=boxes, cls=cls, cands=cands):
                return R.prepare_scene(p, boxes, cls, [("gt_sampling", cands)], check=False, extra_width=GT_CFG["REMOVE_EXTRA_WIDTH"],
                                       num_points_in_gt=np.full(len(boxes), 99))[4][0]
            pts = R.robust_scene(pts, run)
            ref = R.gt_sampling(pts, boxes, cls >= 0, [(np.stack([i["box3d_lidar"] for g, i in cands if g == gid]), [i["points"] for g, i in cands if g == gid])
                                                       for gid in (0, 1)], GT_CFG["REMOVE_EXTRA_WIDTH"])
            scenes.append(dict(points=pts, boxes=boxes, cls=cls, cands=cands, ref=ref))
        return scenes
    return _cached("gtscenes", make)


def test_gt_sampling_cases_hit_their_edges():
    a, b, c = _gt_scenes()
    for s in (a, b, c):
        assert s["ref"][4][1] and s["ref"][4][0].min() >= R.ROBUST
    assert a["ref"][2].tolist() == [False, False, False, True, True, True, False, True, False, True]
    assert b["ref"][2].tolist() == [True, False, False, True, True, True, False, True, True, True]
    assert not c["ref"][2].any() and np.array_equal(c["ref"][0], c["points"]) and np.array_equal(c["ref"][1], c["boxes"])
    # the removal reaches into REMOVE_EXTRA_WIDTH: some removed points are outside every accepted box itself
    acc = [i["box3d_lidar"] for (_, i), ok in zip(a["cands"], a["ref"][2]) if ok]
    inside = np.any([R.in_box(a["points"][:, :3], bx)[0] for bx in acc], axis=0)
    assert (a["ref"][3] & ~inside).sum() > 0 and (a["ref"][3] & inside).sum() > 0


@pytest.mark.gpu
def test_gt_sampling_select_and_paste(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    from seevcn_amd.pcdet.datasets.augmentor.database_sampler import DataBaseSampler, GtDatabase
    infos, db_boxes = _gt_database()
    flat = infos["car"] + infos["truck"]
    db = GtDatabase.from_arrays([i["points"] for i in flat], db_boxes, [i["class_index"] for i in flat], cuda)
    sampler = DataBaseSampler(None, GT_CFG, GT_CLASSES, infos, db)
    scenes = _gt_scenes()
    cands = [s["cands"] for s in scenes]
    batch = A.DeviceBatch.from_scenes([_t(s["points"], cuda) for s in scenes], [_t(s["boxes"], cuda) for s in scenes], [s["cls"] for s in scenes],
                                      [sum(len(i["points"]) for _, i in c) for c in cands], [len(c) for c in cands])
    A.reset_counters()
    accept = sampler(batch, cands).cpu().numpy().astype(bool)
    assert A.COUNTERS["library_calls"] == 2 and A.COUNTERS["host_reads"] == 0
    assert np.array_equal(accept, np.concatenate([s["ref"][2] for s in scenes]))
    out = A.compact(batch)
    want = []
    for s in scenes:
        pts, boxes, acc, removed, _ = s["ref"]
        cls = np.concatenate([s["cls"][s["cls"] >= 0], [i["class_index"] for (_, i), ok in zip(s["cands"], acc) if ok]]) if acc.any() else s["cls"]
        keep = cls >= 0
        want.append((pts, np.concatenate([boxes[keep], (cls[keep] + 1).astype(F)[:, None]], axis=1)))
    ref_pts, ref_gt = R.collate(want)
    assert np.array_equal(out["points"].cpu().numpy(), ref_pts)                                    # object points first, in acceptance order: equal bits
    assert np.array_equal(out["gt_boxes"].cpu().numpy(), ref_gt)
    assert out["boxes_per_scene"].tolist() == [len(g) for _, g in want] == [7, 7, 2]
    # the same call again on the same batch: every candidate now meets its own copy or its old obstacle; nothing is appended past a scene's rows
    assert not sampler(batch, cands).cpu().numpy().any() and bool((batch.box_cnt <= batch.box_cap).all())
    assert A.compact(batch)["boxes_per_scene"].tolist() == [7, 7, 2]


# ---------------------------------------------------------------------------------------------------------- world transforms
# ---------------------------------------------------------------------------------------------------------- world transforms
def _world_scenes(width):
    def make():
        out = []
        for b in range(4):
            rng = np.random.RandomState(20 + b)
            boxes = R.make_boxes(rng, 3 + 2 * b, width=width)
            out.append(dict(points=R.make_points(rng, boxes, 150 + 37 * b, 5), boxes=boxes, cls=np.zeros(len(boxes), np.int32)))
        return out
    return _cached(("world", width), make)


WORLD_OPS = ["flip_x", "flip_y", "rotation", "scaling", "translation_x", "translation_y", "translation_z"]
WORLD_PARAMS = np.array([[0, 0, 0.3925, 1.05, 0.5, -0.25, 0.125], [1, 0, -0.3, 0.95, 0.1, 0.2, 0.3], [0, 1, 0.1234567, 1.0123, -1.5, 2.5, -0.05],
                         [1, 1, -0.39, 0.97, 0.7, 0.0, 0.01]])


@pytest.mark.gpu
@pytest.mark.parametrize("width", [7, 9])
def test_world_transforms_fused_and_one_by_one(cuda, width):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    scenes = _world_scenes(width)
    fused, single = _batch(scenes, cuda), _batch(scenes, cuda)
    A.world_transform(fused, WORLD_OPS, WORLD_PARAMS, limit_heading=True)
    A.random_flip_along_x(single, WORLD_PARAMS[:, 0])
    A.random_flip_along_y(single, WORLD_PARAMS[:, 1])
    A.global_rotation(single, WORLD_PARAMS[:, 2])
    A.global_scaling(single, WORLD_PARAMS[:, 3])
    A.random_translation_along_x(single, WORLD_PARAMS[:, 4])
    A.random_translation_along_y(single, WORLD_PARAMS[:, 5])
    A.random_translation_along_z(single, WORLD_PARAMS[:, 6])
    A.world_transform(single, [], None, limit_heading=True)
    assert np.array_equal(fused.points.cpu().numpy(), single.points.cpu().numpy())
    assert np.array_equal(fused.boxes.cpu().numpy(), single.boxes.cpu().numpy())
    pts, boxes = fused.points.cpu().numpy(), fused.boxes.cpu().numpy()
    p0 = b0 = 0
    for b, s in enumerate(scenes):
        rb, rp, err, berr = R.world_transform(s["boxes"], s["points"], list(zip(WORLD_OPS, WORLD_PARAMS[b])))
        rb[:, 6], e = R.limit_period(rb[:, 6])
        berr[:, 6] += e
        n, m = len(rp), len(rb)
        assert np.array_equal(pts[p0:p0 + n, 3:], s["points"][:, 3:])
        assert (np.abs(pts[p0:p0 + n, :3].astype(np.float64) - rp[:, :3]) <= err).all()
        assert (np.abs(boxes[b0:b0 + m].astype(np.float64) - rb) <= berr).all()
        assert (np.abs(boxes[b0:b0 + m, 6]) <= np.pi + 1e-6).all()
        p0, b0 = p0 + n, b0 + m


@pytest.mark.gpu
def test_flips_are_exact_and_velocity_follows(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    scenes = _world_scenes(9)
    batch = _batch(scenes, cuda)
    A.world_transform(batch, ["flip_x", "flip_y"], WORLD_PARAMS[:, :2])
    pts, boxes = batch.points.cpu().numpy(), batch.boxes.cpu().numpy()
    p0 = b0 = 0
    for b, s in enumerate(scenes):
        rb, rp, _, _ = R.world_transform(s["boxes"], s["points"], [("flip_x", WORLD_PARAMS[b, 0]), ("flip_y", WORLD_PARAMS[b, 1])])
        assert np.array_equal(pts[p0:p0 + len(rp)], rp) and np.array_equal(boxes[b0:b0 + len(rb)][:, [0, 1, 2, 3, 4, 5, 7, 8]], rb[:, [0, 1, 2, 3, 4, 5, 7, 8]])
        assert np.abs(boxes[b0:b0 + len(rb), 6] - rb[:, 6]).max() <= 4 * R.U * 2 * np.pi
        p0, b0 = p0 + len(rp), b0 + len(rb)


# ---------------------------------------------------------------------------------------------------------- the tail
RANGE = [-44.8, -44.8, -5.0, 44.8, 44.8, 3.0]


def _limit_points():
    lo, hi = F(-44.8), F(44.8)
    up, down = lambda v: np.nextafter(v, F(np.inf), dtype=F), lambda v: np.nextafter(v, F(-np.inf), dtype=F)
    xy = [(hi, 0), (up(hi), 0), (lo, 0), (down(lo), 0), (0, hi), (0, up(hi)), (0, lo), (0, down(lo)), (hi, lo), (up(hi), up(hi)), (0, 0), (10, 100)]
    pts = np.zeros((len(xy), 4), F)
    pts[:, :2] = xy
    pts[:, 2] = [0, 0, 0, 0, 9, 9, -9, -9, 0, 0, 0, 0]            # z is not part of mask_points_by_range
    pts[:, 3] = np.arange(len(xy))
    return pts


def test_limit_points_sit_on_the_limits():
    pts = _limit_points()
    assert R.mask_points_by_range(pts, RANGE).tolist() == [True, False, True, False, True, False, True, False, True, False, True, False]
    assert float(pts[0, 0]) < 44.8 < float(pts[1, 0])            # float32(44.8) <= 44.8 holds against the float64 limit, one ulp up does not


def _corner_boxes():
    """Boxes with 8, 1 and 0 corners inside RANGE (and one of another class): heading pi / 4 puts one corner of the second across the x limit only."""
    boxes = np.zeros((5, 7), F)
    boxes[:, 3:6] = [4.0, 2.0, 1.5]
    boxes[0, :3] = [10, 10, -1]
    boxes[1, :3] = [46.9, 0, 2.6]                                 # and z: only its lower face is below the upper limit
    boxes[1, 6] = np.pi / 4
    boxes[2, :3] = [60, 60, -1]
    boxes[3, :3] = [-10, 5, -1]
    boxes[4, :3] = [44.0, -44.0, -1]
    return boxes, np.array([0, 2, 1, -1, 1], np.int32)


def test_corner_boxes_have_the_corner_counts():
    boxes, _ = _corner_boxes()
    corners = R.boxes_to_corners_3d(boxes).astype(np.float64)
    inside = ((corners >= np.array(RANGE[:3])) & (corners <= np.array(RANGE[3:]))).all(axis=2).sum(axis=1)
    assert inside.tolist()[:3] == [8, 1, 0] and 1 < inside[4] < 8


@pytest.mark.gpu
@pytest.mark.parametrize("min_num_corners", [1, 8])
def test_tail_masks_class_column_and_explicit_shuffle(cuda, min_num_corners):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    boxes, cls = _corner_boxes()
    rng = np.random.RandomState(31)
    scenes = [dict(points=_limit_points(), boxes=boxes, cls=cls),
              dict(points=rng.uniform(-60, 60, (700, 4)).astype(F), boxes=boxes[:0], cls=cls[:0]),
              dict(points=rng.uniform(-60, 60, (300, 4)).astype(F), boxes=boxes[::-1].copy(), cls=cls[::-1].copy())]
    masks = [R.mask_points_by_range(s["points"], RANGE) for s in scenes]
    perms = [np.random.RandomState(40 + b).permutation(int(m.sum())) for b, m in enumerate(masks)]
    A.reset_counters()
    out = A.compact(_batch(scenes, cuda), point_range=RANGE, box_range=RANGE, min_num_corners=min_num_corners, shuffle=perms)
    assert A.COUNTERS == {"library_calls": 1, "host_reads": 1}
    want_pts, want_gt = [], []
    for s, m, perm in zip(scenes, masks, perms):
        want_pts.append(s["points"][m][perm])
        b, c = s["boxes"][s["cls"] >= 0], s["cls"][s["cls"] >= 0]
        b = np.concatenate([b, (c + 1).astype(F)[:, None]], axis=1)
        want_gt.append(b[R.mask_boxes_outside_range(b, RANGE, min_num_corners)])
    pts, gt = R.collate(list(zip(want_pts, want_gt)))
    assert np.array_equal(out["points"].cpu().numpy(), pts) and np.array_equal(out["gt_boxes"].cpu().numpy(), gt)
    assert out["points_per_scene"].tolist() == [len(p) for p in want_pts] and out["boxes_per_scene"].tolist() == [len(g) for g in want_gt]
    assert out["empty_scenes"] == [1] and [len(g) for g in want_gt] == ([3, 0, 3] if min_num_corners == 1 else [1, 0, 1])
    assert out["scene_cnt"].cpu().numpy().tolist() == [len(p) for p in want_pts]
    assert out["scene_start"].cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(p) for p in want_pts])]).tolist()


@pytest.mark.gpu
def test_range_helpers_and_device_shuffle(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    from seevcn_amd.pcdet.utils import box_utils, common_utils
    pts = _limit_points()
    assert np.array_equal(common_utils.mask_points_by_range(_t(pts, cuda), RANGE).cpu().numpy(), R.mask_points_by_range(pts, RANGE))
    boxes, _ = _corner_boxes()
    many = np.tile(boxes, (60, 1))                               # 300 boxes: more than one scene's worth
    for k in (1, 8):
        assert np.array_equal(box_utils.mask_boxes_outside_range(_t(many, cuda), RANGE, k).cpu().numpy(), R.mask_boxes_outside_range(many, RANGE, k))
    five = _scale_cases()[0]                                     # remove_points_in_boxes3d: the robust 5-box scene, every box taken as it is
    inside = np.any([R.in_box(five["points"][:, :3], b)[0] for b in five["boxes"]], axis=0)
    got = box_utils.remove_points_in_boxes3d(_t(five["points"], cuda), _t(five["boxes"], cuda)).cpu().numpy()
    assert np.array_equal(got, five["points"][~inside]) and 0 < inside.sum() < len(inside)
    rng = np.random.RandomState(32)
    scenes = [dict(points=rng.uniform(-40, 40, (n, 4)).astype(F), boxes=boxes, cls=np.zeros(5, np.int32)) for n in (257, 100)]
    out = A.compact(_batch(scenes, cuda), shuffle=True)["points"].cpu().numpy()
    for b, s in enumerate(scenes):
        got = out[out[:, 0] == b][:, 1:]
        assert not np.array_equal(got, s["points"]) and np.array_equal(got[np.lexsort(got.T)], s["points"][np.lexsort(s["points"].T)])
    assert (np.diff(out[:, 0]) >= 0).all()


# ---------------------------------------------------------------------------------------------------------- end to end
CLASS_NAMES = ["car", "truck", "bus"]
AUG = {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": [
    {"NAME": "random_object_scaling", "SCALE_UNIFORM_NOISE": [0.75, 1.0]},
    {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x", "y"]},
    {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.3925, 0.3925]},
    {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]}                          # tools/cfgs/source-nuscenes/pvrcnn.yaml
PROCESSOR = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
             {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": False, "test": False}},
             {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.1, 0.1, 0.2], "MAX_POINTS_PER_VOXEL": 5, "MAX_NUMBER_OF_VOXELS": {"train": 2000}}]
E2E_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
MIN_POINTS = 30
NAMES = np.array(CLASS_NAMES + ["pedestrian"])


def _cls_of(names):
    return np.array([CLASS_NAMES.index(n) if n in CLASS_NAMES else -1 for n in names])


def _raw_scenes(num_scenes, num_boxes, seed):
    """Scenes of 800 points; names include one class outside CLASS_NAMES; about a third of the boxes hold fewer than MIN_POINTS points."""
    scenes = []
    for b in range(num_scenes):
        rng = np.random.RandomState(seed + b)
        boxes = R.make_boxes(rng, num_boxes, extent=46.0)
        names = NAMES[rng.randint(0, 4, num_boxes)]
        dense = rng.rand(num_boxes) < 0.7
        fg = np.concatenate([R.make_points(rng, boxes[dense], 0, 45, spread=0.52), R.make_points(rng, boxes[~dense], 0, 6)])[:700]
        pts = np.concatenate([fg, R.make_points(rng, boxes[:0], 800 - len(fg), 0, extent=54.0)])
        scenes.append(dict(points=pts[rng.permutation(800)], gt_boxes=boxes, gt_names=names, rng=rng))
    return scenes


E2E_EXTRA = [0.1, 0.1, 0.1]
AUG_GT = {"DISABLE_AUG_LIST": [], "AUG_CONFIG_LIST": [AUG["AUG_CONFIG_LIST"][0],
          {"NAME": "gt_sampling", "PREPARE": {"filter_by_min_points": ["car:5", "truck:5"]}, "SAMPLE_GROUPS": ["car:8", "truck:7", "cyclist:2"],
           "NUM_POINT_FEATURES": 5, "REMOVE_EXTRA_WIDTH": E2E_EXTRA, "LIMIT_WHOLE_SCENE": True}] + AUG["AUG_CONFIG_LIST"][1:]}


def _e2e_database():
    """20 cars and 20 trucks inside a radius of 30 m (their points stay inside the range under every world transform); some hold fewer than 5 points."""
    def make():
        rng = np.random.RandomState(80)
        boxes = R.make_boxes(rng, 40, extent=21.0, min_gap=0.5)
        infos = {"car": [], "truck": [], "bus": []}
        for k, bx in enumerate(boxes):
            n = 3 if k % 7 == 0 else 10 + k
            pts = np.concatenate([rng.uniform(-0.7, 0.7, (n, 3)), rng.uniform(0, 1, (n, 2))], axis=1).astype(F)
            name = "car" if k < 20 else "truck"
            infos[name].append(dict(name=name, box3d_lidar=bx, points=pts, db_index=k, class_index=CLASS_NAMES.index(name), num_points_in_gt=n, difficulty=0))
        return infos, boxes
    return _cached("e2edb", make)


def _e2e_sampler(database=None):
    from seevcn_amd.pcdet.datasets.augmentor.database_sampler import DataBaseSampler
    return DataBaseSampler(None, AUG_GT["AUG_CONFIG_LIST"][1], CLASS_NAMES, _e2e_database()[0], database)


def _e2e_case(num_scenes, num_boxes, seed=50, gt=False):
    """An input point whose augmented image comes within 5e-4 m of a voxel face, or within 1e-3 m of a range limit or of a box face it is tested
    against, is replaced by a fresh point below every box, until every decision of the case is robust."""
    from seevcn_amd.pcdet.datasets.augmentor import draw_params

    def make():
        scenes = _raw_scenes(num_scenes, num_boxes, seed)
        vs = np.array([0.1, 0.1, 0.2])
        for _ in range(10):
            counts = [R.points_in_boxes_count(s["points"], s["gt_boxes"])[0] for s in scenes]
            names = [s["gt_names"][c >= MIN_POINTS] for s, c in zip(scenes, counts)]
            draws = draw_params(np.random.RandomState(seed), AUG_GT if gt else AUG, [len(n) for n in names], _e2e_sampler() if gt else None, names)
            clean = True
            for s, d in zip(scenes, draws):
                pts, _, err, _, (gap, pairs_ok), origin = R.prepare_scene(s["points"], s["gt_boxes"], _cls_of(s["gt_names"]), d, MIN_POINTS, None, 0,
                                                                          extra_width=E2E_EXTRA)
                assert pairs_ok and err.max() < 5e-4             # the coordinate bound stays below both margins
                frac = (pts[:, :3].astype(np.float64) - np.array(E2E_RANGE[:3])) / vs
                near = (np.abs(np.abs(pts[:, :2].astype(np.float64)) - 51.2) < 1e-3).any(axis=1)
                if not gt:
                    near |= (np.abs(frac - np.round(frac)) * vs < 5e-4).any(axis=1)
                assert not near[origin < 0].any()                # (pasted objects sit well inside the range)
                bad = gap < R.ROBUST
                bad[origin[near & (origin >= 0)]] = True
                if bad.any():
                    clean = False
                    fresh = np.concatenate([s["rng"].uniform(-54, 54, (bad.sum(), 2)), s["rng"].uniform(-4.5, -3.0, (bad.sum(), 1)),
                                            s["rng"].uniform(0, 1, (bad.sum(), 2))], axis=1)
                    s["points"][bad] = fresh.astype(F)
            if clean:
                break
        assert clean, "the end-to-end case does not become robust"
        want = []
        for s, d, c in zip(scenes, draws, counts):
            want.append(R.prepare_scene(s["points"], s["gt_boxes"], _cls_of(s["gt_names"]), d, MIN_POINTS, E2E_RANGE, 1, check=False, extra_width=E2E_EXTRA))
            s["num_points_in_gt"] = c
        return scenes, draws, want
    return _cached(("e2e", num_scenes, num_boxes, seed, gt), make)


def _augmentor(database=None):
    from seevcn_amd.pcdet.datasets.augmentor import BatchDataAugmentor
    from seevcn_amd.pcdet.datasets.processor import DataProcessor
    dp = DataProcessor(PROCESSOR, np.array(E2E_RANGE, F), training=True, num_point_features=5)
    if database is None:
        return BatchDataAugmentor(None, AUG, CLASS_NAMES, min_points_of_gt=MIN_POINTS, data_processor=dp), dp
    return BatchDataAugmentor(None, AUG_GT, CLASS_NAMES, min_points_of_gt=MIN_POINTS, data_processor=dp, db_infos=_e2e_database()[0], database=database), dp


def _device_scenes(scenes, dev, with_counts):
    return [dict(points=_t(s["points"], dev), gt_boxes=_t(s["gt_boxes"], dev), gt_names=s["gt_names"],
                 num_points_in_gt=s["num_points_in_gt"] if with_counts else None) for s in scenes]


def test_end_to_end_case_exercises_the_filters():
    scenes, draws, want = _e2e_case(4, 12)
    for s, (pts, gt, err, berr, _, _) in zip(scenes, want):
        assert (s["num_points_in_gt"] < MIN_POINTS).any() and (s["num_points_in_gt"] >= MIN_POINTS).any()
        assert 0 < len(gt) < 12 and len(pts) < 800 and "pedestrian" in s["gt_names"]


@pytest.mark.gpu
def test_batch_augmentor_end_to_end(cuda):
    import torch
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, reset_counters
    from seevcn_amd.pcdet.ops import voxel_ops
    scenes, draws, want = _e2e_case(4, 12)
    aug, dp = _augmentor()
    reset_counters()
    out = aug.forward(_device_scenes(scenes, cuda, False), rng=np.random.RandomState(50))          # counts made on the device
    first = dict(COUNTERS)
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
    assert out["points_per_scene"].tolist() == [len(w[0]) for w in want] and out["empty_scenes"] == []
    # the same draws from the same seed
    for d, e in zip(out["draws"], draws):
        assert [n for n, _ in d] == [n for n, _ in e] and all(np.array_equal(np.asarray(a), np.asarray(b)) for (_, a), (_, b) in zip(d, e))
    # its points voxelise as the restatement's do
    vs, grid = [0.1, 0.1, 0.2], dp.grid_size.tolist()
    a = voxel_ops.voxelize_hard(out["points"], 1, 5, out["points_per_scene"].tolist(), E2E_RANGE, vs, grid, 5, 2000)
    b = voxel_ops.voxelize_hard(_t(ref_pts, cuda), 1, 5, [len(w[0]) for w in want], E2E_RANGE, vs, grid, 5, 2000)
    nv = a[3].cpu().numpy()
    assert np.array_equal(nv, b[3].cpu().numpy()) and nv.min() > 100
    for s in range(4):
        assert torch.equal(a[1][s, :nv[s]], b[1][s, :nv[s]]) and torch.equal(a[2][s, :nv[s]], b[2][s, :nv[s]])
    # the device starts / counts are what voxelize_dynamic and voxelize_hard take
    assert out["scene_cnt"].cpu().numpy().tolist() == out["points_per_scene"].tolist()
    # a second run: equal bits; with the counts given by the infos: one read less, the same result
    again = aug.forward(_device_scenes(scenes, cuda, False), rng=np.random.RandomState(50))
    assert torch.equal(again["points"], out["points"]) and torch.equal(again["gt_boxes"], out["gt_boxes"])
    reset_counters()
    given = aug.forward(_device_scenes(scenes, cuda, True), rng=np.random.RandomState(50))
    assert torch.equal(given["points"], out["points"]) and torch.equal(given["gt_boxes"], out["gt_boxes"])
    assert COUNTERS["host_reads"] == 1 and first["host_reads"] == 2 and first["library_calls"] == COUNTERS["library_calls"] + 1


def test_end_to_end_gt_case_accepts_and_rejects():
    scenes, draws, want = _e2e_case(4, 12, seed=90, gt=True)
    pasted = [int((w[5] < 0).sum()) for w in want]
    cands = [len(d[1][1]) for d in draws]
    assert sum(cands) >= 15 and min(cands) > 0 and all(d[1][0] == "gt_sampling" and d[0][0] == "object_scaling" for d in draws)
    groups = {g for d in draws for g, _ in d[1][1]}
    assert groups == {0, 1} and sum(p > 0 for p in pasted) >= 3                                    # both groups drew; objects were pasted
    assert any(len(w[0]) - p < 800 - 20 for w, p in zip(want, pasted))                             # scene points were removed or cut by the range


def _compare_with_restatement(out, want):
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
    return ref_pts


@pytest.mark.gpu
def test_batch_augmentor_with_gt_sampling(cuda):
    """The source-nuscenes/pvrcnn.yaml list plus gt_sampling (behind random_object_scaling: the reference's gt_sampling removes the gt_boxes_mask
    that its random_object_scaling reads), sample by sample against the restatement, then collated."""
    import torch
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, reset_counters
    from seevcn_amd.pcdet.datasets.augmentor.database_sampler import GtDatabase
    infos, db_boxes = _e2e_database()
    flat = infos["car"] + infos["truck"]
    db = GtDatabase.from_arrays([i["points"] for i in flat], db_boxes, [i["class_index"] for i in flat], cuda)
    scenes, draws, want = _e2e_case(4, 12, seed=90, gt=True)
    aug, _ = _augmentor(db)
    reset_counters()
    out = aug.forward(_device_scenes(scenes, cuda, True), rng=np.random.RandomState(90))
    assert COUNTERS["host_reads"] == 1
    _compare_with_restatement(out, want)
    for d, e in zip(out["draws"], draws):
        assert [(g, i["db_index"]) for g, i in d[1][1]] == [(g, i["db_index"]) for g, i in e[1][1]]
    aug2, _ = _augmentor(db)
    again = aug2.forward(_device_scenes(scenes, cuda, True), rng=np.random.RandomState(90))
    assert torch.equal(again["points"], out["points"]) and torch.equal(again["gt_boxes"], out["gt_boxes"])
    # batch size does not change the number of calls
    calls = COUNTERS["library_calls"]
    aug3, _ = _augmentor(db)
    reset_counters()
    aug3.forward(_device_scenes(scenes[:2], cuda, True), rng=np.random.RandomState(90))
    assert 2 * COUNTERS["library_calls"] == calls and COUNTERS["host_reads"] == 1


@pytest.mark.gpu
def test_configs_without_a_draw_leave_the_scene_alone(cuda):
    """WORLD_SCALE_RANGE narrower than 1e-3 and NOISE_TRANSLATE_STD 0: no draw, no transform; a std > 0 translates points and boxes alike."""
    from seevcn_amd.pcdet.datasets.augmentor import BatchDataAugmentor
    scenes = _raw_scenes(2, 5, 95)
    for s in scenes:
        s["num_points_in_gt"] = np.full(5, 99)
    cfg = [{"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [1.0, 1.0005]},
           {"NAME": "random_world_translation", "NOISE_TRANSLATE_STD": 0, "ALONG_AXIS_LIST": ["x", "y", "z"]}]
    rs = np.random.RandomState(3)
    out = BatchDataAugmentor(None, cfg, list(NAMES)).forward(_device_scenes(scenes, cuda, True), rng=rs)
    assert rs.uniform() == np.random.RandomState(3).uniform() and out["draws"] == [[], []]
    want = [(s["points"], np.concatenate([s["gt_boxes"], (np.array([list(NAMES).index(n) for n in s["gt_names"]]) + 1).astype(F)[:, None]], axis=1)) for s in scenes]
    ref_pts, ref_gt = R.collate(want)
    assert np.array_equal(out["points"].cpu().numpy(), ref_pts) and np.array_equal(out["gt_boxes"].cpu().numpy(), ref_gt)
    cfg[1]["NOISE_TRANSLATE_STD"] = 0.5
    out = BatchDataAugmentor(None, cfg, list(NAMES)).forward(_device_scenes(scenes, cuda, True), rng=np.random.RandomState(3))
    rs = np.random.RandomState(3)
    for b, s in enumerate(scenes):
        off = np.array([rs.normal(0, 0.5, 1)[0] for _ in range(3)])
        got = out["points"].cpu().numpy()[800 * b:800 * (b + 1), 1:4]
        assert np.array_equal(got, (s["points"][:, :3].astype(np.float64) + off).astype(F))
        assert np.array_equal(out["gt_boxes"].cpu().numpy()[b, :, :3], (s["gt_boxes"][:, :3].astype(np.float64) + off).astype(F))


@pytest.mark.gpu
def test_counters_do_not_depend_on_batch_or_boxes(cuda):
    from seevcn_amd.pcdet.datasets.augmentor import COUNTERS, reset_counters
    aug, _ = _augmentor()
    seen = []
    for num_scenes, num_boxes in ((2, 5), (4, 5), (2, 40), (4, 40)):
        scenes = _raw_scenes(num_scenes, num_boxes, 70 + num_boxes)
        for sc in scenes:
            sc["num_points_in_gt"] = R.points_in_boxes_count(sc["points"], sc["gt_boxes"])[0]
        reset_counters()
        aug.forward(_device_scenes(scenes, cuda, True), rng=np.random.RandomState(1))
        seen.append(dict(COUNTERS))
    assert all(c == seen[0] for c in seen) and seen[0]["host_reads"] == 1
