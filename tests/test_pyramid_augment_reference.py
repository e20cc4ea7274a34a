"""tests/pyramid_augment_reference.py (the numpy restatement of random_local_pyramid_aug and its seeded cases) against the reference's own
functions, recorded in tests/golden/pyramid_augment.npz by tests/golden/make_pyramid_augment_golden.py; and the host half of the device entry
(the plans and the queue) against a hand-written replay of the reference's calls.  No GPU."""
import os

import numpy as np
import pytest

import pyramid_augment_reference as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyramid_augment.npz")
_G = {}


def golden():
    if not _G:
        with np.load(GOLDEN) as z:
            _G.update({k: z[k] for k in z.files})
    return _G


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(case):
    return case["boxes"][case["cls"] != -2][:, :7], case["points"][~case["dead"]]


def test_the_golden_holds_the_generators_cases():
    g = golden()
    assert tuple(g["names"]) == PR.GOLDEN_CASES
    for name in PR.GOLDEN_CASES:
        boxes, points = _inputs(PR.cases()[name])
        assert np.array_equal(_bits(g[name + "/boxes"]), _bits(boxes)) and np.array_equal(_bits(g[name + "/points"]), _bits(points))
        cfg = PR.cases()[name]["cfg"]
        assert g[name + "/cfg"].tolist() == [cfg[k] for k in ("DROP_PROB", "SPARSIFY_PROB", "SPARSIFY_MAX_NUM", "SWAP_PROB", "SWAP_MAX_NUM")]
        assert int(g[name + "/seed"]) == PR.cases()[name]["seed"]


def test_discard_share_is_under_the_cap():
    PR.cases()
    assert PR.TALLY.drawn >= 9000 and PR.TALLY.discarded <= PR.MAX_DISCARD * PR.TALLY.drawn
    assert golden()["discarded"].tolist() == [PR.TALLY.discarded, PR.TALLY.drawn]


@pytest.mark.parametrize("name", PR.GOLDEN_CASES)
def test_pyramids_and_plane_membership_equal_the_references(name):
    """get_pyramids bit for bit, and the five-plane test against scipy's Delaunay on every point and every pyramid, with no filtering beyond the
    generator's band; every point is shown to be at least BAND from every plane."""
    g = golden()
    boxes, points = _inputs(PR.cases()[name])
    pyramids = PR.get_pyramids(boxes)
    assert np.array_equal(_bits(pyramids), _bits(g[name + "/pyramids"]))
    mine = PR.points_in_pyramids_mask(points, pyramids)
    theirs = np.unpackbits(g[name + "/masks"], axis=1, count=6 * len(boxes)).astype(bool) if len(boxes) else np.zeros((len(points), 0), bool)
    assert mine.shape == theirs.shape and np.array_equal(mine, theirs)
    for pyramid in pyramids.reshape(-1, 5, 3):
        assert (np.abs(PR.plane_distances(points, pyramid)) >= PR.BAND).all()


@pytest.mark.parametrize("name", PR.GOLDEN_CASES)
def test_restatement_equals_the_reference(name):
    """The same rows in the same order with equal bits after each of the three functions, swapped values included, and the same stream position."""
    g = golden()
    case = PR.cases()[name]
    boxes, points = _inputs(case)
    cfg, rng = case["cfg"], np.random.RandomState(case["seed"])
    _, p1, pyr = PR.local_pyramid_dropout(boxes, points, cfg["DROP_PROB"], rng)
    assert np.array_equal(_bits(p1), _bits(points[g[name + "/after_dropout_rows"]]))
    _, p2, pyr = PR.local_pyramid_sparsify(boxes, p1, cfg["SPARSIFY_PROB"], cfg["SPARSIFY_MAX_NUM"], rng, pyr)
    assert np.array_equal(_bits(p2), _bits(points[g[name + "/after_sparsify_rows"]]))
    _, p3 = PR.local_pyramid_swap(boxes, p2, cfg["SWAP_PROB"], cfg["SWAP_MAX_NUM"], rng, pyr)
    assert p3.shape == g[name + "/after_swap"].shape and np.array_equal(_bits(p3), _bits(g[name + "/after_swap"]))
    assert rng.uniform() == float(g[name + "/next_uniform"])
    whole, _, rng2 = PR.run_case(case)
    assert np.array_equal(_bits(whole), _bits(p3)) and rng2.uniform() == float(g[name + "/next_uniform"])


def test_cases_do_what_they_are_for():
    c, g = PR.cases(), golden()
    n = lambda name, key: len(g[f"{name}/{key}"])
    assert n("self_swap", "after_swap") > n("self_swap", "points")               # a self-swap emits its pyramid twice
    assert n("shared_partner", "after_swap") > n("shared_partner", "points")     # a partner shared by two pairs is emitted per pair
    assert n("all_dropped", "after_sparsify_rows") == n("all_dropped", "after_dropout_rows") < n("all_dropped", "points")
    assert n("all_sparsified", "after_swap") == n("all_sparsified", "after_sparsify_rows") < n("all_sparsified", "points")
    assert n("no_boxes", "after_swap") == n("no_boxes", "points")
    for mx in (0, 5, 50):                                                        # exactly MAX_NUM stays, MAX_NUM + 1 is sparsified / valid
        d = dict(PR.run_case(c[f"sparsify_max{mx}"])[1])
        picked = [(i, int(f)) for i, f in enumerate(d["pyramid_sparsify_face"])]
        fill = np.array([(mx, mx + 1, mx, mx + 1, mx, mx + 1), (mx + 1, mx, mx + 1, mx, mx + 1, mx), (mx + 1, mx + 1, mx, mx, mx + 1, mx + 1)])
        assert len(d["pyramid_sparsify_choice"]) == sum(fill[i, f] > mx for i, f in picked)
        assert n(f"sparsify_max{mx}", "after_sparsify_rows") == n(f"sparsify_max{mx}", "points") - len(d["pyramid_sparsify_choice"])
        assert len(dict(PR.run_case(c[f"swap_max{mx}"])[1])["pyramid_swap_face"]) == 3
    assert (np.abs(c["large"]["boxes"][:2, 6]) > 3.09).all() and (c["large"]["boxes"][:3, 0] > 60).all() and c["large"]["dead"].sum() > 200


def test_swap_of_three_columns_raises():
    case = PR.cases()["columns3_swap"]
    assert str(golden()["columns3_swap/raised"]) == "ValueError"                 # the reference's np.concatenate
    with pytest.raises(ValueError, match="columns"):
        PR.run_case(case)
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A

    class Batch:
        num_point_features = 3

    plan = {"pairs": np.zeros((1, 8), np.int64), "room": np.zeros(1, np.int64)}
    with pytest.raises(ValueError, match="columns"):
        A.local_pyramid_swap(Batch(), plan)


# ---------------------------------------------------------------------------------------------------------- the host half of the device entry
CFG = {"NAME": "random_local_pyramid_aug", "DROP_PROB": 0.25, "SPARSIFY_PROB": 0.05, "SPARSIFY_MAX_NUM": 50, "SWAP_PROB": 0.1, "SWAP_MAX_NUM": 50}


def test_queue_accepts_the_entry_and_refuses_what_it_must():
    from seevcn_amd.pcdet.datasets.augmentor import BatchDataAugmentor, draw_params
    from seevcn_amd.pcdet.datasets.augmentor import data_augmentor as D
    from seevcn_amd.pcdet import model_cfgs
    aug = BatchDataAugmentor(None, [dict(CFG)], ["Car"])
    assert [len(s) for s in aug.stages] == [0, 1, 0] and D._entry_names(CFG) == list(PR.DRAW_NAMES)
    for key in D.PYRAMID_KEYS:
        cfg = {k: v for k, v in CFG.items() if k != key}
        with pytest.raises(NotImplementedError, match=f"random_local_pyramid_aug without {key}"):
            BatchDataAugmentor(None, [cfg], ["Car"])
    with pytest.raises(ValueError, match="one RandomState per scene"):
        draw_params(np.random.RandomState(0), [dict(CFG)], [3])
    # behind the world dropout the pyramid's per-box draws wait for the existing boundary; no empty stage in between
    q = [{"NAME": "random_world_frustum_dropout", "INTENSITY_RANGE": [0, 0.2], "DIRECTION": ["top"]}, dict(CFG),
         {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]}]
    assert [[e["NAME"] for e in s] for s in D._stages(D._queue(q))] == [["random_world_frustum_dropout"], ["random_local_pyramid_aug"],
                                                                          ["random_world_flip"]]
    block = model_cfgs.pointpillar_pyramid_aug_augmentor_cfg()
    assert [e["NAME"] for e in block["AUG_CONFIG_LIST"]] == ["gt_sampling", "random_world_flip", "random_world_rotation", "random_world_scaling",
                                                             "random_local_pyramid_aug"]
    assert {k: block["AUG_CONFIG_LIST"][-1][k] for k in D.PYRAMID_KEYS} == {k: CFG[k] for k in D.PYRAMID_KEYS}
    assert block["AUG_CONFIG_LIST"][0]["USE_ROAD_PLANE"] is False


def _involved(points, pyramids, left, plan):
    """The points inside any pyramid of the plan's pairs (box rows here are indices into the scene's boxes)."""
    hit = np.zeros(len(points), bool)
    for r in plan["pairs"]:
        hit |= PR.member(points, pyramids[r[1], r[2]]) | PR.member(points, pyramids[r[4], r[5]])
    return hit.sum()


@pytest.mark.parametrize("name", ["large", "classes", "shared_partner", "sparsify_max0", "sparsify_max5", "swap_max0", "all_dropped", "no_boxes"])
def test_plans_draw_in_the_references_order(name):
    """A hand-written replay of the reference's calls on one stream -- randint, uniform; randint, uniform, choice(count, MAX, replace=False) per
    valid pyramid; uniform, choice(valid faces) per box, choice(valid boxes) per pair -- with the counts taken from the restatement's masks, against
    plan_pyramid_sparsify / plan_pyramid_swap fed the same counts and against the restatement's own log; the streams end at the same place."""
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    case = PR.cases()[name]
    boxes, points = _inputs(case)
    cfg = case["cfg"]
    pyramids = PR.get_pyramids(boxes).reshape(-1, 6, 5, 3)
    want_points, want, want_rng = PR.run_case(case)
    want = dict(want)
    hand, plan_rng = np.random.RandomState(case["seed"]), np.random.RandomState(case["seed"])
    n = len(boxes)
    # dropout
    f1, u1 = hand.randint(0, 6, n), hand.uniform(0, 1, n)
    assert np.array_equal(f1, plan_rng.randint(0, 6, n)) and np.array_equal(u1, plan_rng.uniform(0, 1, n))
    drop = u1 <= cfg["DROP_PROB"]
    if drop.any():
        points = points[~PR.points_in_pyramids_mask(points, pyramids[drop, f1[drop]]).any(-1)]
    left = np.nonzero(~drop)[0]
    # sparsify
    m = len(left)
    f2, u2 = (hand.randint(0, 6, m), hand.uniform(0, 1, m)) if m else (np.zeros(0, np.int64), np.zeros(0))
    assert np.array_equal(f2, plan_rng.randint(0, 6, m)) and np.array_equal(u2, plan_rng.uniform(0, 1, m))
    sel = u2 <= cfg["SPARSIFY_PROB"]
    counts = PR.points_in_pyramids_mask(points, pyramids).sum(0).reshape(n, 6)
    hand_choices, parts, gone = [], [], np.zeros(len(points), bool)
    for i, f in zip(left[sel], f2[sel]):
        if counts[i, f] > cfg["SPARSIFY_MAX_NUM"]:
            hand_choices.append(hand.choice(counts[i, f], size=cfg["SPARSIFY_MAX_NUM"], replace=False))
            inside = PR.member(points, pyramids[i, f])
            gone |= inside
            parts.append(points[inside][hand_choices[-1]])
    plan = A.plan_pyramid_sparsify(counts, [(left[sel], f2[sel])], cfg["SPARSIFY_MAX_NUM"], [plan_rng])
    assert len(plan["choices"][0]) == len(hand_choices) == len(want["pyramid_sparsify_choice"])
    for a, b, c in zip(plan["choices"][0], hand_choices, want["pyramid_sparsify_choice"]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert plan["room"].tolist() == [len(hand_choices) * cfg["SPARSIFY_MAX_NUM"]]
    assert plan["pyr"][:, 4].tolist() == [t * cfg["SPARSIFY_MAX_NUM"] for t in range(len(hand_choices))]
    replayed = A.plan_pyramid_sparsify(counts, [(left[sel], f2[sel])], cfg["SPARSIFY_MAX_NUM"], None, [plan["choices"][0]])
    assert np.array_equal(replayed["pyr"], plan["pyr"]) and np.array_equal(replayed["ranks"], plan["ranks"])
    points = np.concatenate([points[~gone]] + parts)
    left = left[~sel]
    # swap
    k = len(left)
    u3 = hand.uniform(0, 1, k) if k else np.zeros(0)
    assert np.array_equal(u3, plan_rng.uniform(0, 1, k))
    chosen = u3 <= cfg["SWAP_PROB"]
    counts = PR.points_in_pyramids_mask(points, pyramids).sum(0).reshape(n, 6)
    hand_faces, hand_partners = [], []
    if chosen.any():
        valid = counts[left] > cfg["SWAP_MAX_NUM"]
        pairs = []
        for i in range(k):
            if chosen[i] and valid[i].any():
                pairs.append((i, hand.choice(np.nonzero(valid[i])[0])))
        for i, j in pairs:
            valid[i, j] = False
        for i, j in pairs:
            cand = np.nonzero(valid[:, j])[0]
            hand_partners.append(hand.choice(cand) if len(cand) else i)
        hand_faces = [j for _, j in pairs]
    plan = A.plan_pyramid_swap(counts, [left], [chosen], cfg["SWAP_MAX_NUM"], [plan_rng])
    assert plan["faces"][0].tolist() == [int(j) for j in hand_faces] == want["pyramid_swap_face"].tolist()
    assert plan["partners"][0].tolist() == [int(q) for q in hand_partners] == want["pyramid_swap_partner"].tolist()
    sizes = [int(r[3] + r[6]) for r in plan["pairs"]]
    assert plan["pairs"][:, 7].tolist() == [sum(sizes[:t]) for t in range(len(sizes))]      # the blocks follow each other, pair after pair
    assert plan["room"].tolist() == [sum(sizes)] and len(want_points) == len(points) - int(_involved(points, pyramids, left, plan)) + sum(sizes)
    replayed = A.plan_pyramid_swap(counts, [left], [chosen], cfg["SWAP_MAX_NUM"], None, plan["faces"], plan["partners"])
    assert np.array_equal(replayed["pairs"], plan["pairs"])
    assert np.array_equal(want["pyramid_drop_face"], f1) and np.array_equal(want["pyramid_drop_u"], u1)
    assert np.array_equal(want["pyramid_sparsify_face"], f2) and np.array_equal(want["pyramid_sparsify_u"], u2)
    assert np.array_equal(want["pyramid_swap_u"], u3)
    nxt = want_rng.uniform()
    assert hand.uniform() == nxt and plan_rng.uniform() == nxt


def test_replayed_draws_that_do_not_fit_the_counts_raise():
    from seevcn_amd.pcdet.datasets.augmentor import augmentor_utils as A
    counts = np.array([[9, 0, 0, 0, 0, 0], [7, 7, 0, 0, 0, 0]])
    with pytest.raises(ValueError, match="distinct"):
        A.plan_pyramid_sparsify(counts, [(np.array([0]), np.array([0]))], 3, None, [[np.array([1, 1, 2])]])
    with pytest.raises(ValueError, match="distinct"):
        A.plan_pyramid_sparsify(counts, [(np.array([0]), np.array([0]))], 3, None, [[np.array([1, 2, 9])]])
    with pytest.raises(ValueError, match="pyramid_sparsify_choice"):
        A.plan_pyramid_sparsify(counts, [(np.array([0]), np.array([0]))], 3, None, [[]])
    with pytest.raises(ValueError, match="pyramid_swap_face"):
        A.plan_pyramid_swap(counts, [np.array([0, 1])], [np.array([True, False])], 5, None, [np.array([1])], [np.array([1])])
    with pytest.raises(ValueError, match="pyramid_swap_partner"):
        A.plan_pyramid_swap(counts, [np.array([0, 1])], [np.array([True, False])], 5, None, [np.array([0])], [np.array([0])])
    with pytest.raises(ValueError, match="SPARSIFY_MAX_NUM"):
        A.plan_pyramid_sparsify(counts, [], 5000, [])
