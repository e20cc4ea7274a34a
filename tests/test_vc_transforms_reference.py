"""CPU: the numpy restatement of the VC training transforms (tests/vc_transforms_reference.py) and the host planners of
seevcn_amd.vcn.datasets.data_transforms against the reference's own outputs (tests/golden/vc_transforms.npz)."""
import os

import numpy as np
import pytest

import vc_transforms_reference as V
from seevcn_amd.vcn.datasets import data_transforms as T


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "vc_transforms.npz")))
    g["clouds"] = np.split(g["points"], np.cumsum(g["counts"])[:-1])
    return g


def _split(rows, lengths):
    return np.split(rows, np.cumsum(lengths)[:-1])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_committed_clouds_are_the_generators(gold):
    names, clouds = V.make_cases()
    assert list(gold["names"]) == names and len(names) == 14
    assert [len(c) for c in clouds] == [99, 100, 101, 256, 257, 1024, 1025, 4097, 150, 200, 300, 120, 400, 300]
    for a, b in zip(clouds, gold["clouds"]):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(V.make_boxes(clouds), gold["gtbox"])


def test_maker_assertions_hold_on_the_committed_file(gold):
    for name, c in zip(gold["names"], gold["clouds"]):
        assert (np.abs(c).sum(1) > 0).all(), f"{name} holds the origin"
        e = V.elevation(c)
        for bins, min_in in (('sqrt', 100), (50, 50)):
            if len(c) >= min_in:
                assert V.edge_distance_ulps(e, bins) >= 64, (name, bins)
    assert {"out", "onetwo", "onetwo_fallback", "original", "small"} == set(gold["lidar_exit"])
    assert {"out", "original"} == set(gold["ds_exit"])
    for key in ("lidar", "ds", "dropout"):
        for name, c, rows in zip(gold["names"], gold["clouds"], _split(gold[key + "_out"], gold[key + "_len"])):
            assert V.is_ordered_subset(rows, c), (key, name)
            r = np.linalg.norm(rows.astype(np.float64), axis=1, keepdims=True)
            assert not (np.abs(rows) < 2.0 ** -24 * r).any(), (key, name)


def test_bin_counts_at_the_thresholds(gold):
    want = {"n100": 10, "n101": 11, "n256": 16, "n257": 17, "n1024": 32, "n1025": 33, "n4097": 65}
    for name, c in zip(gold["names"], gold["clouds"]):
        if name in want:
            e = V.elevation(c)
            assert V.bin_count(e, 'sqrt') == want[name] == len(np.histogram(e, bins='sqrt')[0])


def test_ring_index_equals_histogram_and_digitize(gold):
    """The edge rule against the two numpy calls the reference makes."""
    for name, c in zip(gold["names"], gold["clouds"]):
        e = V.elevation(c)
        for bins in ('sqrt', 50):
            hist = np.histogram(e, bins=bins)
            want = np.digitize(e, hist[1][np.argwhere(hist[0] > 0).squeeze(1)])
            ring, num_rings, ring_cnt = V.ring_index(e, bins)
            assert np.array_equal(ring, want), (name, bins)
            assert num_rings == want.max() and np.array_equal(np.unique(want), np.arange(1, num_rings + 1))
            assert np.array_equal(ring_cnt[:num_rings], np.unique(want, return_counts=True)[1]) and not ring_cnt[num_rings:].any()
    e = V.elevation(gold["clouds"][list(gold["names"]).index("lone_top")])
    assert V.ring_index(e)[0][np.argmax(e)] == V.ring_index(e)[1]            # the maximum belongs to the last bin


@pytest.mark.parametrize("key,bins,planner,min_in", [("lidar", 'sqrt', T.plan_lidar_simulation, 100), ("ds", 50, T.plan_downsample_rings, 50)])
def test_planners_reproduce_every_golden_length_exit_and_row(gold, key, bins, planner, min_in):
    for i, (name, c) in enumerate(zip(gold["names"], gold["clouds"])):
        ring, num_rings, ring_cnt = V.ring_table(c, bins, min_in)
        plan, length = planner(np.random.RandomState(int(gold[key + "_seed"][i])), len(c), num_rings, ring_cnt)
        assert length == gold[key + "_len"][i], name
        assert plan["exit"] == gold[key + "_exit"][i], name
        rows = V.select(c, ring, plan)
        assert np.array_equal(_bits(rows), _bits(_split(gold[key + "_out"], gold[key + "_len"])[i])), name


def test_downsample_rings_raises_on_one_ring(gold):
    i = list(gold["names"]).index("copies120")
    ring, num_rings, ring_cnt = V.ring_table(gold["clouds"][i], 50, 50)
    assert num_rings == 1
    with pytest.raises(ValueError):
        T.plan_downsample_rings(np.random.RandomState(int(gold["ds_raise_seed"])), 120, num_rings, ring_cnt)


def test_host_draws_reproduce_dropout_resample_jitter_gn(gold):
    drop, gn_at = _split(gold["dropout_out"], gold["dropout_len"]), 0
    jit = _split(gold["jitter_out"], gold["counts"])
    for i, c in enumerate(gold["clouds"]):
        mask = T.draw_point_dropout(np.random.RandomState(100 + i), len(c), 0.2)
        assert np.array_equal(_bits(c[mask]), _bits(drop[i]))
        idx = T.draw_resample(np.random.RandomState(200 + i), len(c), V.N_POINTS)
        assert np.array_equal(_bits(c[idx % len(c)]), _bits(gold["resample_out"][i]))
        noise = T.draw_jitter(np.random.RandomState(300 + i), len(c), 0.01, 0.05)
        assert np.array_equal(_bits(V.jitter(c, noise).astype(np.float32)), _bits(jit[i]))
        if i in gold["gn_cases"]:
            noise = T.draw_gn_spherical(np.random.RandomState(400 + i), len(c))
            ref = gold["gn_out"][gn_at:gn_at + len(c)]
            gn_at += len(c)
            mine = c.astype(np.float64) if noise is None else V.gn_spherical(c, noise)
            r = np.linalg.norm(ref, axis=1, keepdims=True)
            assert (np.abs(mine - ref) <= 1e-14 * r).all()


def test_rigid_restatement_and_draws_against_the_reference(gold):
    """Sample 0's points (float64 restatement against the reference's fp32 matmul: the bound of the GPU test) and every sample's box."""
    c, comp, box = gold["clouds"][0], gold["complete"][0], gold["gtbox"][0]
    for name, axis in (("flipx", "flip_x"), ("flipy", "flip_y")):
        op, enable = T.draw_world_flip(np.random.RandomState(int(gold[name + "_seed"][0])), 'X' if axis == "flip_x" else 'Y')
        assert op == axis and enable
        assert np.array_equal(V.world_flip(c, axis), gold[name + "_partial0"]) and np.array_equal(V.world_flip(comp, axis), gold[name + "_complete0"])
        assert np.allclose(V.flip_box(box, axis), gold[name + "_gtbox"][0], rtol=0, atol=1e-12)
    angle = T.draw_global_rotation(np.random.RandomState(int(gold["rot_seed"][0])), [-0.78539816, 0.78539816])
    for p, key in ((c, "rot_partial0"), (comp, "rot_complete0")):
        ref, mag = V.rotate_z(p, angle)
        assert (np.abs(gold[key] - ref) <= 4 * 2.0 ** -24 * mag + V.ulp32(ref)).all()
    s = T.draw_global_scaling(np.random.RandomState(int(gold["gscale_seed"][0])), [0.95, 1.05])
    assert np.allclose(gold["gscale_partial0"], c.astype(np.float64) * s, rtol=1e-15, atol=0)
    assert np.allclose(gold["gscale_gtbox"][0], np.concatenate([box[:6] * s, box[6:]]), rtol=0, atol=1e-12)
    s3 = T.draw_object_scaling(np.random.RandomState(int(gold["oscale_seed"][0])), [0.9, 1.1])
    assert s3 is not None
    for p, key in ((c, "oscale_partial0"), (comp, "oscale_complete0")):
        ref, mag = V.object_scaling(p, box, s3)
        assert (np.abs(gold[key] - ref) <= V.OBJECT_SCALE_UNITS * 2.0 ** -24 * mag + V.ulp32(ref)).all()
    assert np.allclose(gold["oscale_gtbox"][0], np.concatenate([box[:3], box[3:6] * s3, box[6:]]), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name,cls,params", [("flipx", T.RandomWorldFlip, {'along_axis': 'X'}), ("flipy", T.RandomWorldFlip, {'along_axis': 'Y'}),
                                             ("rot", T.GlobalRotation, {'rot_range': [-0.78539816, 0.78539816]}),
                                             ("gscale", T.GlobalScaling, {'scale_range': [0.95, 1.05]}),
                                             ("oscale", T.RandomObjectScaling, {'scale_range': [0.9, 1.1]})])
def test_boxes_of_every_sample(gold, name, cls, params):
    """The host half of the rigid and scale transforms (a batch without clouds launches nothing)."""
    out = cls(params)({"gtbox": gold["gtbox"].copy()}, [np.random.RandomState(int(s)) for s in gold[name + "_seed"]])
    assert np.allclose(out["gtbox"], gold[name + "_gtbox"], rtol=0, atol=1e-12)
    assert not np.array_equal(out["gtbox"], gold["gtbox"])


def test_compose_refuses_what_is_not_built():
    for name in ("PeriodicSampling", "RandomSamplePoints", "RandomMirrorPoints", "NormalizeObjectPose"):
        with pytest.raises(NotImplementedError):
            T.BatchCompose([{'callback': name, 'objects': ['partial']}])


def test_whole_queue_on_the_host_tables(gold):
    """Compose's stream: rnd_value, LidarSimulation's draws, rnd_value, the permutation."""
    for i, c in enumerate(gold["clouds"]):
        rng = np.random.RandomState(int(gold["queue_seed"][i]))
        rng.uniform(0, 1)
        ring, num_rings, ring_cnt = V.ring_table(c, 'sqrt', 100)
        plan, length = T.plan_lidar_simulation(rng, len(c), num_rings, ring_cnt)
        rows = V.select(c, ring, plan)
        assert len(rows) == length
        rng.uniform(0, 1)
        idx = T.draw_resample(rng, len(rows), V.N_POINTS)
        assert np.array_equal(_bits(rows[idx % len(rows)]), _bits(gold["queue_out"][i])), gold["names"][i]
