"""GPU: the VC training transforms on the device (csrc/lidar_sim.hip, seevcn_amd.vcn.datasets.data_transforms) against the reference's outputs
(tests/golden/vc_transforms.npz) and the numpy restatement (tests/vc_transforms_reference.py), on the golden's 14 clouds as one batch and one by one.

What rests on the device's float64 atan2, which nothing pins against the host's: the ring indices.  The golden's clouds keep every elevation (but a
cloud's minimum and maximum, which are edges themselves) at least 64 ulps from every inner bin edge; test_elevation_band holds the device to 16."""
import os

import numpy as np
import pytest
import torch

import vc_transforms_reference as V
from seevcn_amd import _lib as L
from seevcn_amd.vcn.datasets import data_transforms as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "vc_transforms.npz")))
    g["clouds"] = np.split(g["points"], np.cumsum(g["counts"])[:-1])
    return g


@pytest.fixture(scope="module")
def tables(gold):
    """The restatement's ring tables, computed once: {(bins, min_in_pts): [(ring, num_rings, ring_cnt) per cloud]}."""
    return {(bins, m): [V.ring_table(c, bins, m) for c in gold["clouds"]] for bins, m in (('sqrt', 100), (50, 50))}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _split(rows, lengths):
    return np.split(rows, np.cumsum(lengths)[:-1])


def _groups(n):
    """The whole batch, then every sample alone."""
    return [list(range(n))] + [[i] for i in range(n)]


def _stack(gold, idx, dev, key="clouds"):
    rows = [gold[key][i] for i in idx]
    return T.StackedClouds(torch.from_numpy(np.concatenate(rows)).to(dev), [len(r) for r in rows])


def _rngs(seeds, idx):
    return [np.random.RandomState(int(seeds[i])) for i in idx]


@pytest.mark.parametrize("bins,fixed,min_in", [('sqrt', 0, 100), (50, 50, 50)])
def test_ring_indices(cuda, gold, tables, bins, fixed, min_in):
    for idx in _groups(14):
        clouds = _stack(gold, idx, cuda)
        ring, table, _ = T.vc_rings(clouds, fixed, min_in)
        num_rings, ring_cnt = T.read_ring_table(table, len(idx))
        for k, (i, got) in enumerate(zip(idx, _split(ring.cpu().numpy(), clouds.counts))):
            want_ring, want_n, want_cnt = tables[(bins, min_in)][i]
            assert num_rings[k] == want_n, gold["names"][i]
            assert np.array_equal(ring_cnt[k], want_cnt), gold["names"][i]
            assert np.array_equal(got, want_ring), gold["names"][i]


def test_elevation_band(cuda, gold):
    """The device's float64 elevations within 16 ulps of numpy's: a quarter of the 64-ulp band the golden's clouds keep from the inner edges."""
    clouds = _stack(gold, range(14), cuda)
    ring, table, elev = T.vc_rings(clouds, 0, 0, with_elevation=True)
    ring2, table2, _ = T.vc_rings(clouds, 0, 0)                  # without the buffer the bin pass computes the elevations again
    assert torch.equal(ring, ring2) and torch.equal(table, table2)
    want = V.elevation(gold["points"])
    ulps = float((np.abs(elev.cpu().numpy() - want) / np.spacing(want)).max())
    print(f"largest elevation difference, device atan2 against numpy: {ulps:.2f} ulps over {len(want)} points")
    assert ulps <= 16


@pytest.mark.parametrize("key,cls,params", [("lidar", T.LidarSimulation, {}), ("ds", T.DownsampleRings, {}),
                                            ("dropout", T.RandomPointDropout, {'point_dropout': 0.2})])
def test_selection(cuda, gold, key, cls, params):
    seeds = gold[key + "_seed"] if key != "dropout" else 100 + np.arange(14)
    want = _split(gold[key + "_out"], gold[key + "_len"])
    tr = cls(params)
    for idx in _groups(14):
        out = tr(_stack(gold, idx, cuda), _rngs(seeds, idx))
        assert np.array_equal(out.counts, gold[key + "_len"][idx])
        for i, got in zip(idx, _split(out.points.cpu().numpy(), out.counts)):
            assert np.array_equal(_bits(got), _bits(want[i])), (key, gold["names"][i])
        if key != "dropout":
            assert tr.exits == [gold[key + "_exit"][i] for i in idx]


def test_downsample_rings_one_ring_raises(cuda, gold):
    i = list(gold["names"]).index("copies120")
    with pytest.raises(ValueError):
        T.DownsampleRings({})(_stack(gold, [i], cuda), [np.random.RandomState(int(gold["ds_raise_seed"]))])


def test_resample(cuda, gold):
    tr = T.BatchResamplePoints({'n_points': V.N_POINTS})
    for idx in _groups(14):
        out = tr(_stack(gold, idx, cuda), _rngs(200 + np.arange(14), idx))
        got = out.points.view(len(idx), V.N_POINTS, 3).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(gold["resample_out"][idx]))


def test_jitter(cuda, gold):
    tr = T.Jitter({'sigma': 0.01, 'clip': 0.05})
    for idx in _groups(14):
        out = tr(_stack(gold, idx, cuda), _rngs(300 + np.arange(14), idx))
        want = np.concatenate([_split(gold["jitter_out"], gold["counts"])[i] for i in idx])
        assert np.array_equal(_bits(out.points.cpu().numpy()), _bits(want))


def test_add_gn_spherical(cuda, gold):
    """|ours - ref64| <= ulp32(ref) / 2 + 1e-12 r: one rounding to fp32, and two float64 routes that differ by a few 1e-16 r.  The reference's own
    float64 output for the clouds the golden holds, the restatement's spherical route for all."""
    tr = T.AddGNSpherical({})
    gn_ref = dict(zip(gold["gn_cases"], _split(gold["gn_out"], gold["counts"][gold["gn_cases"]])))
    enabled = 0
    for idx in _groups(14):
        out = tr(_stack(gold, idx, cuda), _rngs(400 + np.arange(14), idx))
        for i, got in zip(idx, _split(out.points.cpu().numpy().astype(np.float64), out.counts)):
            c = gold["clouds"][i]
            noise = T.draw_gn_spherical(np.random.RandomState(400 + i), len(c))
            if noise is None:
                assert np.array_equal(_bits(got), _bits(c))
                continue
            enabled += 1
            for ref in [V.gn_spherical(c, noise)] + ([gn_ref[i]] if i in gn_ref else []):
                r = np.linalg.norm(ref, axis=1, keepdims=True)
                assert (np.abs(got - ref) <= V.ulp32(ref) / 2 + 1e-12 * r).all(), gold["names"][i]
    assert enabled >= 14


def test_add_gn_spherical_at_the_origin(cuda):
    pts = T.StackedClouds(torch.tensor([[0., 0., 0.], [3., 4., 12.]], device=cuda), [2])
    T.vc_pointwise(pts, np.array([0.25, 1.0]), 1)
    f = (13.0 + 1.0) / 13.0
    assert np.array_equal(pts.points.cpu().numpy(), np.array([[0, 0, 0.25], [3 * f, 4 * f, 12 * f]]).astype(np.float32))


def _batch(gold, idx, dev):
    p, c = _stack(gold, idx, dev), _stack(gold, idx, dev, "complete")
    return {"partial": p, "complete": c, "gtbox": gold["gtbox"][idx].copy()}


RIGID = [("flipx", T.RandomWorldFlip, {'along_axis': 'X'}), ("flipy", T.RandomWorldFlip, {'along_axis': 'Y'}),
         ("rot", T.GlobalRotation, {'rot_range': [-0.78539816, 0.78539816]}), ("gscale", T.GlobalScaling, {'scale_range': [0.95, 1.05]}),
         ("oscale", T.RandomObjectScaling, {'scale_range': [0.9, 1.1]})]


def _rigid_expected(name, params, seed, p, box):
    """(float64 points, per-element bound) of the restatement for one sample."""
    rng, p64 = np.random.RandomState(int(seed)), p.astype(np.float64)
    if name in ("flipx", "flipy"):
        op, enable = T.draw_world_flip(rng, params['along_axis'])
        return (V.world_flip(p, op) if enable else p64), np.zeros_like(p64)
    if name == "rot":
        ref, mag = V.rotate_z(p, T.draw_global_rotation(rng, params['rot_range']))
        return ref, 4 * 2.0 ** -24 * mag + V.ulp32(ref)              # the reference's fp32 matmul with fp32 cos / sin
    if name == "gscale":
        ref = p64 * T.draw_global_scaling(rng, params['scale_range'])
        return ref, 2 * 2.0 ** -24 * np.abs(ref) + V.ulp32(ref)       # the factor rounded to fp32, one fp32 product
    s3 = T.draw_object_scaling(rng, params['scale_range'])
    if s3 is None:
        return p64, np.zeros_like(p64)
    ref, mag = V.object_scaling(p, box, s3)
    return ref, V.OBJECT_SCALE_UNITS * 2.0 ** -24 * mag + V.ulp32(ref)


@pytest.mark.parametrize("name,cls,params", RIGID)
def test_rigid_and_scale_transforms(cuda, gold, name, cls, params):
    tr, seeds = cls(params), gold[name + "_seed"]
    for idx in _groups(14):
        out = tr(_batch(gold, idx, cuda), _rngs(seeds, idx))
        assert np.allclose(out["gtbox"], gold[name + "_gtbox"][idx], rtol=0, atol=1e-12)
        for key, src in (("partial", "clouds"), ("complete", "complete")):
            for i, got in zip(idx, _split(out[key].points.cpu().numpy().astype(np.float64), out[key].counts)):
                ref, bound = _rigid_expected(name, params, seeds[i], gold[src][i], gold["gtbox"][i])
                assert (np.abs(got - ref) <= bound).all(), (name, key, gold["names"][i])


def _queue_batch(gold, idx, dev):
    return {"partial": torch.from_numpy(np.concatenate([gold["clouds"][i] for i in idx])).to(dev), "partial_cnt": gold["counts"][idx],
            "complete": torch.from_numpy(gold["complete"][idx].reshape(-1, 3)).to(dev), "complete_cnt": [64] * len(idx), "gtbox": gold["gtbox"][idx]}


def test_whole_queue(cuda, gold):
    compose = T.BatchCompose(V.VC_CARS_TRAIN)
    results = []
    for idx in _groups(14) + [list(range(14))]:
        T.reset_counters()
        out = compose.forward(_queue_batch(gold, idx, cuda), _rngs(gold["queue_seed"], idx))
        assert T.COUNTERS == {"library_calls": 3, "host_reads": 1}, (len(idx), T.COUNTERS)
        assert tuple(out["partial"].shape) == (len(idx), V.N_POINTS, 3)
        got = out["partial"].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(gold["queue_out"][idx])), [gold["names"][i] for i in idx]
        assert np.array_equal(_bits(out["complete"].cpu().numpy()), _bits(gold["complete"][idx].reshape(-1, 3)))
        assert np.array_equal(out["gtbox"], gold["gtbox"][idx])
        results.append(got)
    assert np.array_equal(_bits(results[0]), _bits(np.concatenate(results[1:15])))        # the batch equals the one-by-one results
    assert np.array_equal(_bits(results[0]), _bits(results[15]))                           # two runs, equal bits


def test_queue_refuses_cpu_tensors_empty_objects_and_oversize(cuda, gold):
    compose = T.BatchCompose(V.VC_CARS_TRAIN)
    with pytest.raises(L.SeevcnHipError):
        compose.forward({"partial": torch.from_numpy(gold["clouds"][1]), "partial_cnt": [100]}, [np.random.RandomState(0)])
    with pytest.raises(ValueError):
        compose.forward({"partial": torch.from_numpy(gold["clouds"][1]).to(cuda), "partial_cnt": [100, 0]}, [np.random.RandomState(0)] * 2)
    big = torch.ones((1 << 20) + 1, 3, device=cuda)
    with pytest.raises(ValueError):
        compose.forward({"partial": big, "partial_cnt": [len(big)]}, [np.random.RandomState(0)])
    with pytest.raises(NotImplementedError):
        T.BatchCompose([{'callback': 'PeriodicSampling', 'objects': ['partial']}])
