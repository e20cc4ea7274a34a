"""The stated arithmetic of the ray caster (tests/raycast_reference.py) against closed forms, its float32 form against its float64 form, and the
host-side pieces of seevcn_amd.vcn.vc_shapenet.  No GPU."""
import os
import re

import numpy as np
import pytest

import raycast_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    out = R.seeded_cases()
    for c in out:
        c["a32"] = R.brute_force(c["rays"], c["tris"], c["geom_ids"], c["prim_ids"], np.float32)
        c["a64"] = R.brute_force(c["rays"], c["tris"], c["geom_ids"], c["prim_ids"], np.float64)
        c["mask"] = R.jump_mask(c["rays"], c["tris"])
    return out


# ------------------------------------------------------------------ pinhole rays against closed forms
def _angle(a, b):
    return np.degrees(np.arccos(np.clip(a @ b / np.linalg.norm(a) / np.linalg.norm(b), -1, 1)))


@pytest.mark.parametrize("fov", [45, 100, 179])
def test_pinhole_closed_forms(fov):
    center, eye, up, W, H = np.array([3.0, -2.0, 0.5]), np.array([-1.0, 4.0, 2.0]), [0, 0, 1], 7, 5
    M, e, K, Rm = R.pinhole_camera(fov, center, eye, up, W, H)
    assert np.array_equal(e, eye)
    # the image centre looks at `center`; pixel (3, 2) of a 7 x 5 image is that centre
    mid = M @ np.array([W / 2, H / 2, 1.0])
    assert _angle(mid, center - eye) < 1e-6
    rays = R.create_rays_pinhole(fov, center, eye, up, W, H).reshape(H, W, 6)
    assert _angle(rays[2, 3, 3:].astype(np.float64), center - eye) < 1e-4
    assert np.array_equal(rays[..., :3], np.broadcast_to(eye.astype(np.float32), (H, W, 3)))
    # the x = 0 and x = W edges of the middle row subtend the horizontal fov
    left, right = M @ np.array([0.0, H / 2, 1.0]), M @ np.array([float(W), H / 2, 1.0])
    assert abs(_angle(left, right) - fov) < 1e-6
    # M reproduces K and R
    assert np.allclose(np.linalg.inv(M), K @ Rm, rtol=1e-9, atol=1e-9)
    assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and np.linalg.det(Rm) > 0
    assert np.isclose(K[0, 0], 0.5 * W / np.tan(np.radians(fov) / 2)) and K[0, 0] == K[1, 1] and K[0, 2] == W / 2 and K[1, 2] == H / 2
    assert _angle(Rm[2], center - eye) < 1e-6


def test_pinhole_fov_beyond_180_follows_the_arithmetic():
    M, _, K, _ = R.pinhole_camera(190, [5, 0, 0], [0, 0, 0], [0, 0, 1], 8, 4)
    assert K[0, 0] < 0                                          # tan(95 deg) < 0: taken as it comes
    rays = R.create_rays_pinhole(190, [5, 0, 0], [0, 0, 0], [0, 0, 1], 8, 4)
    assert rays.shape == (32, 6) and np.isfinite(rays).all()


def test_rays_are_row_major_y_outer():
    M, eye, _, _ = R.pinhole_camera(60, [4, 1, 0], [0, 0, 1], [0, 0, 1], 5, 3)
    rays = R.pinhole_rays(M, eye, 5, 3)
    want = (M @ np.array([3.5, 1.5, 1.0])).astype(np.float32)   # x = 3, y = 1 -> row 1 * 5 + 3
    assert np.allclose(rays[8, 3:], want, rtol=1e-6)


# ------------------------------------------------------------------ the float64 oracle against analytic answers
def test_oracle_plane_at_known_distance():
    big = np.array([[[-100, -100, 5], [100, -100, 5], [0, 200, 5]]], np.float32)
    rays = R.create_rays_pinhole(70, [0, 0, 5], [0.5, -0.25, 0], [0, 1, 0], 16, 8)
    a = R.brute_force(rays, big, [0], [0], np.float64)
    assert np.isfinite(a["t_hit"]).all() and (a["primitive_ids"] == 0).all()
    assert np.allclose(a["t_hit"], 5.0 / rays[:, 5].astype(np.float64), rtol=1e-12)


def test_oracle_sphere_within_the_chord_error():
    r, c, eye = 1.5, np.array([0.5, -0.25, 0.125]), np.array([7.0, 2.0, 1.0])
    v, f = R.icosphere(3, r, c)
    tris = v[f].astype(np.float64)
    normal = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    r_in = np.abs(((tris[:, 0] - c) * normal).sum(1)).min() * (1 - 1e-6)    # the mesh lies between the spheres of radius r_in and r
    assert 0.98 * r < r_in < r
    rays = R.create_rays_pinhole(35, c, eye, [0, 0, 1], 48, 32)
    a = R.brute_force(rays, v[f], np.zeros(len(f), np.int32), np.arange(len(f)), np.float64)
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)

    def sphere_t(radius):
        oc = o - c
        A, B, C = (d * d).sum(1), 2 * (oc * d).sum(1), (oc * oc).sum(1) - radius * radius
        disc = B * B - 4 * A * C
        return np.where(disc >= 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)

    t_out, t_in = sphere_t(r * (1 + 1e-6)), sphere_t(r_in)
    hit = np.isfinite(a["t_hit"])
    assert hit[np.isfinite(t_in)].all() and not hit[~np.isfinite(t_out)].any() and np.isfinite(t_in).sum() > 200
    inner = np.isfinite(t_in)
    assert (a["t_hit"][inner] >= t_out[inner]).all() and (a["t_hit"][inner] <= t_in[inner]).all()


# ------------------------------------------------------------------ the float32 restatement against the float64 oracle
def test_bands_are_sized_from_the_restatements_own_error(cases):
    duv, dt = R.measure_bands(cases)
    print(f"measured: max |du|, |dv| = {duv:.3g}, max |dt| = {dt:.3g}; bands {R.BAND_UV:g}, {R.BAND_T:g}")
    assert 0 < duv < R.BAND_UV <= 8 * duv and 0 < dt < R.BAND_T <= 8 * dt


def test_float32_restatement_against_float64_oracle(cases):
    for c in cases:
        a32, a64, mask = c["a32"], c["a64"], c["mask"]
        share = mask.mean()
        print(f"{c['name']}: {len(c['tris'])} triangles, {int(np.isfinite(a64['t_hit']).sum())} of {len(mask)} rays hit, mask share {share:.4%}")
        assert share <= R.MASK_CAP, (c["name"], share)
        keep = ~mask
        h32, h64 = np.isfinite(a32["t_hit"]), np.isfinite(a64["t_hit"])
        assert np.array_equal(h32[keep], h64[keep]), c["name"]
        assert np.array_equal(a32["geometry_ids"][keep], a64["geometry_ids"][keep]), c["name"]
        assert np.array_equal(a32["primitive_ids"][keep], a64["primitive_ids"][keep]), c["name"]
        both = keep & h32 & h64
        assert both.sum() > 10, c["name"]
        assert np.abs(a32["t_hit"][both].astype(np.float64) - a64["t_hit"][both]).max() <= R.BAND_T, c["name"]
        assert (a32["geometry_ids"][~h32] == -1).all() and (a32["primitive_ids"][~h32] == -1).all() and np.isinf(a32["t_hit"][~h32]).all()


def test_zero_area_triangles_are_never_hit(cases):
    c = next(c for c in cases if c["name"] == "zero_area")
    e1, e2 = c["tris"][:, 1] - c["tris"][:, 0], c["tris"][:, 2] - c["tris"][:, 0]
    flat = np.flatnonzero(np.abs(np.cross(e1.astype(np.float64), e2.astype(np.float64))).max(1) == 0)
    assert len(flat) >= 6
    assert not np.isin(c["a32"]["primitive_ids"], flat).any() and not np.isin(c["a64"]["primitive_ids"], flat).any()


def test_ties_go_to_the_lowest_geometry_and_primitive():
    tris, gid, pid = R.scene_arrays([R.copies_tris(3), R.copies_tris(2)])
    a = R.brute_force(np.array([[5, 0, 0, -1, 0, 0]], np.float32), tris, gid, pid)
    assert a["t_hit"][0] == 5 and a["geometry_ids"][0] == 0 and a["primitive_ids"][0] == 0


def test_padding_constants_cover_every_accepted_pair(cases):
    """The kernel skips a node only when the ray misses its box grown by RC_PAD * (largest coordinate magnitude).  Every pair the float32 test
    accepts must therefore have its hit point inside the triangle's box grown by that much; here the need is measured on the seeded cases."""
    src = open(os.path.join(ROOT, "see-vcn_amd", "csrc", "raycast.hip")).read()
    pad = re.search(r"RC_PAD = 0x1p-(\d+)f", src)
    slack = re.search(r"RC_TSLACK = 0x1p-(\d+)f", src)
    assert pad and 2.0 ** -int(pad.group(1)) == R.RC_PAD and slack and 2.0 ** -int(slack.group(1)) == R.RC_TSLACK
    worst, pairs = 0.0, 0
    for c in cases:
        w, n = R.padding_residual(c["rays"], c["tris"])
        worst, pairs = max(worst, w), pairs + n
    print(f"accepted pairs {pairs}, worst excursion {worst:.3g} of the coordinate magnitude; RC_PAD {R.RC_PAD:.3g}")
    assert pairs > 10000 and worst < R.RC_PAD / 64


# ------------------------------------------------------------------ host-side pieces of the package
def test_create_cylinder_counts_and_closedness():
    from seevcn_amd.vcn.vc_shapenet import dataset_functions as DF
    for kw in ({}, {"radius": 0.1, "height": 3.0}, {"resolution": 7, "split": 2}):
        v, f = DF.create_cylinder(**kw)
        rv, rf = R.create_cylinder(**kw)
        assert np.array_equal(v, rv) and np.array_equal(f, rf)
        res, split = kw.get("resolution", 20), kw.get("split", 4)
        assert v.shape == (res * (split + 1) + 2, 3) and f.shape == (res * (2 + 2 * split), 3)
        edges = {}
        for a, b, c in f:
            for e in ((a, b), (b, c), (c, a)):
                edges.setdefault((min(e), max(e)), []).append(e)
        assert all(len(es) == 2 and es[0] == es[1][::-1] for es in edges.values())     # closed, and consistently wound
        assert len(np.unique(f)) == len(v)
    v, f = DF.create_cylinder()
    assert v.shape == (102, 3) and f.shape == (200, 3)
    assert np.isclose(v[:, 2].max(), 1.0) and np.isclose(v[:, 2].min(), -1.0) and np.allclose(np.hypot(v[2:, 0], v[2:, 1]), 1.0)


def _cars(n):
    cars = []
    for k in range(n):
        label = np.array([8.0 + 3 * k, -4.0 + 4 * k, -1.2, 4.4, 1.8, 1.4, 0.3 * k])
        cars.append({"label": list(label), "bbox": np.array([[label[0] + sx * 2.2, label[1] + sy * 0.9, label[2] + sz * 0.7]
                                                             for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)])})
    return cars


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_populate_scene_draw_order(seed):
    from seevcn_amd.vcn.vc_shapenet import dataset_functions as DF
    cars = _cars(7)
    signs = {"label": np.array([[20.0, 3.0, 0.5, 0.1, 0.1, 1.0, 0.0], [25.0, -6.0, 0.7, 0.1, 0.1, 1.0, 0.0]])}
    before = signs["label"].copy()
    got = DF.draw_scene_obstacles(cars, signs, np.random.RandomState(seed), random_poles_pct=0.3)
    rng = np.random.RandomState(seed)                           # the reference's sequence of calls (dataset_functions.py:268-306), by hand
    want = []
    for car in cars[:2]:                                        # int(7 * 0.3) = 2
        radius = rng.uniform(0.03, 0.2)
        height = rng.uniform(1, 4, 1)
        which = rng.choice([1, 2, 3])
        lo, hi = car["bbox"].min(0)[:2], car["bbox"].max(0)[:2]
        if rng.choice([True, False]):
            if which == 1:
                xy = np.array([hi[0], car["label"][1]]) + rng.uniform(0, 0.5)
            elif which == 2:
                xy = np.array([car["label"][0], hi[1]]) + rng.uniform(0, 0.5)
            else:
                xy = hi + rng.uniform(0, 1, 2)
        else:
            xy = lo - rng.uniform(0, 1, 2)
        want.append((radius, height[0], np.array([xy[0], xy[1], car["label"][2] + height[0] / 2 - car["label"][5] / 2])))
    for sign in before:
        height = rng.uniform(1, 4, 1)
        radius = rng.uniform(0.03, 0.1)
        want.append((radius, height[0], np.array([sign[0], sign[1], -2.4 + height[0] / 2])))
    assert len(got) == len(want) == 4
    for (r0, h0, c0), (r1, h1, c1) in zip(got, want):
        assert r0 == r1 and h0 == h1 and np.array_equal(c0, c1)
    assert np.array_equal(signs["label"], before)
    assert DF.draw_scene_obstacles(cars, {}, np.random.RandomState(seed), random_poles_pct=0.0) == []


def test_box_helpers():
    from seevcn_amd.vcn.vc_shapenet import dataset_functions as DF
    pts = DF.opd_to_boxpts(np.array([1.0, 2.0, 3.0, 4.0, 2.0, 1.0, 0.0]))
    assert pts.shape == (8, 3) and np.allclose(pts.min(0), [-1, 1, 2.5]) and np.allclose(pts.max(0), [3, 3, 3.5])
    turned = DF.opd_to_boxpts(np.array([0.0, 0.0, 0.0, 4.0, 2.0, 1.0, np.pi / 2]))
    assert np.allclose(np.abs(turned).max(0), [1, 2, 0.5])
    gt = DF.get_gt_for_zero_yaw(pts)
    assert np.allclose(gt["center"], [1, 2, 3]) and np.allclose(gt["dims"], [4, 2, 1]) and np.allclose(np.sort(gt["bbox"], 0), np.sort(pts, 0))


def test_new_ops_refuse_cpu_tensors(hip_lib):
    import torch
    import seevcn_amd._lib as L
    from seevcn_amd.vcn.vc_shapenet import RaycastingScene, raycasting as rc
    scene = RaycastingScene()
    with pytest.raises(L.SeevcnHipError):
        scene.add_triangles(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]))
    with pytest.raises(L.SeevcnHipError):
        scene.add_triangles(np.zeros((3, 3)), np.array([[0, 1, 2]]))
    with pytest.raises(L.SeevcnHipError):
        scene.cast_rays(torch.zeros(4, 6))
    with pytest.raises(L.SeevcnHipError):
        scene.cast_pinhole(torch.zeros(1, 12, dtype=torch.float64), 4, 4)
    with pytest.raises(L.SeevcnHipError):
        rc.rays_pinhole(torch.zeros(1, 12, dtype=torch.float64), 4, 4)
    with pytest.raises(L.SeevcnHipError):
        rc.hit_points(torch.zeros(16), 1, 4, 4, cams=torch.zeros(1, 12, dtype=torch.float64))
    with pytest.raises(L.SeevcnHipError):
        RaycastingScene.create_rays_pinhole(60, [1, 0, 0], [0, 0, 0], [0, 0, 1], 4, 4, device="cpu")


def test_host_refuses_scenes_beyond_the_index_width(hip_lib):
    from seevcn_amd.vcn.vc_shapenet import raycasting as rc
    assert hip_lib.sv_bvh_scratch_bytes(rc.MAX_TRIANGLES) > 0 and hip_lib.sv_bvh_scratch_bytes(rc.MAX_TRIANGLES + 1) == 0
    assert hip_lib.sv_bvh_keys(None, rc.MAX_TRIANGLES + 1, None, None, None, None) != 0
    assert b"index bits" in hip_lib.sv_last_error()
    assert hip_lib.sv_bvh_build(None, None, None, rc.MAX_TRIANGLES + 1, None, None, None, None, None) != 0
    assert hip_lib.sv_ray_hit_points_scratch_bytes(1, 1 << 16, 1 << 15) == 0
