"""csrc/raycast.hip and seevcn_amd.vcn.vc_shapenet against the float32 brute-force restatement (tests/raycast_reference.py): bit for bit, no
exemption.  Images are at most 64 x 32, scenes at most 1 360 triangles; the hit-point compaction is also held at the tile edge of its chunk
scan, on images of 256 x 1023 .. 2049 rays of a two-triangle mesh."""
import numpy as np
import pytest

import raycast_reference as R

pytestmark = pytest.mark.gpu

A = np.array([[5, 0, 0], [5, 1, 0], [5, 0, 1]], np.float32)     # two triangles of the plane x = 5 that share the edge (5, 1, 0) - (5, 0, 1)
B = np.array([[5, 1, 0], [5, 1, 1], [5, 0, 1]], np.float32)


def _soup(n, seed):
    """n small triangles scattered in a 4 x 2 x 1.5 box: they overlap and occlude one another."""
    rng = np.random.RandomState(seed)
    c = rng.uniform([-2, -1, -0.75], [2, 1, 0.75], (n, 1, 3))
    return (c + rng.uniform(-0.25, 0.25, (n, 3, 3))).astype(np.float32)


def _aimed(origin, targets):
    o = np.broadcast_to(np.asarray(origin, np.float32), (len(targets), 3))
    return np.ascontiguousarray(np.concatenate([o, np.asarray(targets, np.float32) - o], 1))


def _edge_rays():
    """Rays aimed exactly at points of the shared edge and at the shared vertices (dyadic coordinates: the arithmetic is exact, the two
    triangles tie), from two origins, plus rays that start on triangle A (t exactly 0)."""
    k = np.arange(0, 17, dtype=np.float32) / 16
    on_edge = np.stack([np.full_like(k, 5), 1 - k, k], 1)       # k = 0 and k = 1 are the shared vertices
    rays = [_aimed((0, 0.5, 0.5), on_edge), _aimed((1, 2, -1), on_edge)]
    start = np.array([[5, 0.25, 0.25], [5, 0.5, 0.5], [5, 0, 0], [5, 0.125, 0.5]], np.float32)
    rays.append(np.concatenate([start, np.broadcast_to(np.array([1, 0, 0], np.float32), start.shape)], 1))
    rays.append(np.concatenate([start, np.broadcast_to(np.array([-1, 0.5, 0.25], np.float32), start.shape)], 1))
    return np.concatenate(rays)


def _parallel_rays():
    """Rays parallel to the plane z = 1 of a triangle: in the plane and beside it; and rays in the plane of a tilted triangle, through it."""
    flat = [[x, -1, z, 0.25, 1, 0] for x in (0.1, 0.3, 0.7) for z in (1, 0.5, 1.5)]
    tilted = [[-1, y, 1 - 0.5 * y, 1, 0, 0] for y in (0.125, 0.25, 0.5, 0.75)] + [[-1, 0.25, 0.875, 2, 0.5, -0.25]]
    return np.array(flat + tilted, np.float32)


def scenes():
    """name -> (meshes, camera (fov, centre, eye, up, W, H), extra rays or None)"""
    sphere3 = R.icosphere(3, 1.0, (0, 0, 0), (2.2, 0.9, 0.7))
    sphere2 = R.icosphere(2, 1.5, (0.25, 0, 0))
    sv, sf = R.icosphere(1, 1.0, (0, 0, 0), (1.5, 1, 0.8))
    pole = R.create_cylinder(0.1, 3.0)
    car = R.icosphere(2, 1.0, (0, 0, 0), (2.2, 0.9, 0.7))
    cam = (40, (0, 0, 0), (7, 3, 2), (0, 0, 1), 64, 32)
    out = {
        "one_triangle": ([A], (30, (5, 0.3, 0.3), (0, 0, 0), (0, 0, 1), 64, 32), None),
        "empty": ([], cam, None),
        "icosphere_1280": ([sphere3], cam, None),
        "strip_300": ([R.strip_tris(300)], (40, (30, 0, 0.5), (-5, -3, 2), (0, 0, 1), 64, 32), None),
        "equal_centroids_33": ([R.copies_tris(33)], (20, (0, 0, 0), (9, 2, 1), (0, 0, 1), 64, 32), None),
        "equal_centroids_two_geometries": ([R.copies_tris(5), R.copies_tris(70)], (20, (0, 0, 0), (9, 2, 1), (0, 0, 1), 32, 16), None),
        "zero_area_mixed": ([R.with_zero_area(sv, sf)], (25, (0, 0, 0), (-8, 3, 2), (0, 0, 1), 64, 32), None),
        "shared_edge": ([A, B], (25, (5, 0.5, 0.5), (0, 0.5, 0.5), (0, 0, 1), 64, 32), _edge_rays()),
        "shared_edge_swapped": ([B, A], (25, (5, 0.5, 0.5), (0, 0.5, 0.5), (0, 0, 1), 64, 32), _edge_rays()),
        "occluder": ([A + np.float32([3, 0, 0]), A + np.float32([-2, 0, 0]), A], (20, (5, 0.3, 0.3), (0, 0.2, 0.2), (0, 0, 1), 64, 32), None),
        "origin_inside": ([sphere2], (100, (3, 0.5, 0.25), (0.25, 0, 0), (0, 0, 1), 64, 32), None),
        "parallel": ([np.array([[[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[0, 0, 1], [1, 0, 1], [0, 1, 0.5]]], np.float32)],
                     (30, (0.3, 0.3, 1), (-3, -2, 1), (0, 0, 1), 64, 32), _parallel_rays()),
        "car_and_poles": ([(car[0] + np.float32([10, 2, -1]), car[1]), ((pole[0] + (8, 1.5, -0.5)).astype(np.float32), pole[1]),
                           R.box_mesh((12, 4, -1), (1, 1, 2))], (25, (10, 2, -1), (0, 0, 0), (0, 0, 1), 64, 32), None),
    }
    for n in (2, 3, 63, 64, 65, 255, 256, 257):
        out[f"soup_{n}"] = ([_soup(n, n)], (35, (0, 0, 0), (6, -3, 1.5), (0, 0, 1), 64, 32), None)
    return out


SCENES = scenes()
_reference = {}


def reference(name):
    """The restatement's answers for a scene, computed once and shared: the camera's rays, then the extra rays."""
    if name not in _reference:
        meshes, cam, extra = SCENES[name]
        tris, gid, pid = R.scene_arrays(meshes)
        rays = R.create_rays_pinhole(*cam)
        allrays = rays if extra is None else np.concatenate([rays, extra])
        ans = R.brute_force(allrays, tris, gid, pid, np.float32)
        for v in ans.values():
            v.setflags(write=False)
        _reference[name] = {"tris": tris, "rays": allrays, "n_cam": len(rays), "ans": ans}
    return _reference[name]


def device_scene(meshes, dev):
    import torch
    from seevcn_amd.vcn.vc_shapenet import RaycastingScene
    scene = RaycastingScene()
    for g, m in enumerate(meshes):
        t, _, _ = R.scene_arrays([m])
        gid = scene.add_triangles(torch.from_numpy(t.reshape(-1, 3)).to(dev), torch.arange(3 * len(t), device=dev).reshape(-1, 3))
        assert gid == g
    return scene


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_answer(got, want, sl=slice(None), what=""):
    for k in ("t_hit", "geometry_ids", "primitive_ids", "primitive_uvs"):
        g, w = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k], want[k][sl]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero((bits(g) != bits(w)).reshape(len(w), -1).any(1))
        assert len(bad) == 0, f"{what}: {k} differs at {len(bad)} of {len(w)} rays, first {bad[:5]}: {g[bad[:5]]} vs {w[bad[:5]]}"


def cams_tensor(cams, dev):
    from seevcn_amd.vcn.vc_shapenet import raycasting as rc
    return rc.cameras_to_device([rc.pinhole_camera(*c) for c in cams], dev)


# ------------------------------------------------------------------ sv_cast_rays and sv_cast_pinhole against brute force
@pytest.mark.parametrize("name", sorted(SCENES))
def test_cast_equals_brute_force(cuda, name):
    import torch
    meshes, cam, extra = SCENES[name]
    ref = reference(name)
    scene = device_scene(meshes, cuda)
    n_hit = int(np.isfinite(ref["ans"]["t_hit"]).sum())
    print(f"{name}: {len(ref['tris'])} triangles, {n_hit} of {len(ref['rays'])} rays hit")
    if name == "empty":
        assert n_hit == 0
    else:
        assert n_hit > (3 if name in ("soup_2", "soup_3") else 20)
    got = scene.cast_rays(torch.from_numpy(ref["rays"]).to(cuda))
    assert_same_answer(got, ref["ans"], what=name + " cast_rays")
    got = scene.cast_pinhole(cams_tensor([cam], cuda), cam[4], cam[5])
    assert_same_answer(got, ref["ans"], slice(0, ref["n_cam"]), what=name + " cast_pinhole")
    assert scene.status.cpu().tolist() == [0, 0]


def test_ties_go_to_the_lower_ids(cuda):
    """The rays aimed at the shared edge hit both triangles at the same t: the answer is geometry 0 whichever triangle that is."""
    for name in ("shared_edge", "shared_edge_swapped"):
        ref = reference(name)
        extra = slice(ref["n_cam"], ref["n_cam"] + 34)
        assert (ref["ans"]["geometry_ids"][extra] == 0).all() and (ref["ans"]["t_hit"][extra][:17] == 1).all()
        start = slice(ref["n_cam"] + 34, ref["n_cam"] + 38)
        assert (ref["ans"]["t_hit"][start] == 0).all()          # the origin on a triangle: t exactly 0 is a hit
    ref = reference("equal_centroids_two_geometries")
    hit = np.isfinite(ref["ans"]["t_hit"])
    assert hit.sum() > 20 and (ref["ans"]["geometry_ids"][hit] == 0).all() and (ref["ans"]["primitive_ids"][hit] == 0).all()
    ref = reference("occluder")
    hit = np.isfinite(ref["ans"]["t_hit"])
    assert set(ref["ans"]["geometry_ids"][hit]) == {1}          # the nearest of the three parallel triangles, listed second


@pytest.mark.parametrize("n", [1, 63, 65])
def test_ray_counts(cuda, n):
    import torch
    ref = reference("icosphere_1280")
    pick = np.flatnonzero(np.isfinite(ref["ans"]["t_hit"]))[:: max(1, 400 // n)][:n]
    assert len(pick) == n
    scene = device_scene(SCENES["icosphere_1280"][0], cuda)
    got = scene.cast_rays(torch.from_numpy(ref["rays"][pick]).to(cuda))
    assert_same_answer(got, {k: v[pick] for k, v in ref["ans"].items()}, what=f"{n} rays")
    shaped = scene.cast_rays(torch.from_numpy(ref["rays"][:64].reshape(8, 8, 6)).to(cuda))
    assert shaped["t_hit"].shape == (8, 8) and shaped["primitive_uvs"].shape == (8, 8, 2)


@pytest.mark.parametrize("wh", [(1, 1), (7, 5), (9, 8), (64, 32)])
def test_image_sizes_and_several_cameras_in_one_launch(cuda, wh):
    """3 cameras with different fov values, 179 included, in one launch, at image sizes that are no multiple of the 8 x 8 tile."""
    W, H = wh
    meshes = SCENES["car_and_poles"][0]
    tris, gid, pid = R.scene_arrays(meshes)
    cams = [(30, (10, 2, -1), (0, 0, 0), (0, 0, 1), W, H), (179, (10, 2, -1), (1, -1, 0.5), (0, 0, 1), W, H), (75, (9, 1, -1), (14, 8, 1), (0, 1, 0), W, H)]
    rays = np.concatenate([R.create_rays_pinhole(*c) for c in cams])
    want = R.brute_force(rays, tris, gid, pid, np.float32)
    if W * H > 1:
        assert np.isfinite(want["t_hit"]).any()
    scene = device_scene(meshes, cuda)
    got = scene.cast_pinhole(cams_tensor(cams, cuda), W, H)
    assert_same_answer(got, want, what=f"3 cameras {W} x {H}")


# ------------------------------------------------------------------ sv_rays_pinhole
@pytest.mark.parametrize("fov", [20, 60, 100, 179, 190])
def test_rays_pinhole_bit_equal(cuda, fov):
    from seevcn_amd.vcn.vc_shapenet import RaycastingScene
    for W, H, center, eye, up in ((64, 32, (10, 2, -1), (0, 0, 0), (0, 0, 1)), (7, 5, (0, 0, 0), (1, 1, -1), (0, 1, 0)), (1, 1, (3, 0, 0), (0, 0, 2.4), (0, 0, 1))):
        got = RaycastingScene.create_rays_pinhole(fov, center, eye, up, W, H, device=cuda)
        want = R.create_rays_pinhole(fov, center, eye, up, W, H).reshape(H, W, 6)
        assert got.shape == (H, W, 6) and got.dtype.is_floating_point
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))


# ------------------------------------------------------------------ sv_ray_hit_points
# the in-box flag is an fp32 test on fp32 hit points: it may differ from the float64 test only within 64 ulp of the largest coordinate (20 m
# here: 64 * 2^-24 * 20 = 7.6e-5 m) of a face
FACE_BAND = 64 * 2.0 ** -24 * 20


def test_hit_points_order_flags_and_counts(cuda):
    import torch
    from seevcn_amd.vcn.vc_shapenet import raycasting as rc
    meshes = SCENES["car_and_poles"][0]
    tris, gid, pid = R.scene_arrays(meshes)
    W, H = 64, 32
    wall = np.array([[[20, -90, -90], [20, 90, -90], [20, 0, 90]]], np.float32)
    cams = [(30, (10, 2, -1), (0, 0, 0), (0, 0, 1), W, H),      # the car, a pole in front of it and the box behind
            (40, (-10, 0, 0), (0, 0, 0), (0, 0, 1), W, H),       # looks away: no hit
            (50, (10, 3, -1), (0, 1, 0), (0, 0, 1), W, H),
            (20, (20, 0, 0), (0, 0, 0), (0, 0, 1), W, H)]        # a wall fills the image: every ray hits
    tris = np.concatenate([tris, wall])
    gid, pid = np.concatenate([gid, [3]]).astype(np.int32), np.concatenate([pid, [0]]).astype(np.int32)
    boxes = np.array([[10, 2, -1, 4.4, 1.8, 1.4, 0.0], [10, 2, -1, 4.4, 1.8, 1.4, 0.0], [10, 2, -1, 4.0, 1.2, 1.0, 0.4], [20, 0, 0, 2, 3, 3, 0.2]], np.float32)
    scene = device_scene(meshes + [wall], cuda)
    camt = cams_tensor(cams, cuda)
    ans = scene.cast_pinhole(camt, W, H)
    pts, flags, obj, counts = rc.hit_points(ans["t_hit"], len(cams), W, H, cams=camt, boxes=torch.from_numpy(boxes).to(cuda))
    counts = counts.cpu().numpy()
    pts, flags, obj = pts.cpu().numpy(), flags.cpu().numpy(), obj.cpu().numpy()
    at = at_in = 0
    for c, cam in enumerate(cams):
        rays = R.create_rays_pinhole(*cam)
        want = R.brute_force(rays, tris, gid, pid, np.float32)
        assert np.array_equal(bits(ans["t_hit"].cpu().numpy()[c * W * H:(c + 1) * W * H]), bits(want["t_hit"]))
        wp = R.hit_points(rays, want["t_hit"])
        n = len(wp)
        assert counts[0, c] == n, (c, counts, n)
        assert np.array_equal(bits(pts[at:at + n]), bits(wp))   # bit for bit, in ray order
        inside, face = R.in_box(wp, boxes[c])
        sure = face > FACE_BAND
        f = flags[at:at + n]
        assert np.array_equal(f[sure] != 0, inside[sure]) and set(np.unique(f)) <= {0, 1}
        assert counts[1, c] == f.sum()
        assert np.array_equal(bits(obj[at_in:at_in + f.sum()]), bits(wp[f != 0]))
        at, at_in = at + n, at_in + int(f.sum())
    assert counts[0, 1] == 0 and counts[1, 1] == 0 and counts[0, 3] == W * H
    assert 0 < counts[1, 0] < counts[0, 0] and 0 < counts[1, 3] < W * H
    # the same from a ray tensor, as one segment, without boxes
    rays0 = R.create_rays_pinhole(*cams[0])
    t0 = ans["t_hit"][:W * H].contiguous()
    p2, f2, _, c2 = rc.hit_points(t0, 1, W * H, 1, rays=torch.from_numpy(rays0).to(cuda))
    n0 = int(counts[0, 0])
    assert c2.cpu().tolist() == [[n0], [0]] and np.array_equal(bits(p2.cpu().numpy()[:n0]), bits(pts[:n0])) and not f2.cpu().numpy()[:n0].any()


# One workgroup scans the chunk counts (a chunk: 256 rays) in tiles of 1024 with a carry: images of 256 x H rays make H chunks a camera.  The
# trapezoid fills part of every image row, the last one included, and narrows from row to row: every chunk counts and the counts differ.
TILE_QUAD = np.array([[[5, -1.7, -15], [5, 1.7, -15], [5, 0.2, 15]], [[5, -1.7, -15], [5, 0.2, 15], [5, -0.2, 15]]], np.float32)
TILE_BOX = np.array([5, 0.26, 0, 1, 0.6, 40, 0.3], np.float32)    # of every row's hits some are inside and some outside


def _assert_hit_points_equal_the_restatement(cuda, cams, boxes, W, H, last_tile_from):
    """Counts, order and flags of sv_ray_hit_points for TILE_QUAD against the restatement; the integer work (counts, ranks) exactly."""
    import torch
    from seevcn_amd.vcn.vc_shapenet import raycasting as rc
    tris, gid, pid = R.scene_arrays([TILE_QUAD])
    scene = device_scene([TILE_QUAD], cuda)
    camt = cams_tensor(cams, cuda)
    ans = scene.cast_pinhole(camt, W, H)
    pts, flags, obj, counts = rc.hit_points(ans["t_hit"], len(cams), W, H, cams=camt, boxes=torch.from_numpy(boxes).to(cuda))
    t_hit, counts = ans["t_hit"].cpu().numpy(), counts.cpu().numpy()
    pts, flags, obj = pts.cpu().numpy(), flags.cpu().numpy(), obj.cpu().numpy()
    at = at_in = chunk = 0
    for c, cam in enumerate(cams):
        rays = R.create_rays_pinhole(*cam)
        want = R.brute_force(rays, tris, gid, pid, np.float32, chunk=1 << 16)
        assert np.array_equal(bits(t_hit[c * W * H:(c + 1) * W * H]), bits(want["t_hit"]))
        per_chunk = np.add.reduceat(np.isfinite(want["t_hit"]), np.arange(0, W * H, 256))
        assert per_chunk.min() > 0 and len(set(per_chunk)) > 8, c     # no empty chunk: each one moves the offsets behind it
        chunk += len(per_chunk)
        wp = R.hit_points(rays, want["t_hit"])
        n = len(wp)
        assert counts[0, c] == n, (c, counts, n)
        assert np.array_equal(bits(pts[at:at + n]), bits(wp))       # bit for bit, in ray order
        inside, face = R.in_box(wp, boxes[c])
        sure = face > FACE_BAND
        f = flags[at:at + n]
        assert np.array_equal(f[sure] != 0, inside[sure]) and set(np.unique(f)) == {0, 1}
        assert counts[1, c] == f.sum()
        assert np.array_equal(bits(obj[at_in:at_in + f.sum()]), bits(wp[f != 0]))
        if c == len(cams) - 1 and last_tile_from is not None:       # hits and in-box hits behind the first 1024 chunks of the launch
            tail = f[np.isfinite(want["t_hit"])[:last_tile_from * 256].sum():]
            assert chunk > 1024 and 0 < tail.sum() < len(tail)
        at, at_in = at + n, at_in + int(f.sum())


@pytest.mark.parametrize("H", [1023, 1024, 1025, 2049])
def test_hit_points_chunk_scan_at_its_tile_edge(cuda, H):
    """One camera of 256 x H rays: 1023, 1024, 1025 and 2049 chunks -- below, at and one past the tile of the scan, and into its third tile."""
    cams = [(40, (5, 0, 0), (0, 0, 0), (0, 0, 1), 256, H)]
    _assert_hit_points_equal_the_restatement(cuda, cams, TILE_BOX[None], 256, H, 1024 if H > 1024 else None)


def test_hit_points_chunk_scan_carries_across_cameras(cuda):
    """Five cameras of 205 chunks each: 1025 in all, so the last camera's last chunk lies behind the scan's first tile."""
    cams = [(40 + 3 * c, (5, 0, 0), (0, 0.1 * c, 0), (0, 0, 1), 256, 205) for c in range(5)]
    boxes = np.stack([TILE_BOX + np.float32([0, 0.05 * c, 0, 0, 0, 0, 0]) for c in range(5)])
    _assert_hit_points_equal_the_restatement(cuda, cams, boxes, 256, 205, 204)


# ------------------------------------------------------------------ RaycastingScene
def test_scene_rebuilds_after_add_and_counts_ids_per_geometry(cuda):
    import torch
    import seevcn_amd._lib as L
    meshes = SCENES["car_and_poles"][0]
    cam = SCENES["car_and_poles"][1]
    rays = R.create_rays_pinhole(*cam)
    rt = torch.from_numpy(rays).to(cuda)
    scene = device_scene(meshes[:1], cuda)
    assert scene.builds == 0
    got = scene.cast_rays(rt)
    assert scene.builds == 1
    assert_same_answer(got, R.brute_force(rays, *R.scene_arrays(meshes[:1]), np.float32), what="one geometry")
    scene.cast_rays(rt)
    assert scene.builds == 1                                    # nothing added: no rebuild
    for m in meshes[1:]:
        t, _, _ = R.scene_arrays([m])
        scene.add_triangles(torch.from_numpy(t.reshape(-1, 3)).to(cuda), torch.arange(3 * len(t), device=cuda).reshape(-1, 3))
    got = scene.cast_rays(rt)
    assert scene.builds == 2
    want = R.brute_force(rays, *R.scene_arrays(meshes), np.float32)
    assert_same_answer(got, want, what="three geometries")
    g, p = got["geometry_ids"].cpu().numpy(), got["primitive_ids"].cpu().numpy()
    assert set(np.unique(g)) == {-1, 0, 1} or set(np.unique(g)) == {-1, 0, 1, 2}
    assert p[g == 1].max() < 200 and p[g == 0].max() >= 200     # primitive ids count within the geometry
    # indexed vertices, as add_triangles takes them
    v, f = R.icosphere(1, 1.0, (10, 2, -1))
    indexed = device_scene([], cuda)
    indexed.add_triangles(torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda))
    assert_same_answer(indexed.cast_rays(rt), R.brute_force(rays, *R.scene_arrays([(v, f)]), np.float32), what="indexed")
    # a vertex that is not finite: the scene is refused
    bad = device_scene([np.array([[[0, 0, 0], [1, 0, 0], [0, np.nan, 0]]], np.float32)], cuda)
    with pytest.raises(L.SeevcnHipError):
        bad.cast_rays(rt[:4])


# ------------------------------------------------------------------ the frame and the surface
def _frame():
    cars = []
    for k, (centre, yaw) in enumerate([((9.0, 1.5, -1.2), 0.0), ((13.0, -5.0, -1.0), 0.5), ((7.0, 6.0, -1.1), -1.1)]):
        v, f = R.icosphere(2, 1.0, (0, 0, 0), (2.2, 0.9, 0.7))
        rmat = np.array([[np.cos(yaw), np.sin(yaw), 0], [-np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        label = list(centre) + [4.4, 1.8, 1.4, yaw]
        bbox = np.array([[sx * 2.2, sy * 0.9, sz * 0.7] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]) @ rmat + np.array(centre)
        cars.append({"vertices": (v.astype(np.float64) @ rmat + np.array(centre)).astype(np.float32), "triangles": f, "label": label, "bbox": bbox})
    return cars


def test_raycast_frame_against_the_restatement_car_by_car(cuda):
    from seevcn_amd.vcn.vc_shapenet import dataset_functions as DF, raycasting as rc
    cars = _frame()
    H, W = 32, 64
    runs = []
    for _ in range(2):
        rng = np.random.RandomState(7)
        rc.reset_counters()
        scene = DF.populate_scene(cars, {}, rng, random_poles_pct=0.7, device=cuda)      # int(3 * 0.7) = 2 poles
        out = DF.raycast_frame(cars, scene, rng, aspect_ratio=2, height_px=H)
        assert rc.COUNTERS["host_reads"] == 1 and rc.COUNTERS["library_calls"] == 4      # keys, build, cast, hit points: whatever the frame holds
        runs.append(out)
    # the restatement: the same draws, the scene in the reference's geometry order, one car at a time
    rng = np.random.RandomState(7)
    poles = DF.draw_scene_obstacles(cars, {}, rng, 0.7)
    assert len(poles) == 2
    meshes = []
    for i, car in enumerate(cars):
        meshes.append((car["vertices"], car["triangles"]))
        if i < 2:
            v, f = R.create_cylinder(poles[i][0], poles[i][1])
            meshes.append(((v + poles[i][2]).astype(np.float32), f))
    tris, gid, pid = R.scene_arrays(meshes)
    assert len(tris) == 3 * 320 + 2 * 200
    for car, got in zip(cars, runs[0]):
        fov = rng.normal(60, 30)
        assert got["fov_deg"] == fov
        rays = R.create_rays_pinhole(fov, car["label"][:3], [0, 0, 0], [0, 0, 1], W, H)
        want = R.hit_points(rays, R.brute_force(rays, tris, gid, pid, np.float32)["t_hit"])
        ray_pts, obj_pts = got["ray_pts"].cpu().numpy(), got["obj_pts"].cpu().numpy()
        assert got["num_ray_pts"] == len(want) > 50 and np.array_equal(bits(ray_pts), bits(want))
        inside, face = R.in_box(want, np.asarray(car["label"], np.float32))
        sure = face > FACE_BAND
        # obj_pts is the in-box subsequence of ray_pts: recover the flags by walking both
        flag, j = np.zeros(len(want), bool), 0
        for i in range(len(want)):
            if j < len(obj_pts) and np.array_equal(bits(ray_pts[i]), bits(obj_pts[j])):
                flag[i], j = True, j + 1
        assert j == len(obj_pts) == got["num_obj_pts"] > 10
        assert np.array_equal(flag[sure], inside[sure])
    # two runs: equal bits
    for a, b in zip(*runs):
        assert a["num_ray_pts"] == b["num_ray_pts"] and a["num_obj_pts"] == b["num_obj_pts"] and a["fov_deg"] == b["fov_deg"]
        assert np.array_equal(bits(a["ray_pts"].cpu().numpy()), bits(b["ray_pts"].cpu().numpy()))
        assert np.array_equal(bits(a["obj_pts"].cpu().numpy()), bits(b["obj_pts"].cpu().numpy()))


def test_raycast_object_and_cast_rays_at_point(cuda):
    from seevcn_amd.vcn.vc_shapenet import dataset_functions as DF
    cars = _frame()
    scene = DF.populate_scene(cars, {}, np.random.RandomState(3), random_poles_pct=0.0, device=cuda)
    tris, gid, pid = R.scene_arrays([(c["vertices"], c["triangles"]) for c in cars])
    pts = DF.cast_rays_at_point(scene, cars[1]["label"][:3], fov_deg=40, aspect_ratio=2, height_px=16).cpu().numpy()
    rays = R.create_rays_pinhole(40, cars[1]["label"][:3], [0, 0, 0], [0, 0, 1], 32, 16)
    want = R.hit_points(rays, R.brute_force(rays, tris, gid, pid, np.float32)["t_hit"])
    assert len(want) > 10 and np.array_equal(bits(pts), bits(want))
    one = DF.raycast_object(cars[0], scene, np.random.RandomState(11), height_px=16)
    assert one["fov_deg"] == np.random.RandomState(11).normal(60, 30) and one["ray_pts"].shape == (one["num_ray_pts"], 3)


def test_get_object_surface(cuda):
    import torch
    from seevcn_amd.vcn.utils import misc
    from seevcn_amd.vcn.vc_shapenet import raycast_surface_from_meshes as RS
    v, f = R.icosphere(2, 0.4, (0, 0, 0), (1.0, 0.35, 0.3))
    scene = device_scene([(v, f)], cuda)
    W, H = 32, 24
    surface, views = RS.get_object_surface(scene, complete_pts=64, width_px=W, height_px=H, return_views=True)
    tris, gid, pid = R.scene_arrays([(v, f)])
    want = []
    for eye in RS.EYES:
        rays = R.create_rays_pinhole(45, [0, 0, 0], eye, [0, 1, 0], W, H)
        want.append(R.hit_points(rays, R.brute_force(rays, tris, gid, pid, np.float32)["t_hit"]))
    assert RS.EYES[:2] == [[1, 1, 1], [-1, 1, 1]] and RS.EYES[8:] == [[0, 0, -1], [0, 0, 1], [-1, 0, 0], [1, 0, 0]] and len(RS.EYES) == 12
    want = np.concatenate(want)
    assert len(want) > 64 and np.array_equal(bits(views.cpu().numpy()), bits(want))
    thinned = misc.fps(torch.from_numpy(want).to(cuda).unsqueeze(0), 64).squeeze(0)
    assert surface.shape == (64, 3) and torch.equal(surface, thinned)
    one = RS.generate_views(scene, RS.EYES[2], width_px=W, height_px=H).cpu().numpy()
    rays = R.create_rays_pinhole(45, [0, 0, 0], RS.EYES[2], [0, 1, 0], W, H)
    assert np.array_equal(bits(one), bits(R.hit_points(rays, R.brute_force(rays, tris, gid, pid, np.float32)["t_hit"])))
