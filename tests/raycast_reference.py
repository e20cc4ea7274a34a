"""The arithmetic of the mesh ray caster, stated once in numpy (no torch, no GPU).  csrc/raycast.hip follows it statement for statement.

UNPINNED restatements.  open3d is not available to this project's tests, so two things are restated from memory of open3d's sources and not
checked against a run of it: `pinhole_camera` / `pinhole_rays` (open3d.t.geometry.RaycastingScene.create_rays_pinhole(fov_deg, center, eye, up,
width_px, height_px)) and `create_cylinder` (open3d.geometry.TriangleMesh.create_cylinder(radius, height, resolution=20, split=4): 102 vertices,
200 triangles, two cap fans and `split` bands).  Everything else here is the project's own statement: the library is built with
-ffp-contract=off and a correctly rounded fp32 divide, so a sequence of fp32 statements has one answer, and numpy float32 reproduces it.

Pinhole rays, all float64: focal = 0.5 W / tan(0.5 pi / 180 fov_deg) (horizontal fov, never clamped); K = [[focal, 0, 0.5 W], [0, focal, 0.5 H],
[0, 0, 1]]; R row 2 = (center - eye) normalised, row 0 = up x row 2 normalised (up normalised first), row 1 = row 2 x row 0; M = R^-1 K^-1.  Pixel
(x, y) has direction M (x + 0.5, y + 0.5, 1), three explicit products summed left to right, rounded once to float32 and not normalised; the origin
is the eye rounded to float32; rays are row-major, y outer.

Intersection, float32 with one rounding per operation (Moeller-Trumbore, no culling): e1 = v1 - v0, e2 = v2 - v0, p = d x e2, det = e1 . p,
inv = 1 / det, s = o - v0, u = (s . p) inv, q = s x e1, v = (d . q) inv, t = (e2 . q) inv; every cross component is a b - c d with both products
rounded, every dot is ((x + y) + z).  Hit: det != 0 and u >= 0 and v >= 0 and u + v <= 1 and t >= 0 (NaN fails every comparison).  The ray's result
is the smallest t, ties to the lowest (geometry_id, primitive_id); a miss is t = +inf and both ids -1; a hit point is o + d t per component.
"""
import numpy as np

F32, F64 = np.float32, np.float64

# ---- the bands of the jump mask, measured by measure_bands() below on seeded_cases() (fp32 restatement against the fp64 oracle; nothing here comes
# from the kernel).  Measured: max |u32 - u64|, |v32 - v64| over the pairs that decide a ray (in front, not behind the fp64 hit, within 0.25 of the
# triangle) = 7.6e-5; max |t32 - t64| over the rays hit in both = 2.7e-5 at t of 6 - 22.  Both bands are 4 x the measured figure, rounded.
BAND_UV = 3e-4
BAND_T = 1e-4
# the share of a case's rays the mask may exempt (a cap, so that the mask cannot hide a wrong test)
MASK_CAP = 0.005

# the kernel's padding constants (csrc/raycast.hip RC_PAD, RC_TSLACK; DESIGN.md section 3 derives them): test_raycast_reference.py checks on the
# seeded cases that every accepted (ray, triangle) pair has its fp32 hit point inside the triangle's padded box
RC_PAD = 2.0 ** -11
RC_TSLACK = 2.0 ** -20


# ------------------------------------------------------------------ pinhole rays
def pinhole_camera(fov_deg, center, eye, up, width_px, height_px):
    """(M, eye, K, R), float64."""
    center, eye, up = (np.asarray(a, F64).reshape(3) for a in (center, eye, up))
    focal = 0.5 * width_px / np.tan(0.5 * np.pi / 180.0 * fov_deg)
    K = np.array([[focal, 0.0, 0.5 * width_px], [0.0, focal, 0.5 * height_px], [0.0, 0.0, 1.0]], F64)
    R = np.zeros((3, 3), F64)
    up = up / np.linalg.norm(up)
    R[2] = center - eye
    R[2] = R[2] / np.linalg.norm(R[2])
    R[0] = np.cross(up, R[2])
    R[0] = R[0] / np.linalg.norm(R[0])
    R[1] = np.cross(R[2], R[0])
    M = np.linalg.inv(R) @ np.linalg.inv(K)
    return M, eye.copy(), K, R


def pinhole_rays(M, eye, width_px, height_px):
    """(H * W, 6) float32, row-major with y outer."""
    x, y = np.meshgrid(np.arange(width_px, dtype=F64) + 0.5, np.arange(height_px, dtype=F64) + 0.5)
    d = np.stack([(M[i, 0] * x + M[i, 1] * y) + M[i, 2] * 1.0 for i in range(3)], -1).astype(F32).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(eye, F64).astype(F32), d.shape)
    return np.ascontiguousarray(np.concatenate([o, d], 1))


def create_rays_pinhole(fov_deg, center, eye, up, width_px, height_px):
    M, e, _, _ = pinhole_camera(fov_deg, center, eye, up, width_px, height_px)
    return pinhole_rays(M, e, width_px, height_px)


# ------------------------------------------------------------------ intersection
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pair_terms(rays, tris, dtype):
    """det, u, v, t and the hit verdict of every (ray, triangle) pair, shapes (N, T), in `dtype` arithmetic on the float32 inputs."""
    rays, tris = np.asarray(rays, F32).astype(dtype), np.asarray(tris, F32).astype(dtype)
    o, d = rays[:, None, :3], rays[:, None, 3:]
    v0 = tris[None, :, 0]
    e1, e2 = (tris[:, 1] - tris[:, 0])[None], (tris[:, 2] - tris[:, 0])[None]
    shape = (rays.shape[0], tris.shape[0], 3)
    with np.errstate(all="ignore"):
        p = _cross(np.broadcast_to(d, shape), np.broadcast_to(e2, shape))
        det = _dot(e1, p)
        inv = dtype(1) / det
        s = o - v0
        u = _dot(s, p) * inv
        q = _cross(s, np.broadcast_to(e1, shape))
        v = _dot(d, q) * inv
        t = _dot(e2, q) * inv
        hit = (det != 0) & (u >= 0) & (v >= 0) & ((u + v) <= 1) & (t >= 0)
    return det, u, v, t, hit


def brute_force(rays, tris, geom_ids, prim_ids, dtype=F32, chunk=256):
    """The same statements over every (ray, triangle) pair.  tris (T, 3, 3) in scene order (geometry-major, so the lowest index is the lowest
    (geometry_id, primitive_id)).  Returns a dict with open3d's keys, t_hit in `dtype`."""
    rays = np.asarray(rays, F32).reshape(-1, 6)
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    N, T = len(rays), len(tris)
    t_hit = np.full(N, np.inf, dtype)
    idx = np.full(N, -1, np.int64)
    uv = np.zeros((N, 2), dtype)
    if T:
        for a in range(0, N, chunk):
            _, u, v, t, hit = pair_terms(rays[a:a + chunk], tris, dtype)
            t = np.where(hit, t, np.inf)
            k = t.argmin(1)                                     # the first minimum: the lowest index among equal t
            r = np.arange(len(k))
            found = np.isfinite(t[r, k])
            t_hit[a:a + chunk] = t[r, k]
            idx[a:a + chunk] = np.where(found, k, -1)
            uv[a:a + chunk] = np.where(found[:, None], np.stack([u[r, k], v[r, k]], -1), 0)
    geom = np.where(idx >= 0, np.asarray(geom_ids, np.int64)[idx], -1).astype(np.int32) if T else np.full(N, -1, np.int32)
    prim = np.where(idx >= 0, np.asarray(prim_ids, np.int64)[idx], -1).astype(np.int32) if T else np.full(N, -1, np.int32)
    return {"t_hit": t_hit, "geometry_ids": geom, "primitive_ids": prim, "primitive_uvs": uv}


def hit_points(rays, t_hit):
    """rays[hit][:, :3] + rays[hit][:, 3:] * t_hit[hit], float32, in ray order."""
    rays, t = np.asarray(rays, F32), np.asarray(t_hit, F32)
    hit = np.isfinite(t)
    return rays[hit][:, :3] + rays[hit][:, 3:] * t[hit].reshape(-1, 1)


def in_box(points, box):
    """(inside, distance to the nearest face) in float64 by the test of csrc/box_test.h without a margin: box [x, y, z, l, w, h, yaw]."""
    p, b = np.asarray(points, F64).reshape(-1, 3), np.asarray(box, F64)
    sx, sy = p[:, 0] - b[0], p[:, 1] - b[1]
    ca, sa = np.cos(-b[6]), np.sin(-b[6])
    lx, ly, lz = sx * ca + sy * (-sa), sx * sa + sy * ca, p[:, 2] - b[2]
    inside = (np.abs(lz) <= b[5] / 2) & (np.abs(lx) < b[3] / 2) & (np.abs(ly) < b[4] / 2)
    face = np.minimum(np.minimum(np.abs(np.abs(lx) - b[3] / 2), np.abs(np.abs(ly) - b[4] / 2)), np.abs(np.abs(lz) - b[5] / 2))
    return inside, face


# ------------------------------------------------------------------ the jump mask
def jump_mask(rays, tris, band_uv=BAND_UV, band_t=BAND_T, chunk=256):
    """Rays whose float64 result sits on a decision boundary: a triangle that could decide the ray (in front of the origin up to band_t, not
    farther than the nearest hit + band_t) has its smallest barycentric margin min(u, v, 1 - u - v) within band_uv of zero, or lies inside
    with |t| < band_t; or the two nearest hits are closer in t than band_t (and not at the
    same t: copies of one triangle tie in both precisions, and the tie has one answer)."""
    rays = np.asarray(rays, F32).reshape(-1, 6)
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    mask = np.zeros(len(rays), bool)
    if len(tris) == 0:
        return mask
    for a in range(0, len(rays), chunk):
        det, u, v, t, hit = pair_terms(rays[a:a + chunk], tris, F64)
        with np.errstate(all="ignore"):
            m = np.minimum(np.minimum(u, v), 1 - u - v)
            ts = np.sort(np.where(hit, t, np.inf), 1)
            nearest = ts[:, :1]
            live = (det != 0) & (t >= -band_t) & (t <= nearest + band_t)
            edge = live & (np.abs(m) < band_uv)
            origin = (det != 0) & (m >= -band_uv) & (np.abs(t) < band_t)
            gap = ts[:, 1] - ts[:, 0] if ts.shape[1] > 1 else np.full(len(ts), np.inf)
            close = (gap > 0) & (gap < band_t)
        mask[a:a + chunk] = edge.any(1) | origin.any(1) | (close & np.isfinite(ts[:, 0]))
    return mask


def measure_bands(cases=None):
    """(max |du| or |dv|, max |dt|) of the float32 restatement against the float64 oracle on the seeded cases: the figures BAND_UV and BAND_T are
    sized from.  u and v are compared on the pairs that can decide a ray and lie within 0.25 of the triangle, t on the rays hit in both."""
    duv = dt = 0.0
    for case in cases or seeded_cases():
        if len(case["tris"]) == 0:
            continue
        for a in range(0, len(case["rays"]), 256):
            r = case["rays"][a:a + 256]
            d32, u32, v32, t32, h32 = pair_terms(r, case["tris"], F32)
            d64, u64, v64, t64, h64 = pair_terms(r, case["tris"], F64)
            with np.errstate(all="ignore"):
                near = np.where(h64, t64, np.inf).min(1, keepdims=True)
                sel = (d64 != 0) & (t64 >= 0) & (t64 <= near) & (np.minimum(np.minimum(u64, v64), 1 - u64 - v64) > -0.25)
                if sel.any():
                    duv = max(duv, float(np.abs(u32[sel] - u64[sel]).max()), float(np.abs(v32[sel] - v64[sel]).max()))
        a32 = brute_force(case["rays"], case["tris"], case["geom_ids"], case["prim_ids"], F32)["t_hit"]
        a64 = brute_force(case["rays"], case["tris"], case["geom_ids"], case["prim_ids"], F64)["t_hit"]
        both = np.isfinite(a32) & np.isfinite(a64)
        if both.any():
            dt = max(dt, float(np.abs(a32[both].astype(F64) - a64[both]).max()))
    return duv, dt


def padding_residual(rays, tris, chunk=256):
    """For every (ray, triangle) pair the float32 test accepts: how far the point o + d t (t the float32 value, the sum in float64) lies outside
    the triangle's own box, as a share of the largest coordinate magnitude of the ray's origin and that box.  The kernel's culling is
    conservative as long as this stays below RC_PAD.  Returns (max share, accepted pairs)."""
    rays = np.asarray(rays, F32).reshape(-1, 6)
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    lo, hi = tris.min(1).astype(F64), tris.max(1).astype(F64)
    worst, n = 0.0, 0
    for a in range(0, len(rays), chunk):
        r = rays[a:a + chunk]
        _, _, _, t, hit = pair_terms(r, tris, F32)
        i, k = np.nonzero(hit)
        if len(i) == 0:
            continue
        o, d = r[i, :3].astype(F64), r[i, 3:].astype(F64)
        p = o + d * t[i, k].astype(F64)[:, None]
        out = np.maximum(np.maximum(lo[k] - p, p - hi[k]), 0).max(1)
        mag = np.maximum(np.abs(o).max(1), np.maximum(np.abs(lo[k]).max(1), np.abs(hi[k]).max(1)))
        worst, n = max(worst, float((out / mag).max())), n + len(i)
    return worst, n


# ------------------------------------------------------------------ seeded case generators (vertices rounded to float32)
def icosphere(subdivision, radius=1.0, centre=(0, 0, 0), scale=(1, 1, 1)):
    """(vertices (V, 3) float32, triangles (F, 3) int64); an anisotropic `scale` makes a car-like ellipsoid.  20 * 4^subdivision triangles."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, F64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivision):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (v[a] + v[b]) / 2
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.array(v) * radius * np.asarray(scale, F64) + np.asarray(centre, F64)
    return verts.astype(F32), np.array(f, np.int64)


def box_mesh(centre=(0, 0, 0), size=(1, 1, 1)):
    """12 triangles."""
    c, h = np.asarray(centre, F64), np.asarray(size, F64) / 2
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F64) * h + c
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v.astype(F32), np.array(f, np.int64)


def create_cylinder(radius=1.0, height=2.0, resolution=20, split=4):
    """open3d.geometry.TriangleMesh.create_cylinder as recalled (UNPINNED, see the header): the axis is z, centred at the origin; vertex 0 / 1 are
    the top / bottom centres, then split + 1 rings of `resolution` vertices from the top down; two cap fans, then two triangles per band cell.
    Float64 vertices, as open3d's; callers round."""
    v = np.zeros((resolution * (split + 1) + 2, 3), F64)
    v[0] = (0, 0, height * 0.5)
    v[1] = (0, 0, -height * 0.5)
    step, h_step = 2 * np.pi / resolution, height / split
    for i in range(split + 1):
        for j in range(resolution):
            theta = step * j
            v[2 + resolution * i + j] = (np.cos(theta) * radius, np.sin(theta) * radius, height * 0.5 - h_step * i)
    f = []
    for j in range(resolution):
        j1 = (j + 1) % resolution
        f.append((0, 2 + j, 2 + j1))
        base = 2 + resolution * split
        f.append((1, base + j1, base + j))
    for i in range(split):
        base1 = 2 + resolution * i
        base2 = base1 + resolution
        for j in range(resolution):
            j1 = (j + 1) % resolution
            f.append((base2 + j, base1 + j1, base1 + j))
            f.append((base2 + j, base2 + j1, base1 + j1))
    return v, np.array(f, np.int64)


def strip_tris(n, axis=0, step=0.25):
    """n triangles in a row along one axis (the deepest tree: the Morton codes differ in one coordinate only).  (n, 3, 3) float32."""
    t = np.zeros((n, 3, 3), F64)
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3
    for i in range(n):
        t[i, :, a] = (i * step, (i + 1) * step, i * step)
        t[i, :, b] = (0, 0, 1)
        t[i, :, c] = 0.125 * (i % 3)
    return t.astype(F32)


def copies_tris(n, tri=((0, -1, -1), (0, 1, -1), (0, 0, 1))):
    """n copies of one triangle: all centroids, so all Morton codes, are equal."""
    return np.broadcast_to(np.asarray(tri, F32), (n, 3, 3)).copy()


def with_zero_area(verts, faces, every=3):
    """The mesh's triangles (T, 3, 3) float32 with zero-area ones mixed in after every `every`-th: a repeated vertex, three equal vertices, and
    three distinct collinear vertices along an axis (their determinant is exactly zero in float32 as in float64)."""
    t = np.asarray(verts, F32)[faces]
    out = []
    for i, tri in enumerate(t):
        out.append(tri)
        if i % every == 0:
            kind = (i // every) % 3
            if kind == 0:
                out.append(np.stack([tri[0], tri[0], tri[2]]))
            elif kind == 1:
                out.append(np.stack([tri[1], tri[1], tri[1]]))
            else:
                out.append(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F32) + np.round(tri[0]))
    return np.stack(out).astype(F32)


def scene_arrays(meshes):
    """[(verts, faces) or (T, 3, 3) triangles, ...] -> (tris (T, 3, 3) float32, geometry ids, primitive ids): geometry-major, as a scene stores
    them."""
    tris, gid, pid = [], [], []
    for g, m in enumerate(meshes):
        t = np.asarray(m, F32) if not isinstance(m, tuple) else np.asarray(m[0], F32)[np.asarray(m[1])]
        t = t.reshape(-1, 3, 3)
        tris.append(t)
        gid.append(np.full(len(t), g, np.int32))
        pid.append(np.arange(len(t), dtype=np.int32))
    if not tris:
        return np.zeros((0, 3, 3), F32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.concatenate(tris), np.concatenate(gid), np.concatenate(pid)


def _case(name, meshes, fov, centre, eye, up=(0, 0, 1), W=64, H=32):
    tris, gid, pid = scene_arrays(meshes)
    return {"name": name, "tris": tris, "geom_ids": gid, "prim_ids": pid, "rays": create_rays_pinhole(fov, centre, eye, up, W, H),
            "camera": (fov, centre, eye, up, W, H)}


def seeded_cases(seed=0):
    """The cases the float32 restatement is held to the float64 oracle on: six frames of a 320-triangle ellipsoid and an 80-triangle sphere seen
    from 6 - 20 m at fov 20 - 60, then one case per generator.  64 x 32 rays each."""
    rng = np.random.RandomState(seed)
    cases = []
    for k in range(6):
        c = (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 0.5))
        car = icosphere(2, 1.0, c, (2.2, 0.9, 0.7))
        ball = icosphere(1, 0.4, (rng.uniform(-3, 3), rng.uniform(-3, 3), 0))
        eye = np.array([rng.uniform(6, 20) * rng.choice([-1, 1]), rng.uniform(-10, 10), rng.uniform(1, 2.4)])
        cases.append(_case(f"frame{k}", [car, ball], rng.uniform(20, 60), car[0].astype(F64).mean(0), eye))
    cases.append(_case("box", [box_mesh((0.3, -0.2, 0.1), (2, 1, 1.5))], 30, (0.3, -0.2, 0.1), (7, 4, 2)))
    cv, cf = create_cylinder(0.2, 3.0)
    cases.append(_case("cylinder", [((cv + (1, 2, 0.5)).astype(F32), cf)], 25, (1, 2, 0.5), (-6, -3, 1.5)))
    cases.append(_case("strip", [strip_tris(64)], 50, (8, 0, 0.5), (8, -14, 3)))
    cases.append(_case("copies", [copies_tris(16)], 20, (0, 0, 0), (9, 2, 1)))
    sv, sf = icosphere(1, 1.0, (0, 0, 0), (1.5, 1, 0.8))
    cases.append(_case("zero_area", [with_zero_area(sv, sf)], 25, (0, 0, 0), (-8, 3, 2)))
    return cases
