"""RaycastingScene: open3d.t.geometry.RaycastingScene's interface (the reference's vc_shapenet scripts use add_triangles, cast_rays and
create_rays_pinhole) on csrc/raycast.hip.  Arrays in, arrays out: device tensors, no file formats.  The arithmetic is the one
tests/raycast_reference.py states; DESIGN.md section 3 "VC ray casting" has the layout and the derivations.
"""
import numpy as np
import torch

from ... import _lib as L
from ... import data_pipeline as P

# library calls and blocking device -> host reads since the last reset_counters(); neither depends on the number of triangles, cameras or cars
_counted = P.Counted()
COUNTERS, reset_counters, call, host_ints = _counted.counters, _counted.reset, _counted.call, _counted.host_ints
MAX_TRIANGLES = 1 << 24                                         # the sort key holds 24 index bits (csrc/raycast.hip RC_KEY_INDEX_BITS)


def pinhole_camera(fov_deg, center, eye, up, width_px, height_px):
    """The twelve doubles of one camera, made on the host: M = R^-1 K^-1 (row-major) and the eye.  focal = 0.5 W / tan(0.5 pi / 180 fov_deg), the
    fov is horizontal and is never clamped; R rows: up x z normalised, z x row 0, z = (center - eye) normalised."""
    center, eye, up = (np.asarray(a, np.float64).reshape(3) for a in (center, eye, up))
    focal = 0.5 * width_px / np.tan(0.5 * np.pi / 180.0 * fov_deg)
    K = np.array([[focal, 0.0, 0.5 * width_px], [0.0, focal, 0.5 * height_px], [0.0, 0.0, 1.0]], np.float64)
    R = np.zeros((3, 3), np.float64)
    up = up / np.linalg.norm(up)
    R[2] = center - eye
    R[2] = R[2] / np.linalg.norm(R[2])
    R[0] = np.cross(up, R[2])
    R[0] = R[0] / np.linalg.norm(R[0])
    R[1] = np.cross(R[2], R[0])
    M = np.linalg.inv(R) @ np.linalg.inv(K)
    return np.concatenate([M.reshape(9), eye])


def cameras_to_device(cams, device):
    """(C, 12) float64 on the device, one copy."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(cams, np.float64).reshape(-1, 12))).to(device)


def rays_pinhole(cams, width_px, height_px):
    """cams (C, 12) float64 on the device -> (C, H, W, 6) float32."""
    C = cams.shape[0]
    out = torch.empty((C, height_px, width_px, 6), dtype=torch.float32, device=cams.device)
    call("sv_rays_pinhole", L.ptr(cams), C, int(width_px), int(height_px), L.ptr(out))
    return out


def hit_points(t_hit, segments, width_px, height_px, rays=None, cams=None, boxes=None):
    """rays[hit][:, :3] + rays[hit][:, 3:] * t_hit[hit] for `segments` runs of width_px * height_px rays each, in ray order, segment after segment,
    with the in-box crop: (points (N, 3), flags (N,), obj_points (N, 3), counts (2, segments)) on the device, N = all rays; the rows in use are
    the first counts[0].sum() (points, flags) and counts[1].sum() (obj_points).  No host read."""
    dev = t_hit.device
    n = segments * width_px * height_px
    assert t_hit.numel() == n and (rays is None) != (cams is None)
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    obj_points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    flags = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.empty((2, segments), dtype=torch.int32, device=dev)
    nbytes = int(L.load().sv_ray_hit_points_scratch_bytes(segments, int(width_px), int(height_px)))
    if nbytes == 0:
        raise L.SeevcnHipError(f"hit_points: {segments} segments of {width_px} x {height_px} rays exceed the index width (2^31 rays, 65535 segments)")
    scratch = L.workspace.scratch("ray_hit_points", nbytes, dev)
    call("sv_ray_hit_points", L.ptr(rays), L.ptr(cams), segments, int(width_px), int(height_px), L.ptr(t_hit), L.ptr(boxes), L.ptr(scratch), L.ptr(points),
         L.ptr(flags), L.ptr(obj_points), L.ptr(counts))
    return points, flags, obj_points, counts


class RaycastingScene:
    """A set of triangle meshes and the hierarchy over them.  add_triangles(vertices, triangles) returns the geometry id; the hierarchy is rebuilt
    lazily at the next cast.  A scene with more than 2^24 triangles is refused at once, one with a vertex that is not finite at the first host
    read after the build (cast_rays makes that read; the batched paths carry the check on their own single read)."""

    def __init__(self):
        self._meshes = []                                       # (T_g, 3, 3) float32 per geometry
        self._built = None
        self.builds = 0

    # ---- geometry
    def add_triangles(self, vertices, triangles):
        if not (torch.is_tensor(vertices) and torch.is_tensor(triangles)):
            raise L.SeevcnHipError("add_triangles takes device tensors: vertices (V, 3) float, triangles (F, 3) integer")
        L.require_cuda(vertices, triangles)
        assert vertices.dim() == 2 and vertices.shape[1] == 3 and triangles.dim() == 2 and triangles.shape[1] == 3
        tris = vertices.detach().to(torch.float32)[triangles.long()].contiguous()
        if self.num_triangles + tris.shape[0] > MAX_TRIANGLES:
            raise L.SeevcnHipError(f"a scene holds at most {MAX_TRIANGLES} triangles (24 index bits in the sort key)")
        self._meshes.append(tris)
        self._built = None
        return len(self._meshes) - 1

    @property
    def num_triangles(self):
        return sum(int(m.shape[0]) for m in self._meshes)

    @property
    def device(self):
        return self._meshes[0].device if self._meshes else torch.device("cuda", torch.cuda.current_device())

    def _build(self):
        """(nodes, leaves, T, status): three library calls and one torch.sort, whatever T is."""
        if self._built is not None:
            return self._built
        dev = self.device
        T = self.num_triangles
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        nodes = torch.empty((max(T - 1, 1), 16), dtype=torch.float32, device=dev)
        leaves = torch.empty((max(T, 1), 12), dtype=torch.float32, device=dev)
        if T > 0:
            tris = torch.cat(self._meshes) if len(self._meshes) > 1 else self._meshes[0]
            sizes = [int(m.shape[0]) for m in self._meshes]
            geom = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32, device=dev), torch.tensor(sizes, device=dev), output_size=T)
            starts = torch.repeat_interleave(torch.tensor(np.cumsum([0] + sizes[:-1]), dtype=torch.int32, device=dev), torch.tensor(sizes, device=dev),
                                             output_size=T)
            prim = torch.arange(T, dtype=torch.int32, device=dev) - starts
            keys = torch.empty(T, dtype=torch.int64, device=dev)
            scratch = L.workspace.scratch("bvh", int(L.load().sv_bvh_scratch_bytes(T)), dev)
            call("sv_bvh_keys", L.ptr(tris), T, L.ptr(keys), L.ptr(status), L.ptr(scratch))
            keys = torch.sort(keys).values
            call("sv_bvh_build", L.ptr(tris), L.ptr(geom), L.ptr(prim), T, L.ptr(keys), L.ptr(nodes), L.ptr(leaves), L.ptr(scratch))

            def refuse(v):
                if v & 1:
                    self._built = None
                    raise L.SeevcnHipError("RaycastingScene: a vertex is not finite; the scene is refused")

            L.defer_check(status[0:1], refuse)
        self._built = (nodes, leaves, T, status)
        self.builds += 1
        return self._built

    # ---- casting
    @staticmethod
    def _answer(n, dev):
        return {"t_hit": torch.empty(n, dtype=torch.float32, device=dev), "geometry_ids": torch.empty(n, dtype=torch.int32, device=dev),
                "primitive_ids": torch.empty(n, dtype=torch.int32, device=dev), "primitive_uvs": torch.empty((n, 2), dtype=torch.float32, device=dev)}

    def cast_rays(self, rays):
        """rays (..., 6) float32 [origin, direction] -> dict with open3d's keys (no normals), shaped like rays.shape[:-1]."""
        L.require_cuda(rays)                                   # before the scene is built for them
        assert rays.shape[-1] == 6
        nodes, leaves, T, status = self._build()
        flat = rays.detach().to(torch.float32).reshape(-1, 6).contiguous()
        n = flat.shape[0]
        ans = self._answer(n, flat.device)
        call("sv_cast_rays", L.ptr(nodes), L.ptr(leaves), T, L.ptr(flat), n, L.ptr(ans["t_hit"]), L.ptr(ans["geometry_ids"]), L.ptr(ans["primitive_ids"]),
             L.ptr(ans["primitive_uvs"]), L.ptr(status))
        L.flush_checks()                                        # a read only after a rebuild: the refusal of a scene that is not finite
        shape = tuple(rays.shape[:-1])
        return {k: v.reshape(shape + tuple(v.shape[1:])) for k, v in ans.items()}

    def cast_pinhole(self, cams, width_px, height_px):
        """cams (C, 12) float64 on the device -> the answer of cast_rays for the C * H * W rays of all cameras, flat, from one launch and without a
        ray tensor.  No host read: the caller's own read carries the scene's check."""
        L.require_cuda(cams)
        nodes, leaves, T, status = self._build()
        C = cams.shape[0]
        ans = self._answer(C * width_px * height_px, cams.device)
        call("sv_cast_pinhole", L.ptr(nodes), L.ptr(leaves), T, L.ptr(cams), C, int(width_px), int(height_px), L.ptr(ans["t_hit"]), L.ptr(ans["geometry_ids"]),
             L.ptr(ans["primitive_ids"]), L.ptr(ans["primitive_uvs"]), L.ptr(status))
        return ans

    @property
    def status(self):
        """(2,) int32 on the device: [a vertex is not finite, the traversal stack was full]; both stay 0."""
        return self._build()[3]

    @staticmethod
    def create_rays_pinhole(fov_deg, center, eye, up, width_px, height_px, device=None):
        """(height_px, width_px, 6) float32 on the device; open3d's argument names."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.SeevcnHipError("seevcn_amd ops run on the GPU only; there is no CPU fallback")
        cams = cameras_to_device(pinhole_camera(fov_deg, center, eye, up, width_px, height_px), dev)
        return rays_pinhole(cams, width_px, height_px)[0]
