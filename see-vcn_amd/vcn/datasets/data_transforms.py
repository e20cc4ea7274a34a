"""The VC training transforms (reference: see/surface_completion/models/vcn/datasets/data_transforms.py).

`ResamplePoints` is the reference's host class as it is.  Everything below it runs a whole batch of objects on the device (csrc/lidar_sim.hip):
the clouds stay stacked in one (sum N, 3) fp32 buffer, the kernels compute ring indices, copy rows and apply point-wise arithmetic, and every random
draw is made on the host, per sample, in the reference's order.  The ring transforms' draws depend on the data through n, the number of rings and
the points per ring only, so they cost one host read of that integer table for the whole batch (`plan_lidar_simulation`, `plan_downsample_rings`).
"""
import numpy as np
import torch

from ... import _lib as L
from ... import data_pipeline as P
from ..utils.transform import rotate_points_along_z


class ResamplePoints(object):
    """Drop or duplicate points so that a cloud has exactly n points: tile up, then keep the first n of a random
    permutation drawn from numpy's global RNG (same contract and RNG consumption as the reference,
    see/surface_completion/models/vcn/datasets/data_transforms.py:247-262)."""

    def __init__(self, parameters):
        self.n_points = parameters['n_points']

    def __call__(self, pts):
        tiled = np.tile(pts, (int(np.ceil(self.n_points / len(pts))), 1))
        choice = np.random.permutation(tiled.shape[0])
        return tiled[choice[:self.n_points]]


# library calls and blocking device -> host reads since the last reset_counters(); neither depends on the batch size
_counted = P.Counted()
COUNTERS, reset_counters, call, read = _counted.counters, _counted.reset, _counted.call, _counted.read

MAX_RINGS = 1024                      # SV_VC_MAX_RINGS
MAX_OBJECT_POINTS = 1 << 20           # bins = 'sqrt' gives at most MAX_RINGS bins up to here
PLAN_WORDS = 40                       # SV_VC_PLAN_WORDS


# ---------------------------------------------------------------------------------------------------------------- planners
def _passthrough(n, exit_name):
    return {"pass": True, "rings": None, "first": 0, "step": 1, "exit": exit_name}, int(n)


def _selection(rings, first, step, total, exit_name):
    """sph_pts[in1d(ring_indices, rings)][first::step]: `total` rows carry one of `rings`."""
    return ({"pass": False, "rings": np.unique(np.asarray(rings, np.int64)), "first": int(first), "step": int(step), "exit": exit_name},
            len(range(int(first), int(total), int(step))))


def plan_lidar_simulation(rng, n, num_rings, ring_cnt, min_in_pts=100, min_out_pts=30, max_sel_n_hpts_1_2_ring=30):
    """LidarSimulation.__call__ (data_transforms.py:156-201) on the integer table: n points, num_rings rings, ring_cnt[r - 1] points in ring r.
    The same rng calls in the same order.  Returns (plan, output length); plan["exit"] names the return statement taken: "small" (:159), "out"
    (:198), "onetwo" (:194), "onetwo_fallback" (:191) or "original" (:201)."""
    if n < min_in_pts:
        return _passthrough(n, "small")
    ring_cnt = np.asarray(ring_cnt, np.int64)[:num_rings]
    unique_rings = np.arange(1, num_rings + 1)                                  # np.unique(ring_indices)
    sel_n_ring = rng.randint(1, max(np.ceil(num_rings * 0.3), 2))
    choose_rings = unique_rings[rng.randint(0, max(np.ceil(num_rings * 0.1), 1))::sel_n_ring]
    onetwo_ring = rng.choice([False, True], replace=False, p=[0.8, 0.2])
    if onetwo_ring and len(choose_rings) > 2:
        onetwo_ring_idxs = rng.choice(choose_rings, size=rng.randint(1, 3))
    counts = ring_cnt[choose_rings - 1]                                         # np.unique(ring_indices[mask], return_counts=True)
    sel_n_hpts = rng.randint(1, max(np.ceil(min(counts) * 0.5), 2))
    out = _selection(choose_rings, rng.randint(0, min(counts)), sel_n_hpts, counts.sum(), "out")
    if onetwo_ring and len(choose_rings) > 2:
        sel_n_hpts = min(max_sel_n_hpts_1_2_ring, sel_n_hpts)
        onetwo = _selection(onetwo_ring_idxs, rng.randint(0, min(counts)), sel_n_hpts, ring_cnt[np.unique(onetwo_ring_idxs) - 1].sum(), "onetwo")
        if onetwo[1] < min_out_pts:
            out[0]["exit"] = "onetwo_fallback"
            return out
        return onetwo
    if out[1] > min_out_pts:
        return out
    return _passthrough(n, "original")


def plan_downsample_rings(rng, n, num_rings, ring_cnt, min_in_pts=50, min_out_pts=30):
    """DownsampleRings.__call__ (data_transforms.py:122-140) on the integer table of the 50-bin histogram.  Exits "small" (:125), "out" (:138) and
    "original" (:140); rng.randint(1, 1) raises the reference's ValueError when an enabled cloud has one ring."""
    if n < min_in_pts:
        return _passthrough(n, "small")
    enable = rng.choice([False, True], replace=False, p=[0.5, 0.5])
    if enable:
        ring_cnt = np.asarray(ring_cnt, np.int64)[:num_rings]
        choose_rings = np.arange(1, num_rings + 1)[rng.randint(0, 3)::rng.randint(1, num_rings)]
        total = ring_cnt[choose_rings - 1].sum()
        if total > min_out_pts:
            return _selection(choose_rings, 0, 1, total, "out")
    return _passthrough(n, "original")


# ---------------------------------------------------------------------------------------------------------------- draws
def draw_point_dropout(rng, n, point_dropout, min_pts=30):
    """RandomPointDropout.__call__ (:58-73): the keep mask (n,) bool, or None for a cloud below min_pts (no draw)."""
    if n < min_pts:
        return None
    if rng.choice([False, True], replace=False, p=[0.5, 0.5]):
        return rng.choice(a=[False, True], size=n, p=[point_dropout, 1 - point_dropout])
    return rng.choice(a=[True], size=n)


def draw_jitter(rng, n, sigma, clip):
    """Jitter.__call__ (:214-217): the clipped noise (n, 3)."""
    return np.clip(sigma * rng.randn(n, 3), -1 * clip, clip)


def draw_gn_spherical(rng, n, stdev_bounds=(0.005, 0.03)):
    """AddGNSpherical.__call__ (:232-245): the range noise (n,), or None when the transform is not enabled."""
    enable = rng.choice([False, True], replace=False, p=[0.2, 0.8])
    if not enable:
        return None
    noise_stdev = rng.uniform(stdev_bounds[0], stdev_bounds[1])
    noise = rng.normal(0, noise_stdev, n)
    mask = rng.choice([True, False], size=n, p=[0.5, 0.5])
    noise[mask] = 0.0
    return noise


def draw_resample(rng, n, n_points):
    """ResamplePoints.__call__ (:254-262): the first n_points of the permutation of the tiled cloud; row i of the tiled cloud is row i % n."""
    return rng.permutation(n * int(np.ceil(n_points / n)))[:n_points]


def draw_world_flip(rng, along_axis):
    """RandomWorldFlip.__call__ (:268-285): ("flip_x" | "flip_y" | None, enable)."""
    if 'X' in along_axis:
        return "flip_x", bool(rng.choice([False, True], replace=False, p=[0.5, 0.5]))
    if 'Y' in along_axis:
        return "flip_y", bool(rng.choice([False, True], replace=False, p=[0.5, 0.5]))
    return None, False


def draw_object_scaling(rng, scale_range):
    """RandomObjectScaling.__call__ (:299-309): the three factors, or None (range narrower than 1e-3: no draw; not enabled: one draw)."""
    if scale_range[1] - scale_range[0] < 1e-3:
        return None
    if rng.choice([False, True], replace=False, p=[0.5, 0.5]):
        return rng.uniform(scale_range[0], scale_range[1], 3)
    return None


def draw_global_scaling(rng, scale_range):
    """GlobalScaling.__call__ (:332-334): the factor, or None for a range narrower than 1e-3."""
    if scale_range[1] - scale_range[0] < 1e-3:
        return None
    return rng.uniform(scale_range[0], scale_range[1])


def draw_global_rotation(rng, rot_range):
    """GlobalRotation.__call__ (:353)."""
    return rng.uniform(rot_range[0], rot_range[1])


# ---------------------------------------------------------------------------------------------------------------- device layer
class StackedClouds:
    """B clouds in one (sum N, 3) fp32 device buffer; counts on the host, start / cnt (B,) int32 on the device (one upload)."""

    def __init__(self, points, counts):
        L.require_cuda(points)
        counts = np.asarray(counts, np.int64).reshape(-1)
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("stacked clouds are (sum N, 3) float32")
        if len(counts) < 1 or int(counts.sum()) != points.shape[0]:
            raise ValueError("counts do not add up to the number of rows")
        if counts.min() < 1:
            raise ValueError("an object has no points")
        if counts.max() > MAX_OBJECT_POINTS:
            raise ValueError(f"at most 2^20 points per object, got {int(counts.max())}")
        self.points, self.counts = points.contiguous(), counts
        self.starts = np.cumsum(counts) - counts
        meta = torch.from_numpy(np.concatenate([self.starts, counts]).astype(np.int32)).to(points.device)
        self.start, self.cnt = meta[:len(counts)], meta[len(counts):]

    @property
    def batch_size(self):
        return len(self.counts)

    def args(self):
        return L.ptr(self.points), L.ptr(self.start), L.ptr(self.cnt), self.batch_size


def vc_rings(clouds, fixed_bins=0, min_in_pts=0, with_elevation=False):
    """sv_vc_rings: ring (sum N,) int32 and the table (B, 1 + MAX_RINGS) int32 on the device, [num_rings, points per ring]; the float64 elevations on
    request.  fixed_bins = 0: bins = 'sqrt'."""
    dev, B = clouds.points.device, clouds.batch_size
    ring = torch.empty(clouds.points.shape[0], dtype=torch.int32, device=dev)
    table = torch.empty(B * (1 + MAX_RINGS), dtype=torch.int32, device=dev)
    elev = torch.empty(clouds.points.shape[0], dtype=torch.float64, device=dev) if with_elevation else None
    call("sv_vc_rings", *clouds.args(), int(fixed_bins), int(min_in_pts), L.ptr(ring), L.ptr(table[:B]), L.ptr(table[B:]), L.ptr(elev))
    return ring, table, elev


def read_ring_table(table, B):
    """The one host read of a ring transform: num_rings (B,) and ring_cnt (B, MAX_RINGS)."""
    host = read(table)
    return host[:B].astype(np.int64), host[B:].reshape(B, MAX_RINGS).astype(np.int64)


def pack_plans(plans, lengths, keep_used=None):
    """The host table of sv_vc_select: one row of PLAN_WORDS int32 per object, output offsets = the running sum of the lengths."""
    B = len(plans)
    table = np.zeros((B, PLAN_WORDS), np.int64)
    lengths = np.asarray(lengths, np.int64)
    table[:, 5], table[:, 6] = np.cumsum(lengths) - lengths, lengths
    for b, p in enumerate(plans):
        if p["step"] < 1 or p["first"] < 0:
            raise ValueError("a selection needs first >= 0 and step >= 1")
        table[b, 0], table[b, 3], table[b, 4] = int(p["pass"]), p["first"], p["step"]
        table[b, 2] = int(bool(keep_used is not None and keep_used[b]))
        if p["rings"] is not None:
            table[b, 1] = 1
            r = np.asarray(p["rings"], np.int64) - 1
            if len(r) and (r.min() < 0 or r.max() >= MAX_RINGS):
                raise ValueError("ring index out of range")
            np.bitwise_or.at(table[b], 8 + (r >> 5), np.int64(1) << (r & 31))
    return (table & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def vc_select(clouds, plans, lengths, ring=None, keep=None, keep_used=None):
    """sv_vc_select: the selected rows of every object as new StackedClouds."""
    dev = clouds.points.device
    lengths = np.asarray(lengths, np.int64)
    if lengths.min() < 1:
        raise ValueError("an object has no points")
    table = torch.from_numpy(pack_plans(plans, lengths, keep_used)).to(dev)
    out = torch.empty(int(lengths.sum()), 3, dtype=torch.float32, device=dev)
    call("sv_vc_select", *clouds.args(), L.ptr(ring), L.ptr(keep), L.ptr(table), L.ptr(out))
    return StackedClouds(out, lengths)


def vc_resample(clouds, index):
    """sv_vc_resample: index (B, n_points) host integers -> (B, n_points, 3)."""
    dev = clouds.points.device
    index = np.ascontiguousarray(index, np.int32)
    B, n_points = index.shape
    out = torch.empty(B, n_points, 3, dtype=torch.float32, device=dev)
    call("sv_vc_resample", *clouds.args(), L.ptr(torch.from_numpy(index).to(dev)), n_points, L.ptr(out))
    return out


def vc_pointwise(clouds, noise, mode):
    """sv_vc_pointwise in place: mode 0 Jitter (noise (sum N, 3)), mode 1 AddGNSpherical (noise (sum N,)); host float64 noise."""
    noise = np.ascontiguousarray(noise, np.float64)
    assert noise.size == clouds.points.shape[0] * (3 if mode == 0 else 1)
    dev_noise = torch.from_numpy(noise).to(clouds.points.device)
    call("sv_vc_pointwise", L.ptr(clouds.points), int(clouds.points.shape[0]), L.ptr(dev_noise), int(mode))


def vc_world_transform(clouds, op, params):
    """One op of sv_world_transform_points (flip_x, flip_y, rotation, scaling) with one float64 parameter per object, in place."""
    code = P.pack_codes([op], "world")
    p = torch.from_numpy(np.ascontiguousarray(params, np.float64).reshape(clouds.batch_size, 1)).to(clouds.points.device)
    call("sv_world_transform_points", L.ptr(clouds.points), 3, L.ptr(clouds.start), L.ptr(clouds.cnt), clouds.batch_size, int(clouds.counts.max()), code, 1,
         L.ptr(p))


def vc_object_scale(clouds, params):
    """sv_vc_object_scale in place: params (B, 8) host float64 = enable, centre, heading, scale."""
    p = torch.from_numpy(np.ascontiguousarray(params, np.float64).reshape(clouds.batch_size, 8)).to(clouds.points.device)
    call("sv_vc_object_scale", L.ptr(clouds.points), L.ptr(clouds.start), L.ptr(clouds.cnt), clouds.batch_size, int(clouds.counts.max()), L.ptr(p))


# ---------------------------------------------------------------------------------------------------------------- batch transforms
# A cloud transform takes (clouds, rngs) and returns the new StackedClouds; a data transform takes the whole batch dict.
class LidarSimulation(object):
    """data_transforms.py:142-201: 2 library calls and 1 host read for the batch."""

    def __init__(self, parameters):
        pass

    def __call__(self, clouds, rngs, min_in_pts=100, min_out_pts=30, max_sel_n_hpts_1_2_ring=30):
        ring, table, _ = vc_rings(clouds, 0, min_in_pts)
        num_rings, ring_cnt = read_ring_table(table, clouds.batch_size)
        plans = [plan_lidar_simulation(rng, int(n), int(r), c, min_in_pts, min_out_pts, max_sel_n_hpts_1_2_ring)
                 for rng, n, r, c in zip(rngs, clouds.counts, num_rings, ring_cnt)]
        self.exits = [p["exit"] for p, _ in plans]
        return vc_select(clouds, [p for p, _ in plans], [m for _, m in plans], ring=ring)


class DownsampleRings(object):
    """data_transforms.py:113-140."""

    def __init__(self, parameters):
        pass

    def __call__(self, clouds, rngs, min_in_pts=50, min_out_pts=30):
        ring, table, _ = vc_rings(clouds, 50, min_in_pts)
        num_rings, ring_cnt = read_ring_table(table, clouds.batch_size)
        plans = [plan_downsample_rings(rng, int(n), int(r), c, min_in_pts, min_out_pts) for rng, n, r, c in zip(rngs, clouds.counts, num_rings, ring_cnt)]
        self.exits = [p["exit"] for p, _ in plans]
        return vc_select(clouds, [p for p, _ in plans], [m for _, m in plans], ring=ring)


class RandomPointDropout(object):
    """data_transforms.py:46-73: the masks are drawn on the host, so the lengths are known without a read."""

    def __init__(self, parameters):
        self.point_dropout = parameters['point_dropout']

    def __call__(self, clouds, rngs, min_pts=30):
        masks = [draw_point_dropout(rng, int(n), self.point_dropout, min_pts) for rng, n in zip(rngs, clouds.counts)]
        keep = np.concatenate([np.ones(int(n), np.uint8) if m is None else m.astype(np.uint8) for m, n in zip(masks, clouds.counts)])
        plans = [_passthrough(n, "small")[0] if m is None else {"pass": False, "rings": None, "first": 0, "step": 1, "exit": "out"} for m, n in zip(masks, clouds.counts)]
        lengths = [int(n) if m is None else int(m.sum()) for m, n in zip(masks, clouds.counts)]
        return vc_select(clouds, plans, lengths, keep=torch.from_numpy(keep).to(clouds.points.device), keep_used=[m is not None for m in masks])


class Jitter(object):
    """data_transforms.py:203-217."""

    def __init__(self, parameters):
        self.clip = parameters['clip'] if parameters['clip'] is not None else 0.05
        self.sigma = parameters['sigma'] if parameters['sigma'] is not None else 0.01

    def __call__(self, clouds, rngs):
        vc_pointwise(clouds, np.concatenate([draw_jitter(rng, int(n), self.sigma, self.clip) for rng, n in zip(rngs, clouds.counts)]), 0)
        return clouds


class AddGNSpherical(object):
    """data_transforms.py:219-245.  A cloud that is not enabled gets zero noise, which leaves its rows as they are."""

    def __init__(self, parameters):
        self.stdev_bounds = [0.005, 0.03]

    def __call__(self, clouds, rngs):
        noise = [draw_gn_spherical(rng, int(n), self.stdev_bounds) for rng, n in zip(rngs, clouds.counts)]
        vc_pointwise(clouds, np.concatenate([np.zeros(int(n)) if z is None else z for z, n in zip(noise, clouds.counts)]), 1)
        return clouds


class BatchResamplePoints(object):
    """ResamplePoints (data_transforms.py:247-262) for the batch: (B, n_points, 3), kept as stacked clouds of n_points rows each."""

    def __init__(self, parameters):
        self.n_points = parameters['n_points']

    def __call__(self, clouds, rngs):
        index = np.stack([draw_resample(rng, int(n), self.n_points) for rng, n in zip(rngs, clouds.counts)])
        out = vc_resample(clouds, index)
        return StackedClouds(out.view(-1, 3), np.full(clouds.batch_size, self.n_points))


def _both(batch):
    return [batch[k] for k in ("partial", "complete") if batch.get(k) is not None]


class RandomWorldFlip(object):
    """data_transforms.py:264-285."""

    def __init__(self, parameters):
        self.along_axis = parameters['along_axis']

    def __call__(self, batch, rngs):
        draws = [draw_world_flip(rng, self.along_axis) for rng in rngs]
        op, gtbox = draws[0][0], batch["gtbox"]
        if op is None:
            return batch
        enable = np.array([e for _, e in draws])
        for b in np.nonzero(enable)[0]:
            if op == "flip_x":
                gtbox[b, 1], gtbox[b, 6] = -gtbox[b, 1], -gtbox[b, 6]
            else:
                gtbox[b, 0], gtbox[b, 6] = -gtbox[b, 0], -(gtbox[b, 6] + np.pi)
        for clouds in _both(batch):
            vc_world_transform(clouds, op, enable.astype(np.float64))
        return batch


class RandomObjectScaling(object):
    """data_transforms.py:287-318."""

    def __init__(self, parameters):
        self.scale_range = parameters['scale_range']

    def __call__(self, batch, rngs):
        scales = [draw_object_scaling(rng, self.scale_range) for rng in rngs]
        if self.scale_range[1] - self.scale_range[0] < 1e-3:
            return batch
        gtbox, params = batch["gtbox"], np.zeros((len(rngs), 8))
        for b, s in enumerate(scales):
            if s is not None:
                params[b] = [1.0, *gtbox[b, :3], gtbox[b, 6], *s]
                gtbox[b, 3:6] *= s
        for clouds in _both(batch):
            vc_object_scale(clouds, params)
        return batch


class GlobalScaling(object):
    """data_transforms.py:320-339 (fp32 products on the device)."""

    def __init__(self, parameters):
        self.scale_range = parameters['scale_range']

    def __call__(self, batch, rngs):
        scales = [draw_global_scaling(rng, self.scale_range) for rng in rngs]
        if scales[0] is None:
            return batch
        batch["gtbox"][:, :6] *= np.asarray(scales)[:, None]
        for clouds in _both(batch):
            vc_world_transform(clouds, "scaling", scales)
        return batch


class GlobalRotation(object):
    """data_transforms.py:341-359: the fp32 rotation of utils/transform.py:33-58 for the points (device) and the box centre (host, the same torch ops)."""

    def __init__(self, parameters):
        self.rot_range = parameters['rot_range']

    def __call__(self, batch, rngs):
        angles = np.array([draw_global_rotation(rng, self.rot_range) for rng in rngs])
        gtbox = batch["gtbox"]
        for b, angle in enumerate(angles):                          # one sample at a time, the shapes the reference's matmul sees
            centre = rotate_points_along_z(torch.from_numpy(gtbox[b:b + 1, None, 0:3].copy()).float(), torch.from_numpy(angles[b:b + 1]).float())
            gtbox[b, 0:3] = centre[0, 0].numpy()
            gtbox[b, 6] += angle
        for clouds in _both(batch):
            vc_world_transform(clouds, "rotation", angles)
        return batch


_CLOUD_TRANSFORMS = {"LidarSimulation": LidarSimulation, "DownsampleRings": DownsampleRings, "RandomPointDropout": RandomPointDropout,
                     "Jitter": Jitter, "AddGNSpherical": AddGNSpherical, "ResamplePoints": BatchResamplePoints}
# the reference's Compose hands the whole sample to RandomWorldFlip, GlobalRotation and RandomObjectScaling; GlobalScaling takes the sample too
_DATA_TRANSFORMS = {"RandomWorldFlip": RandomWorldFlip, "GlobalRotation": GlobalRotation, "RandomObjectScaling": RandomObjectScaling,
                    "GlobalScaling": GlobalScaling}
NOT_BUILT = ("PeriodicSampling", "RandomSamplePoints", "RandomMirrorPoints", "NormalizeObjectPose", "ToTensor")


class BatchCompose(object):
    """The reference's Compose (data_transforms.py:8-37) for a batch on the device, from the same list of dicts.

    forward(batch, rngs): batch = {"partial": (sum N, 3) fp32 device tensor, "partial_cnt": (B,) host counts, "complete" / "complete_cnt" the same
    or absent, "gtbox": (B, 7) host float64}; rngs: one np.random.RandomState per sample.  The queue runs stage by stage over the whole batch; each
    sample's stream is consumed as Compose under np.random.seed consumes the global one: `rnd_value` first, then the transform's own draws (for the
    listed objects in the order partial, complete).  Returns {"partial": (B, n_points, 3) when the queue's last step on it is ResamplePoints, else
    the stacked rows, "partial_cnt", "complete", "complete_cnt", "gtbox"}."""

    def __init__(self, transform_list):
        self.transformers = []
        for tr in transform_list:
            name = tr['callback']
            if name in NOT_BUILT or (name not in _CLOUD_TRANSFORMS and name not in _DATA_TRANSFORMS):
                raise NotImplementedError(f"{name} is not built on the device (DESIGN.md section 7)")
            parameters = tr['parameters'] if 'parameters' in tr else None
            cls = _CLOUD_TRANSFORMS.get(name) or _DATA_TRANSFORMS[name]
            self.transformers.append({'callback': cls(parameters), 'objects': tr['objects'], 'data': name in _DATA_TRANSFORMS})

    def forward(self, batch, rngs):
        gtbox = batch.get("gtbox")
        data = {"partial": StackedClouds(batch["partial"], batch["partial_cnt"]),
                "complete": None if batch.get("complete") is None else StackedClouds(batch["complete"], batch["complete_cnt"]),
                "gtbox": None if gtbox is None else np.array(gtbox, np.float64)}
        B = data["partial"].batch_size
        if len(rngs) != B or (data["complete"] is not None and data["complete"].batch_size != B):
            raise ValueError("one RandomState per sample, and as many complete clouds as partial ones")
        dense = {"partial": None, "complete": None}
        for tr in self.transformers:
            for rng in rngs:
                rng.uniform(0, 1)                                   # Compose's rnd_value
            if tr['data']:
                data = tr['callback'](data, rngs)
                dense = {"partial": None, "complete": None}
                continue
            for k in ("partial", "complete"):
                if k in tr['objects'] and data[k] is not None:
                    data[k] = tr['callback'](data[k], rngs)
                    dense[k] = tr['callback'].n_points if isinstance(tr['callback'], BatchResamplePoints) else None
        out = {"gtbox": data["gtbox"]}
        for k in ("partial", "complete"):
            c = data[k]
            out[k] = None if c is None else (c.points.view(B, dense[k], 3) if dense[k] else c.points)
            out[k + "_cnt"] = None if c is None else c.counts
        return out

    __call__ = forward
