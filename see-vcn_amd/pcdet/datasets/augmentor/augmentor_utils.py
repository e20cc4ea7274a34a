"""Training augmentation on the device (reference: datasets/augmentor/augmentor_utils.py, numpy on dataloader workers) on csrc/augment.hip,
csrc/augment_local.hip and csrc/augment_pyramid.hip.

The functions keep the reference's names and take a `DeviceBatch` -- every scene of the batch in one stacked point buffer and one stacked box
buffer -- plus the random draws, which the caller makes on the host in the reference's order (data_augmentor.draw_params).  Points are never
removed between stages: a dropped point gets keep = 0 and `compact` removes it at the very end, which preserves order and so gives the same
result as the reference's compaction after every stage.
"""
import ctypes

import numpy as np
import torch

from .... import _lib as L
from .... import data_pipeline as P

# library calls and blocking device -> host reads since the last reset_counters(); neither depends on the batch size or the number of boxes
_counted = P.Counted()
COUNTERS, reset_counters, call, read = _counted.counters, _counted.reset, _counted.call, _counted.read

MAX_BOXES_PER_SCENE = 256
MAX_NUM_TRY = 64
OPS, LOCAL_STEPS, WORLD_DROPOUT = P.codes_of("world"), P.codes_of("local"), P.codes_of("drop")   # views of data_pipeline.OP_CODES


class DeviceBatch:
    """The scenes of one batch, stacked.  points (P, C) fp32 and keep (P,) int32; boxes (N, W) fp32 and box_cls (N,) int32 (>= 0 index into
    class_names, -1 another class, -2 filtered out); pt_start / pt_cnt / box_start / box_cnt (B,) int32 on the device.  max_scene_points and
    max_scene_boxes are host upper bounds.  With point_slots / box_slots (GT sampling) scene b's point rows begin with point_slots[b] spare rows
    (keep = 0 until an object is pasted there) and its box rows end with box_slots[b] spare rows (box_cls = -2, beyond box_cnt).  add_room
    re-stacks the points with spare rows behind each scene's (the pyramid augmentor's appended rows).  check: None, or one int32 on the device
    that kernels raise on a broken plan; it is read with the next host read (compact's at the latest) and a non-zero value is an error."""

    def __init__(self, points, boxes, box_cls, pt_sizes, box_sizes, box_slots=None, point_slots=None):
        L.require_cuda(points, boxes)
        assert points.dtype == boxes.dtype == torch.float32 and points.dim() == boxes.dim() == 2
        assert points.shape[1] >= 3 and boxes.shape[1] >= 7
        pt_sizes, box_rows = np.asarray(pt_sizes, np.int64), np.asarray(box_sizes, np.int64)
        B = len(pt_sizes)
        box_slots = np.zeros(B, np.int64) if box_slots is None else np.asarray(box_slots, np.int64)
        self.point_slots = np.zeros(B, np.int64) if point_slots is None else np.asarray(point_slots, np.int64)
        box_cls = np.asarray(box_cls, np.int32).reshape(-1)
        assert len(box_rows) == B >= 1 and pt_sizes.sum() == points.shape[0] and box_rows.sum() == boxes.shape[0] == len(box_cls)
        if box_rows.max() > MAX_BOXES_PER_SCENE:
            raise ValueError(f"at most {MAX_BOXES_PER_SCENE} boxes per scene (existing + candidates), got {int(box_rows.max())}")
        dev = points.device
        self.batch_size = B
        self.num_point_features, self.box_width = points.shape[1], boxes.shape[1]
        self.max_scene_points, self.max_scene_boxes = int(pt_sizes.max()), int(box_rows.max())
        self.total_points, self.total_boxes = int(points.shape[0]), int(boxes.shape[0])
        # at least one row each, so that no kernel is handed a null pointer for an empty batch
        self.points = points.contiguous() if self.total_points else torch.zeros(1, points.shape[1], device=dev)
        self.boxes = boxes.contiguous() if self.total_boxes else torch.zeros(1, boxes.shape[1], device=dev)
        self.keep = torch.ones(max(self.total_points, 1), dtype=torch.int32, device=dev)
        self.pt_offsets, self.box_offsets = np.cumsum(pt_sizes) - pt_sizes, np.cumsum(box_rows) - box_rows
        self.pt_sizes, self.check = pt_sizes, None
        self.box_sizes = box_rows - box_slots                     # the boxes that exist on entry
        host = np.concatenate([self.pt_offsets, pt_sizes, self.box_offsets, self.box_sizes, box_rows, box_cls, [-2]]).astype(np.int32)
        meta = torch.from_numpy(host).to(dev)                   # one upload for the whole layout
        self.pt_start, self.pt_cnt, self.box_start, self.box_cnt = meta[:B], meta[B:2 * B], meta[2 * B:3 * B], meta[3 * B:4 * B]
        self.box_cap, self.box_cls = meta[4 * B:5 * B], meta[5 * B:]   # rows a scene owns (existing + spare), class codes

    @classmethod
    def from_scenes(cls, points_list, boxes_list, cls_list, point_slots=None, box_slots=None):
        """points_list[b] (n_b, C), boxes_list[b] (m_b, W) device tensors; cls_list[b] (m_b,) host integers."""
        B = len(points_list)
        pts, boxes, codes = list(points_list), list(boxes_list), [np.asarray(c, np.int32).reshape(-1) for c in cls_list]
        if point_slots is None and box_slots is None:
            return cls(torch.cat(pts), torch.cat(boxes), np.concatenate(codes), [len(p) for p in pts], [len(b) for b in boxes])
        point_slots, box_slots = [int(v) for v in point_slots], [int(v) for v in box_slots]
        dev, C, W = pts[0].device, pts[0].shape[1], boxes[0].shape[1]
        spare_p = torch.zeros(max(point_slots), C, device=dev)     # one block of zeros, sliced per scene
        spare_b = torch.zeros(max(box_slots), W, device=dev)
        inst = cls(torch.cat([t for b in range(B) for t in (spare_p[:point_slots[b]], pts[b])]),
                   torch.cat([t for b in range(B) for t in (boxes[b], spare_b[:box_slots[b]])]),
                   np.concatenate([np.concatenate([codes[b], np.full(box_slots[b], -2, np.int32)]) for b in range(B)]),
                   [len(p) + s for p, s in zip(pts, point_slots)], [len(b) + s for b, s in zip(boxes, box_slots)], box_slots, point_slots)
        flags = torch.ones(2, max(max(point_slots), max(len(p) for p in pts), 1), dtype=torch.int32, device=dev)
        flags[0] = 0
        inst.keep = torch.cat([t for b in range(B) for t in (flags[0, :point_slots[b]], flags[1, :len(pts[b])])] + [flags[1, :1]])
        return inst

    def add_room(self, extra):
        """Re-stack the points with extra[b] spare rows (zeros, keep = 0) behind scene b's rows; pt_cnt then includes them and max_scene_points
        follows.  The spare rows in front (point_slots) stay where they are.  Returns the first spare row of every scene (host, global rows)."""
        extra = np.asarray(extra, np.int64).reshape(-1)
        assert len(extra) == self.batch_size and (extra >= 0).all()
        if extra.sum() == 0:
            return self.pt_offsets + self.pt_sizes
        dev, B = self.points.device, self.batch_size
        spare_p = torch.zeros(int(extra.max()), self.num_point_features, device=dev)
        spare_k = torch.zeros(int(extra.max()), dtype=torch.int32, device=dev)
        ends = self.pt_offsets + self.pt_sizes
        self.points = torch.cat([t for b in range(B) for t in (self.points[self.pt_offsets[b]:ends[b]], spare_p[:extra[b]])])
        self.keep = torch.cat([t for b in range(B) for t in (self.keep[self.pt_offsets[b]:ends[b]], spare_k[:extra[b]])])
        first = np.cumsum(self.pt_sizes + extra) - extra
        self.pt_sizes = self.pt_sizes + extra
        self.pt_offsets = np.cumsum(self.pt_sizes) - self.pt_sizes
        self.max_scene_points, self.total_points = int(self.pt_sizes.max()), int(self.pt_sizes.sum())
        meta = torch.from_numpy(np.concatenate([self.pt_offsets, self.pt_sizes]).astype(np.int32)).to(dev)
        self.pt_start, self.pt_cnt = meta[:B], meta[B:]
        return first

    def _pt_args(self):
        return L.ptr(self.points), self.num_point_features, L.ptr(self.pt_start), L.ptr(self.pt_cnt)

    def _box_args(self):
        return L.ptr(self.boxes), self.box_width, L.ptr(self.box_start), L.ptr(self.box_cnt)


def _device_f64(values, device):
    if isinstance(values, torch.Tensor):
        assert values.dtype == torch.float64 and values.is_cuda
        return values.contiguous()
    return torch.from_numpy(np.ascontiguousarray(values, np.float64)).to(device)


def points_in_boxes_count(batch):
    """(N,) int32: the points of its scene inside each box by the CPU matrix test, margin 1e-2 in x / y and none in z (dataset.py:131-133)."""
    counts = torch.empty(max(batch.total_boxes, 1), dtype=torch.int32, device=batch.points.device)
    call("sv_points_in_boxes_count", *batch._pt_args(), L.ptr(batch.keep), batch.batch_size, batch.max_scene_points, *batch._box_args(), batch.total_boxes,
         L.ptr(counts))
    return counts[:batch.total_boxes]


def filter_boxes_by_min_points(batch, min_points, counts=None):
    """MIN_POINTS_OF_GT (dataset.py:135-137) without a host read: boxes below the limit stop existing (box_cls = -2)."""
    counts = points_in_boxes_count(batch) if counts is None else counts
    cls = batch.box_cls[:batch.total_boxes]
    cls.copy_(torch.where(counts >= int(min_points), cls, torch.full_like(cls, -2)))
    return counts


def scale_pre_object(batch, scale_noises):
    """augmentor_utils.py:10-80 for every scene of the batch.  scale_noises (N, num_try) fp64: row i holds the tries of box row i (rows of boxes
    that are skipped are not read).  Returns the plan (N,) fp64 on the device: the chosen scale per box, 0 = none."""
    dev = batch.points.device
    noises = _device_f64(scale_noises, dev)
    if batch.total_boxes == 0:
        return torch.zeros(0, dtype=torch.float64, device=dev)
    assert noises.dim() == 2 and noises.shape[0] == batch.total_boxes
    num_try = int(noises.shape[1])
    if not 1 <= num_try <= MAX_NUM_TRY:
        raise ValueError(f"num_try must be in 1..{MAX_NUM_TRY}, got {num_try}")
    before = batch.boxes.clone()
    plan = torch.empty(batch.total_boxes, dtype=torch.float64, device=dev)
    call("sv_object_scale_plan", *batch._box_args(), L.ptr(batch.box_cls), batch.batch_size, L.ptr(noises), num_try, L.ptr(plan))
    call("sv_object_scale_points", *batch._pt_args(), L.ptr(batch.keep), batch.batch_size, batch.max_scene_points, L.ptr(before), batch.box_width,
         L.ptr(batch.box_start), L.ptr(batch.box_cnt), L.ptr(batch.box_cls), L.ptr(plan))
    return plan


def world_transform(batch, ops, params, limit_heading=False):
    """`ops`: names from OPS in the order they apply; params (B, len(ops)) fp64, one value per scene and op.  One launch over the points and one over
    the boxes, whatever the number of ops; limit_heading adds limit_period(heading, 0.5, 2 pi) (data_augmentor.py:258-260)."""
    if len(ops) > 16:
        raise ValueError("at most 16 world transforms in one call")
    code = P.pack_codes(ops, "world")
    dev = batch.points.device
    p = _device_f64(np.zeros((batch.batch_size, 1)) if len(ops) == 0 else params, dev)
    assert len(ops) == 0 or tuple(p.shape) == (batch.batch_size, len(ops))
    if len(ops):
        call("sv_world_transform_points", *batch._pt_args(), batch.batch_size, batch.max_scene_points, code, len(ops), L.ptr(p))
    if len(ops) or limit_heading:
        call("sv_world_transform_boxes", *batch._box_args(), L.ptr(batch.box_cls), batch.batch_size, code, len(ops), L.ptr(p), int(limit_heading))


def _per_scene(batch, values):
    return np.asarray(values, np.float64).reshape(batch.batch_size, 1)


def random_flip_along_x(batch, enable):
    """augmentor_utils.py:82-99; enable: one bool per scene (the draw)."""
    world_transform(batch, ["flip_x"], _per_scene(batch, enable))


def random_flip_along_y(batch, enable):
    """augmentor_utils.py:102-119."""
    world_transform(batch, ["flip_y"], _per_scene(batch, enable))


def global_rotation(batch, noise_rotation):
    """augmentor_utils.py:122-142; noise_rotation: one angle per scene."""
    world_transform(batch, ["rotation"], _per_scene(batch, noise_rotation))


def global_scaling(batch, noise_scale):
    """augmentor_utils.py:145-160; noise_scale: one factor per scene (the caller skips the call when the range is narrower than 1e-3)."""
    world_transform(batch, ["scaling"], _per_scene(batch, noise_scale))


def random_translation_along_x(batch, offset):
    """augmentor_utils.py:203-219."""
    world_transform(batch, ["translation_x"], _per_scene(batch, offset))


def random_translation_along_y(batch, offset):
    """augmentor_utils.py:222-238."""
    world_transform(batch, ["translation_y"], _per_scene(batch, offset))


def random_translation_along_z(batch, offset):
    """augmentor_utils.py:241-254."""
    world_transform(batch, ["translation_z"], _per_scene(batch, offset))


# ------------------------------------------------------------------ local and frustum augmentors (csrc/augment_local.hip)
PLAN_ROW = 12


def local_transform(batch, steps, params):
    """`steps`: names from LOCAL_STEPS in the order they apply; params (N, len(steps)) fp64, one draw per box row and step (rows with box_cls == -2
    are not read).  Every run of up to 16 steps is one plan call (a thread per box) and one points call (a thread per point walks the boxes in
    order, step by step), whatever the number of boxes.  get_points_in_box (augmentor_utils.py:553-570) is the test: margin 0.1 in x / y, <=."""
    if "local_rotation" in steps and batch.box_width > 8:
        # np.hstack((gt_boxes[idx, 7:9], np.zeros((gt_boxes.shape[0], 1)))) raises ValueError for any N != 1 in the reference
        raise NotImplementedError("local_rotation on boxes wider than 8 columns (augmentor_utils.py:465-468)")
    if len(steps) == 0 or batch.total_boxes == 0:
        return
    dev, N = batch.points.device, batch.total_boxes
    p = _device_f64(params, dev)
    assert tuple(p.shape) == (N, len(steps))
    for first in range(0, len(steps), 16):
        run = steps[first:first + 16]
        code = P.pack_codes(run, "local")
        draws = p if len(run) == len(steps) else p[:, first:first + 16].contiguous()
        plan = torch.empty(len(run) * N * PLAN_ROW, dtype=torch.float32, device=dev)
        call("sv_local_transform_plan", *batch._box_args(), L.ptr(batch.box_cls), batch.batch_size, N, code, len(run), L.ptr(draws), L.ptr(plan))
        call("sv_local_transform_points", *batch._pt_args(), L.ptr(batch.keep), batch.batch_size, batch.max_scene_points, L.ptr(batch.box_start),
             L.ptr(batch.box_cnt), N, code, len(run), L.ptr(plan))


def _per_box(batch, values):
    return np.asarray(values, np.float64).reshape(batch.total_boxes, 1)


def random_local_translation_along_x(batch, offsets):
    """augmentor_utils.py:257-277; offsets: one per box row (the draws)."""
    local_transform(batch, ["local_translation_x"], _per_box(batch, offsets))


def random_local_translation_along_y(batch, offsets):
    """augmentor_utils.py:280-300."""
    local_transform(batch, ["local_translation_y"], _per_box(batch, offsets))


def random_local_translation_along_z(batch, offsets):
    """augmentor_utils.py:303-320."""
    local_transform(batch, ["local_translation_z"], _per_box(batch, offsets))


def local_rotation(batch, noise_rotation):
    """augmentor_utils.py:425-470; one angle per box row.  Boxes wider than 8 columns raise, as they do there."""
    local_transform(batch, ["local_rotation"], _per_box(batch, noise_rotation))


def local_scaling(batch, noise_scale):
    """augmentor_utils.py:391-422; one factor per box row (the caller skips the call when the range is narrower than 1e-3)."""
    local_transform(batch, ["local_scaling"], _per_box(batch, noise_scale))


def local_frustum_dropout_top(batch, intensity):
    """augmentor_utils.py:473-490; one intensity per box row."""
    local_transform(batch, ["local_dropout_top"], _per_box(batch, intensity))


def local_frustum_dropout_bottom(batch, intensity):
    """augmentor_utils.py:493-510."""
    local_transform(batch, ["local_dropout_bottom"], _per_box(batch, intensity))


def local_frustum_dropout_left(batch, intensity):
    """augmentor_utils.py:513-530 (the box's extent along world y)."""
    local_transform(batch, ["local_dropout_left"], _per_box(batch, intensity))


def local_frustum_dropout_right(batch, intensity):
    """augmentor_utils.py:533-550."""
    local_transform(batch, ["local_dropout_right"], _per_box(batch, intensity))


def world_frustum_dropout(batch, directions, intensity):
    """`directions`: names from WORLD_DROPOUT in order, each over the survivors of the last; intensity (B, len(directions)) fp64.  One library call.
    Deviations from augmentor_utils.py:323-388: a dropped box takes its class with it (box_cls = -2; the reference shortens gt_boxes and leaves
    gt_names / gt_boxes_mask at their old length), and a scene without live points passes through (np.max of an empty array raises there)."""
    if len(directions) > 16:
        raise ValueError("at most 16 directions in one call")
    if len(directions) == 0:
        return
    code = P.pack_codes(directions, "drop")
    dev, B = batch.points.device, batch.batch_size
    v = _device_f64(intensity, dev)
    assert tuple(v.shape) == (B, len(directions))
    scratch = L.workspace.scratch("world_frustum_dropout", max(int(L.load().sv_world_frustum_dropout_scratch_bytes(B, len(directions))), 4), dev)
    call("sv_world_frustum_dropout", *batch._pt_args(), L.ptr(batch.keep), B, batch.max_scene_points, *batch._box_args(), L.ptr(batch.box_cls),
         batch.total_boxes, code, len(directions), L.ptr(v), L.ptr(scratch))


def global_frustum_dropout_top(batch, intensity):
    """augmentor_utils.py:323-337; one intensity per scene."""
    world_frustum_dropout(batch, ["world_dropout_top"], _per_scene(batch, intensity))


def global_frustum_dropout_bottom(batch, intensity):
    """augmentor_utils.py:340-354."""
    world_frustum_dropout(batch, ["world_dropout_bottom"], _per_scene(batch, intensity))


def global_frustum_dropout_left(batch, intensity):
    """augmentor_utils.py:357-371."""
    world_frustum_dropout(batch, ["world_dropout_left"], _per_scene(batch, intensity))


def global_frustum_dropout_right(batch, intensity):
    """augmentor_utils.py:374-388."""
    world_frustum_dropout(batch, ["world_dropout_right"], _per_scene(batch, intensity))


# ------------------------------------------------------------------ the pyramid augmentor (csrc/augment_pyramid.hip)
# The draws of one scene, in the reference's stream order (augmentor_utils.py:617-619, :635-637, :656, :687, :699, :708); out["draws"] carries them
# under these names.  *_face / *_u hold one value per box the step looks at, sparsify_choice one index array per sparsified pyramid, swap_face and
# swap_partner one value per swapped pair (the partner as an index into the boxes the swap looks at).
PYRAMID_DRAWS = ("pyramid_drop_face", "pyramid_drop_u", "pyramid_sparsify_face", "pyramid_sparsify_u", "pyramid_sparsify_choice", "pyramid_swap_u",
                 "pyramid_swap_face", "pyramid_swap_partner")
MAX_SPARSIFY_NUM = 1024
_CHECK_BITS = ((1, "a pyramid holds another number of points than the count its draws and rows were planned with"),
               (2, "appended rows outside the scene's rows"), (4, "a plan row that names no scene, box or face"))


def _check_tensor(batch):
    if batch.check is None:
        batch.check = torch.zeros(1, dtype=torch.int32, device=batch.points.device)
    return batch.check


def read_checked(batch, t):
    """One counted host read of the int32 tensor t; the batch's check flag rides on it and a raised flag is an error."""
    if batch.check is None:
        return read(t)
    values = read(torch.cat([t.reshape(-1), batch.check]))
    if values[-1] != 0:
        raise L.SeevcnHipError("pyramid augmentor: " + "; ".join(text for bit, text in _CHECK_BITS if int(values[-1]) & bit))
    return values[:-1].reshape(t.shape)


def get_pyramids(boxes):
    """augmentor_utils.py:573-595: boxes (N, W >= 7) fp32 on the device -> (N, 6, 15) fp32, per face the apex (the centre) and the four base corners,
    as boxes_to_corners_3d makes them in float32 (cos / sin: the float64 function rounded once)."""
    assert boxes.dtype == torch.float32 and boxes.dim() == 2 and boxes.shape[1] >= 7
    boxes = boxes.contiguous()
    out = torch.empty(boxes.shape[0], 6, 15, dtype=torch.float32, device=boxes.device)
    call("sv_get_pyramids", L.ptr(boxes), int(boxes.shape[1]), int(boxes.shape[0]), L.ptr(out))
    return out


def _box_ints(batch, values):
    """One int32 per box row on the device (and one more, so that an empty batch hands no null pointer)."""
    host = np.zeros(batch.total_boxes + 1, np.int32)
    host[:batch.total_boxes] = np.asarray(values, np.int64).reshape(-1)
    return torch.from_numpy(host).to(batch.points.device)


def points_in_pyramids_mask(batch, face_mask=None, member=False):
    """augmentor_utils.py:606-611 for the whole batch: face_mask (N,) holds 6 bits per box row, the faces asked for (default: all six of every row;
    rows with box_cls == -2 never take part).  Returns counts (N, 6) int32 on the device, the live points per pyramid, and with member=True also
    (total_points, max_scene_boxes) uint8: per point row and box of its scene the faces whose pyramid holds the point.  One library call."""
    dev, N = batch.points.device, batch.total_boxes
    mask = _box_ints(batch, np.full(N, 63) if face_mask is None else face_mask)
    counts = torch.zeros(max(N, 1), 6, dtype=torch.int32, device=dev)
    stride = batch.max_scene_boxes if member else 0
    flags = torch.zeros(max(batch.total_points, 1), max(stride, 1), dtype=torch.uint8, device=dev) if member else None
    call("sv_pyramid_count", *batch._pt_args(), L.ptr(batch.keep), batch.batch_size, batch.max_scene_points, *batch._box_args(), L.ptr(batch.box_cls), N,
         L.ptr(mask), L.ptr(counts), L.ptr(flags), stride)
    return (counts[:N], flags[:batch.total_points]) if member else counts[:N]


def local_pyramid_dropout(batch, faces, u, dropout_prob):
    """augmentor_utils.py:614-627: faces / u (N,) are the draws randint(0, 6) and uniform(0, 1) per box row (rows that do not take part are not
    read: NaN is fine there); box row i loses the live points of face faces[i] when u[i] <= dropout_prob.  Returns the (N,) bool host mask of the
    boxes that dropped a face: they leave the pyramid list.  One library call."""
    u, faces = np.asarray(u, np.float64).reshape(-1), np.asarray(faces, np.float64).reshape(-1)
    assert len(u) == len(faces) == batch.total_boxes
    drop = np.zeros(len(u), bool)
    np.less_equal(u, float(dropout_prob), out=drop, where=~np.isnan(u))
    if drop.any():
        code = _box_ints(batch, np.where(drop, np.nan_to_num(faces), -1))
        call("sv_pyramid_dropout", *batch._pt_args(), L.ptr(batch.keep), batch.batch_size, batch.max_scene_points, *batch._box_args(), L.ptr(batch.box_cls),
             L.ptr(code))
    return drop


def plan_pyramid_sparsify(counts, selected, max_num, rngs=None, choices=None):
    """The count-dependent half of local_pyramid_sparsify (augmentor_utils.py:645-657) on the host.  counts (N, 6): the live points per pyramid as read
    from the device; selected[b] = (box rows, faces) of scene b's selected boxes in box order.  Per selected pyramid with more than max_num points,
    in order, choice(count, size=max_num, replace=False) from rngs[b] (or choices[b], the replay).  Returns the plan local_pyramid_sparsify runs:
    pyr rows (scene, box row, face, count, first output row relative to the scene's appended rows), ranks, the draws per scene and the rows to
    append per scene."""
    K = int(max_num)
    if not 0 <= K <= MAX_SPARSIFY_NUM:
        raise ValueError(f"SPARSIFY_MAX_NUM must be in 0..{MAX_SPARSIFY_NUM}, got {K}")
    pyr, ranks, drawn, room = [], [], [], []
    for b, (rows, faces) in enumerate(selected):
        mine = []
        for row, face in zip(rows, faces):
            c = int(counts[int(row), int(face)])
            if c <= K:
                continue
            if choices is None:
                idx = np.asarray(rngs[b].choice(c, size=K, replace=False), np.int64).reshape(-1)
            else:
                if len(mine) >= len(choices[b]):
                    raise ValueError(f"scene {b}: pyramid_sparsify_choice holds {len(choices[b])} draws, more pyramids than that hold over {K} points")
                idx = np.asarray(choices[b][len(mine)], np.int64).reshape(-1)
                if len(idx) != K or len(set(idx.tolist())) != K or (K and (idx.min() < 0 or idx.max() >= c)):
                    raise ValueError(f"scene {b}: a replayed choice is not {K} distinct indices below the pyramid's {c} points")
            pyr.append((b, int(row), int(face), c, len(mine) * K))
            ranks.append(idx)
            mine.append(idx)
        if choices is not None and len(mine) != len(choices[b]):
            raise ValueError(f"scene {b}: pyramid_sparsify_choice holds {len(choices[b])} draws for {len(mine)} pyramids over {K} points")
        drawn.append(mine)
        room.append(len(mine) * K)
    return {"pyr": np.array(pyr, np.int64).reshape(-1, 5), "ranks": np.array(ranks, np.int64).reshape(len(pyr), K), "K": K, "choices": drawn,
            "room": np.array(room, np.int64)}


def _plan_rows(batch, plan, key, column):
    """Make room behind the scenes for the plan's rows and turn its relative output rows into global ones; the table on the device."""
    first = batch.add_room(plan["room"])
    table = plan[key].copy()
    table[:, column] += first[table[:, 0]]
    return table


def local_pyramid_sparsify(batch, plan):
    """augmentor_utils.py:647-659 with a plan from plan_pyramid_sparsify: every member of a planned pyramid gets keep = 0 and the chosen ones are
    copied behind the scene's rows in choice order, pyramid after pyramid.  One library call (none for an empty plan), no host read; a count that
    differs from the plan's raises the batch's check flag."""
    if len(plan["pyr"]) == 0:
        return
    table = _plan_rows(batch, plan, "pyr", 4)
    up = torch.from_numpy(np.concatenate([table.reshape(-1), plan["ranks"].reshape(-1), [0]]).astype(np.int32)).to(batch.points.device)
    keep_in = batch.keep.clone()
    call("sv_pyramid_sparsify", *batch._pt_args(), L.ptr(keep_in), L.ptr(batch.keep), batch.batch_size, L.ptr(batch.boxes), batch.box_width, batch.total_boxes,
         L.ptr(up[:table.size]), len(table), L.ptr(up[table.size:]), plan["K"], L.ptr(_check_tensor(batch)))


def plan_pyramid_swap(counts, left, selected, max_num, rngs=None, faces=None, partners=None):
    """The count-dependent half of local_pyramid_swap (augmentor_utils.py:689-713) on the host.  counts (N, 6) as read from the device; left[b]: the
    box rows the swap looks at, in order; selected[b]: (k,) bool, the boxes whose uniform fell under SWAP_PROB.  Per selected box with a face of more
    than max_num points choice(its valid faces); the chosen pairs leave the valid table; per pair choice(boxes whose face is still valid), or the
    box itself without a draw.  faces / partners: the replay.  Returns the plan local_pyramid_swap runs: pairs (scene, box row, face, count,
    partner row, face, count, first output row relative to the scene's appended rows), the draws and the rows to append per scene."""
    pairs, f_out, p_out, room = [], [], [], []
    for b, rows in enumerate(left):
        rows, sel = np.asarray(rows, np.int64), np.asarray(selected[b], bool)
        nums = np.asarray(counts)[rows].reshape(len(rows), 6)
        valid = nums > int(max_num)
        chosen = valid & sel[:, None]
        ci = [i for i in range(len(rows)) if chosen[i].any()]
        if faces is None:
            cj = [int(rngs[b].choice(np.nonzero(chosen[i])[0])) for i in ci]
        else:
            cj = [int(v) for v in np.asarray(faces[b]).reshape(-1)]
            if len(cj) != len(ci) or not all(0 <= j < 6 and chosen[i, j] for i, j in zip(ci, cj)):
                raise ValueError(f"scene {b}: the replayed pyramid_swap_face does not name one valid face per selected box")
        valid[np.array(ci, np.int64), np.array(cj, np.int64)] = False
        part = []
        for t, (i, j) in enumerate(zip(ci, cj)):
            cand = np.nonzero(valid[:, j])[0]
            if partners is None:
                part.append(int(rngs[b].choice(cand)) if len(cand) else i)
            else:
                q = int(np.asarray(partners[b]).reshape(-1)[t]) if t < len(np.asarray(partners[b]).reshape(-1)) else -1
                if not (q in cand.tolist() if len(cand) else q == i):
                    raise ValueError(f"scene {b}: the replayed pyramid_swap_partner names no box whose face is still valid")
                part.append(q)
        if partners is not None and len(np.asarray(partners[b]).reshape(-1)) != len(ci):
            raise ValueError(f"scene {b}: pyramid_swap_partner holds another number of draws than there are pairs")
        at = 0
        for i, j, q in zip(ci, cj, part):
            pairs.append((b, rows[i], j, nums[i, j], rows[q], j, nums[q, j], at))
            at += int(nums[i, j] + nums[q, j])
        f_out.append(np.array(cj, np.int64))
        p_out.append(np.array(part, np.int64))
        room.append(at)
    return {"pairs": np.array(pairs, np.int64).reshape(-1, 8), "faces": f_out, "partners": p_out, "room": np.array(room, np.int64)}


def local_pyramid_swap(batch, plan):
    """augmentor_utils.py:716-761 with a plan from plan_pyramid_swap: the points of every involved pyramid get keep = 0; per pair the partner's points
    mapped into the to-swap pyramid and then the to-swap pyramid's points mapped into the partner are written behind the scene's rows (a self-swap
    and a partner shared by two pairs come out once per pair, as they do there).  One library call (none for an empty plan), no host read."""
    if len(plan["pairs"]) == 0:
        return
    if batch.num_point_features != 4:
        raise ValueError(f"local_pyramid_swap re-assembles x y z and the last column: points with {batch.num_point_features} columns cannot be "
                         "swapped (np.concatenate raises in the reference)")
    table = _plan_rows(batch, plan, "pairs", 7)
    up = torch.from_numpy(table.reshape(-1).astype(np.int32)).to(batch.points.device)
    keep_in = batch.keep.clone()
    call("sv_pyramid_swap", *batch._pt_args(), L.ptr(keep_in), L.ptr(batch.keep), batch.batch_size, L.ptr(batch.boxes), batch.box_width, batch.total_boxes,
         L.ptr(up), len(table), L.ptr(_check_tensor(batch)))


def launch_compact(batch, point_range=None, box_range=None, min_num_corners=0):
    """sv_augment_compact without the host read: (out_points, out_meta, gt, box_keep).  batch.keep holds the points' final flags afterwards."""
    dev, B, C, W = batch.points.device, batch.batch_size, batch.num_point_features, batch.box_width
    out_points = torch.empty(max(batch.total_points, 1), C + 1, dtype=torch.float32, device=dev)
    out_meta = torch.empty(3 * B + 1, dtype=torch.int32, device=dev)
    gt_stride = batch.max_scene_boxes
    gt = torch.empty(B, max(gt_stride, 1), W + 1, dtype=torch.float32, device=dev)
    box_keep = torch.zeros(max(batch.total_boxes, 1), dtype=torch.int32, device=dev)
    scratch = L.workspace.scratch("augment_compact", max(int(L.load().sv_augment_compact_scratch_bytes(B, batch.max_scene_points)), 4), dev)
    pr = None if point_range is None else L.host_array(ctypes.c_double, [float(point_range[i]) for i in (0, 1, 3, 4)])
    br = None if not min_num_corners else L.host_array(ctypes.c_double, [float(v) for v in list(box_range)[:6]])
    call("sv_augment_compact", *batch._pt_args(), L.ptr(batch.keep), B, batch.max_scene_points, pr, *batch._box_args(), L.ptr(batch.box_cls), br,
         int(min_num_corners), L.ptr(scratch), L.ptr(out_points), L.ptr(out_meta[:B + 1]), L.ptr(out_meta[B + 1:]), L.ptr(gt), gt_stride, L.ptr(box_keep))
    return out_points, out_meta, gt, box_keep


def compact(batch, point_range=None, box_range=None, min_num_corners=0, shuffle=None):
    """The tail of prepare_data and DataProcessor: the gt_boxes_mask / class filter with the class column (data_augmentor.py:265-267,
    dataset.py:152-157), mask_points_by_range (x / y, both bounds inclusive), mask_boxes_outside_range_numpy (min_num_corners > 0) and one stable
    compaction, with ONE host read for the B point counts and B box counts.  shuffle: None, or a list of one permutation per scene of its
    surviving points (shuffle_points with explicit draws), or True for device-generated ones.

    Returns points (P, 1 + C) [b, x, y, z, ...], scene_start (B + 1) / scene_cnt (B) int32 on the device, gt_boxes (B, max_gt, W + 1),
    points_per_scene / boxes_per_scene (host) and empty_scenes (scenes that ended with no box)."""
    B = batch.batch_size
    out_points, out_meta, gt, _ = launch_compact(batch, point_range, box_range, min_num_corners)
    counts = read_checked(batch, out_meta[B + 1:])
    points_per_scene, boxes_per_scene = counts[:B].astype(np.int64), counts[B:].astype(np.int64)
    points = out_points[:int(points_per_scene.sum())]
    if shuffle is not None and shuffle is not False:
        points = points[_shuffle_index(shuffle, points_per_scene, points.device)]
    return {"points": points, "scene_start": out_meta[:B + 1], "scene_cnt": out_meta[B + 1:2 * B + 1],
            "gt_boxes": gt[:, :int(boxes_per_scene.max())].contiguous(), "points_per_scene": points_per_scene,
            "boxes_per_scene": boxes_per_scene, "batch_size": B, "empty_scenes": [int(b) for b in np.nonzero(boxes_per_scene == 0)[0]]}


def _shuffle_index(shuffle, points_per_scene, dev):
    """shuffle_points (data_processor.py:93-103): a gather index that permutes every scene's rows among themselves."""
    starts = np.cumsum(points_per_scene) - points_per_scene
    if shuffle is True:
        total = int(points_per_scene.sum())
        scene = torch.repeat_interleave(torch.arange(len(points_per_scene), device=dev), torch.from_numpy(points_per_scene).to(dev), output_size=total)
        return torch.argsort(scene.double() + torch.rand(total, dtype=torch.float64, device=dev))
    idx = []
    for b, perm in enumerate(shuffle):
        perm = np.asarray(perm, np.int64)
        if sorted(perm.tolist()) != list(range(int(points_per_scene[b]))):
            raise ValueError(f"scene {b}: not a permutation of its {int(points_per_scene[b])} surviving points")
        idx.append(perm + starts[b])
    return torch.from_numpy(np.concatenate(idx) if idx else np.zeros(0, np.int64)).to(dev)
