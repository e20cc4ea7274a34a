"""KITTI AP evaluation on the GPU (reference: kitti_object_eval_python/eval.py, numba.jit + a numba.cuda overlap kernel).

Same function names, argument lists and return values as the reference.  One `eval_class` is: overlaps of every frame's own (detection, ground
truth) block in one launch -> pass 1 of the matching (true-positive scores) -> sort -> get_thresholds -> pass 2 (tp / fp / fn / similarity at every
threshold) -> ONE host read of the (combination, 41, 4) table and the threshold counts; recall, precision, AOS and the running maximum follow
on the host in fp64.  The number of library calls and host reads does not depend on the number of frames.  `clean_data` runs on the host,
vectorised over the concatenated annotations.  The cross-frame overlap blocks the reference computes and throws away are never computed:
`calculate_iou_partly` returns `parted_overlaps = None`, and `num_parts` is accepted and ignored.
"""
import io as sysio

import numpy as np
import torch

from ..... import _lib as L
from . import rotate_iou as R
from .rotate_iou import rotate_iou_gpu_eval

CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'truck']
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]
N_SAMPLE_PTS = 41


def max_detections_per_frame():
    """The most detections one frame may hold (a wave keeps their "assigned" flags in one 64-bit register per lane)."""
    return int(L.load().sv_kitti_eval_max_detections())


# ----------------------------------------------------------------------------------------------------------------------------------------
# host: clean_data, vectorised
# ----------------------------------------------------------------------------------------------------------------------------------------
def _name_codes(names):
    """Lower-cased names -> index in CLASS_NAMES (-1: none of them), and the case-sensitive DontCare flag; the string work runs once per DISTINCT name."""
    names = np.asarray(names)
    if names.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    uniq, inv = np.unique(names, return_inverse=True)
    code = np.array([CLASS_NAMES.index(str(u).lower()) if str(u).lower() in CLASS_NAMES else -1 for u in uniq], dtype=np.int64)
    dontcare = np.array([str(u) == "DontCare" for u in uniq], dtype=bool)
    inv = inv.reshape(-1)
    return code[inv], dontcare[inv]


def _ignored(gt_code, gt_occluded, gt_truncated, gt_bbox, dt_code, dt_bbox, current_class, difficulty):
    """ignored_gt, ignored_dt (int8) of clean_data for whole arrays of boxes."""
    current = CLASS_NAMES.index(CLASS_NAMES[current_class].lower())
    valid = np.where(gt_code == current, 1, -1)
    if CLASS_NAMES[current] == "pedestrian":
        valid[(gt_code == CLASS_NAMES.index("person_sitting")) & (valid != 1)] = 0
    elif CLASS_NAMES[current] == "car":
        valid[(gt_code == CLASS_NAMES.index("van")) & (valid != 1)] = 0
    height = gt_bbox[:, 3] - gt_bbox[:, 1]
    ignore = (gt_occluded > MAX_OCCLUSION[difficulty]) | (gt_truncated > MAX_TRUNCATION[difficulty]) | (height <= MIN_HEIGHT[difficulty])
    ignored_gt = np.where((valid == 1) & ~ignore, 0, np.where((valid == 0) | (ignore & (valid == 1)), 1, -1)).astype(np.int8)
    dt_height = np.abs(dt_bbox[:, 3] - dt_bbox[:, 1])
    ignored_dt = np.where(dt_height < MIN_HEIGHT[difficulty], 1, np.where(dt_code == current, 0, -1)).astype(np.int8)
    return ignored_gt, ignored_dt


def _bbox(anno):
    return np.asarray(anno["bbox"]).reshape(-1, 4)


def clean_data(gt_anno, dt_anno, current_class, difficulty):
    gt_code, dontcare = _name_codes(gt_anno["name"])
    dt_code, _ = _name_codes(dt_anno["name"])
    gt_bbox = _bbox(gt_anno)
    ignored_gt, ignored_dt = _ignored(gt_code, np.asarray(gt_anno["occluded"]), np.asarray(gt_anno["truncated"]), gt_bbox, dt_code, _bbox(dt_anno),
                                      current_class, difficulty)
    return int((ignored_gt == 0).sum()), ignored_gt.astype(np.int64).tolist(), ignored_dt.astype(np.int64).tolist(), list(gt_bbox[dontcare])


def _cat(annos, key, shape, dtype=None):
    parts = [np.asarray(a[key]).reshape(shape) for a in annos]
    out = np.concatenate(parts, 0) if parts else np.zeros(shape if shape[0] != -1 else (0,) + tuple(shape[1:]))
    return out.astype(dtype) if dtype is not None else out


def _metric_boxes(annos, metric):
    """The box columns calculate_iou_partly hands to each overlap (eval.py:360-393), concatenated over the frames, fp32."""
    if metric == 0:
        return _cat(annos, "bbox", (-1, 4), np.float32)
    loc, dims, rots = _cat(annos, "location", (-1, 3)), _cat(annos, "dimensions", (-1, 3)), _cat(annos, "rotation_y", (-1,))
    if metric == 1:
        loc, dims = loc[:, [0, 2]], dims[:, [0, 2]]
    elif metric != 2:
        raise ValueError("unknown metric")
    return np.ascontiguousarray(np.concatenate([loc, dims, rots[..., np.newaxis]], axis=1).astype(np.float32))


class _Frames:
    """The concatenated annotations of one evaluation and their per-frame offsets (host side)."""

    def __init__(self, gt_annos, dt_annos):
        assert len(gt_annos) == len(dt_annos)
        self._tables = {}
        self.num = len(gt_annos)
        self.gt_num = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
        self.dt_num = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
        cap = max_detections_per_frame() if self.num else 0
        if self.num and self.dt_num.max() > cap:
            raise ValueError(f"frame {int(self.dt_num.argmax())} holds {int(self.dt_num.max())} detections; the evaluation kernels take at most {cap} a frame")
        self.gt_off, self.dt_off, self.ov_off = R.offsets(self.gt_num), R.offsets(self.dt_num), R.offsets(self.gt_num * self.dt_num)
        self.gt_code, self.dontcare = _name_codes(_cat(gt_annos, "name", (-1,)))
        self.dt_code, _ = _name_codes(_cat(dt_annos, "name", (-1,)))
        self.gt_bbox, self.dt_bbox = _cat(gt_annos, "bbox", (-1, 4)), _cat(dt_annos, "bbox", (-1, 4))
        self.gt_occluded, self.gt_truncated = _cat(gt_annos, "occluded", (-1,)), _cat(gt_annos, "truncated", (-1,))
        self.gt_alpha, self.dt_alpha = _cat(gt_annos, "alpha", (-1,), np.float64), _cat(dt_annos, "alpha", (-1,), np.float64)
        self.dt_score = _cat(dt_annos, "score", (-1,), np.float64)
        frame_of_gt = np.repeat(np.arange(self.num), self.gt_num)
        self.dc_boxes = np.ascontiguousarray(self.gt_bbox[self.dontcare].astype(np.float32)).reshape(-1, 4)
        self.dc_off = R.offsets(np.bincount(frame_of_gt[self.dontcare], minlength=self.num))

    def tables(self, current_classes, difficultys):
        """ignored_gt (rows, total_gt), ignored_dt (rows, total_dt) int8 and total_num_valid_gt (rows), row = class index * len(difficultys) + difficulty index."""
        key = (tuple(current_classes), tuple(difficultys))
        if key in self._tables:
            return self._tables[key]
        ig, idt = [], []
        for current_class in current_classes:
            for difficulty in difficultys:
                a, b = _ignored(self.gt_code, self.gt_occluded, self.gt_truncated, self.gt_bbox, self.dt_code, self.dt_bbox, current_class, difficulty)
                ig.append(a), idt.append(b)
        ig, idt = np.stack(ig, 0), np.stack(idt, 0)
        self._tables[key] = ig, idt, (ig == 0).sum(1).astype(np.int32)
        return self._tables[key]


# ----------------------------------------------------------------------------------------------------------------------------------------
# device: matching
# ----------------------------------------------------------------------------------------------------------------------------------------
def match_on_device(overlaps, dt_off, gt_off, ov_off, dt_scores, ignored_dt, ignored_gt, combo_cd, min_overlaps, num_valid_gt, metric=1,
                    compute_aos=False, dt_bbox=None, dc_boxes=None, dc_off=None, gt_alpha=None, dt_alpha=None, detail=False):
    """Pass 1 -> sort -> thresholds -> pass 2 on device tensors (layouts: include/seevcn_hip.h).  Returns the device tensors
    (table (C, 41, 4) fp64, num_thresholds (C) int32); with detail=True also (sorted true-positive scores (C, total_gt), their counts (C),
    thresholds (C, 41)).  Four library calls, no host read."""
    dev = overlaps.device
    frames, combos = dt_off.numel() - 1, combo_cd.numel()
    total_dt, total_gt = dt_scores.numel(), ignored_gt.shape[1]
    assert overlaps.dtype == torch.float32 and dt_scores.dtype == min_overlaps.dtype == torch.float64
    assert ignored_dt.dtype == ignored_gt.dtype == torch.int8 and ignored_dt.shape == (ignored_gt.shape[0], total_dt)
    assert combo_cd.dtype == num_valid_gt.dtype == torch.int32 and min_overlaps.numel() == num_valid_gt.numel() == combos
    assert dt_off.dtype == gt_off.dtype == ov_off.dtype == torch.int64 and gt_off.numel() == ov_off.numel() == frames + 1
    if dc_off is None:
        dc_off = torch.zeros(frames + 1, dtype=torch.int64, device=dev)
    assert dc_off.dtype == torch.int64 and dc_off.numel() == frames + 1
    if metric == 0:
        assert dt_bbox.dtype == dc_boxes.dtype == torch.float32 and dt_bbox.shape == (total_dt, 4)
        if dc_boxes.numel() == 0:
            dc_boxes = torch.zeros(1, 4, dtype=torch.float32, device=dev)            # never read: every frame's DontCare run is empty
    if compute_aos:
        assert gt_alpha.dtype == dt_alpha.dtype == torch.float64 and gt_alpha.numel() == total_gt and dt_alpha.numel() == total_dt
    tp_scores = torch.full((combos, total_gt), float("-inf"), dtype=torch.float64, device=dev)
    tp_count = torch.zeros(combos, dtype=torch.int32, device=dev)
    common = (L.ptr(overlaps), L.ptr(dt_off), L.ptr(gt_off), L.ptr(ov_off), frames, L.ptr(dt_scores), L.ptr(ignored_dt), L.ptr(ignored_gt),
              L.ptr(combo_cd), L.ptr(min_overlaps), combos, total_dt, total_gt)
    R.call("sv_kitti_match_scores", *common, L.ptr(tp_scores), L.ptr(tp_count))
    sorted_scores = torch.sort(tp_scores, dim=1, descending=True).values.contiguous()
    thresholds = torch.zeros(combos, N_SAMPLE_PTS, dtype=torch.float64, device=dev)
    num_thresholds = torch.empty(combos, dtype=torch.int32, device=dev)
    R.call("sv_kitti_thresholds", L.ptr(sorted_scores), total_gt, L.ptr(tp_count), L.ptr(num_valid_gt), combos, L.ptr(thresholds), L.ptr(num_thresholds))
    counts = torch.zeros(combos, N_SAMPLE_PTS, 3, dtype=torch.int32, device=dev)
    table = torch.empty(combos, N_SAMPLE_PTS, 4, dtype=torch.float64, device=dev)
    sim_part = torch.empty(frames, combos, N_SAMPLE_PTS, dtype=torch.float64, device=dev) if compute_aos else None
    R.call("sv_kitti_match_stats", *common, L.ptr(thresholds), L.ptr(num_thresholds), int(metric), int(bool(compute_aos)),
           L.ptr(dt_bbox) if metric == 0 else None, L.ptr(dc_boxes) if metric == 0 else None, L.ptr(dc_off), L.ptr(gt_alpha) if compute_aos else None,
           L.ptr(dt_alpha) if compute_aos else None, L.ptr(counts), L.ptr(sim_part), L.ptr(table))
    if detail:
        return table, num_thresholds, sorted_scores, tp_count, thresholds
    return table, num_thresholds


def get_thresholds(scores, num_gt, num_sample_pts=41):
    """The reference's recall-sampled score thresholds, computed on the device in fp64; returns a list."""
    if num_sample_pts != N_SAMPLE_PTS:
        raise ValueError(f"the thresholds kernel samples {N_SAMPLE_PTS} recall points")
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    if scores.size == 0:
        return []
    dev = R.device()
    s = torch.sort(torch.from_numpy(scores).to(dev).reshape(1, -1), dim=1, descending=True).values.contiguous()
    thresholds = torch.zeros(1, N_SAMPLE_PTS, dtype=torch.float64, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    sizes = torch.tensor([scores.size, int(num_gt)], dtype=torch.int32, device=dev)          # named: it must outlive the launch
    R.call("sv_kitti_thresholds", L.ptr(s), scores.size, sizes.data_ptr(), sizes.data_ptr() + 4, 1, L.ptr(thresholds), L.ptr(n))
    out = R.read(torch.cat([thresholds.reshape(-1), n.to(torch.float64)]))
    return out[:int(out[-1])].tolist()


# ----------------------------------------------------------------------------------------------------------------------------------------
# overlaps with the reference's signatures
# ----------------------------------------------------------------------------------------------------------------------------------------
def image_box_overlap(boxes, query_boxes, criterion=-1):
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    N, K = boxes.shape[0], query_boxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=boxes.dtype)
    return R.ragged_overlaps(boxes, query_boxes, [N], [K], 0, criterion)[0].astype(boxes.dtype)


def bev_box_overlap(boxes, qboxes, criterion=-1):
    return rotate_iou_gpu_eval(boxes, qboxes, criterion)


def d3_box_overlap(boxes, qboxes, criterion=-1):
    boxes, qboxes = np.asarray(boxes), np.asarray(qboxes)
    N, K = boxes.shape[0], qboxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=np.float32)
    return R.ragged_overlaps(boxes, qboxes, [N], [K], 2, criterion)[0]


def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50):
    """Per-frame overlaps, rows = the first argument's boxes (eval_class passes the detections first, as the reference does).  Returns
    (overlaps, None, total_gt_num, total_dt_num): only each frame's own block is computed, so there are no parted (cross-frame) overlaps."""
    assert len(gt_annos) == len(dt_annos)
    total_dt_num = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
    total_gt_num = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
    blocks = R.ragged_overlaps(_metric_boxes(gt_annos, metric), _metric_boxes(dt_annos, metric), total_gt_num, total_dt_num, metric)
    if metric != 0:
        blocks = [b.astype(np.float64) for b in blocks]
    return blocks, None, total_gt_num, total_dt_num


# ----------------------------------------------------------------------------------------------------------------------------------------
# eval_class and above
# ----------------------------------------------------------------------------------------------------------------------------------------
def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=100, detail=None, frames=None):
    """Kitti eval. support 2d/bev/3d/aos eval.
    Args:
        gt_annos, dt_annos: lists of annotation dicts of numpy arrays
        current_classes: list of int, 0: car, 1: pedestrian, 2: cyclist, ...
        difficultys: list of int. eval difficulty, 0: easy, 1: normal, 2: hard
        metric: eval type. 0: bbox, 1: bev, 2: 3d
        min_overlaps: float, min overlap. format: [num_overlap, metric, class].
        num_parts: accepted and ignored
        detail: a dict, for tests and tools: receives the kernels' intermediates as numpy (one extra host read): "overlaps" (flat, frame blocks
            of (n_dt, n_gt)), "ov_off", and per combination in (class, difficulty, min-overlap row) order "tp_scores" (sorted, descending),
            "tp_count", "thresholds", "num_thresholds", "table" (combinations, 41, 4)
        frames: the `_Frames` of these very annotations (do_eval concatenates them once for its three metrics)
    Returns:
        dict of recall, precision and aos
    """
    assert len(gt_annos) == len(dt_annos)
    if metric not in (0, 1, 2):
        raise ValueError("unknown metric")
    min_overlaps = np.asarray(min_overlaps, dtype=np.float64)
    num_minoverlap, num_class, num_difficulty = len(min_overlaps), len(current_classes), len(difficultys)
    shape = [num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS]
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    ret_dict = {"recall": recall, "precision": precision, "orientation": aos}
    used = min_overlaps[:, metric, :num_class]
    if used.size and not (used >= 0).all():
        raise ValueError("a negative min_overlap is not supported: pass 2 of the matching relies on min_overlap >= 0")
    fr = frames if frames is not None else _Frames(gt_annos, dt_annos)
    total_pairs = int(fr.ov_off[-1])
    if total_pairs == 0 or used.size == 0 or num_difficulty == 0:
        return ret_dict                                   # no (detection, ground truth) pair anywhere: no true positive, no threshold, zero rows
    ignored_gt, ignored_dt, num_valid = fr.tables(current_classes, difficultys)
    # combination c = (class m, difficulty l, min-overlap row k), in that order
    m, l, k = np.meshgrid(np.arange(num_class), np.arange(num_difficulty), np.arange(num_minoverlap), indexing="ij")
    combo_cd = (m * num_difficulty + l).reshape(-1).astype(np.int32)
    combo_mo = np.ascontiguousarray(used[k.reshape(-1), m.reshape(-1)])

    dev = R.device()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dt_off, gt_off, ov_off = up(fr.dt_off), up(fr.gt_off), up(fr.ov_off)
    dt_bbox = up(fr.dt_bbox.astype(np.float32)) if metric == 0 else None
    dt_boxes = dt_bbox if metric == 0 else up(_metric_boxes(dt_annos, metric))
    overlaps = R.ragged_overlaps_device(dt_boxes, up(_metric_boxes(gt_annos, metric)), dt_off, gt_off, ov_off, total_pairs, metric, -1)
    out = match_on_device(
        overlaps, dt_off, gt_off, ov_off, up(fr.dt_score), up(ignored_dt), up(ignored_gt), up(combo_cd), up(combo_mo), up(num_valid[combo_cd]), metric,
        compute_aos, dt_bbox, up(fr.dc_boxes) if metric == 0 else None, up(fr.dc_off), up(fr.gt_alpha) if compute_aos else None,
        up(fr.dt_alpha) if compute_aos else None, detail=detail is not None)
    table, num_thresholds = out[:2]
    if detail is not None:
        parts = [overlaps.to(torch.float64), out[2].reshape(-1), out[3].to(torch.float64), out[4].reshape(-1)]
        sizes = np.cumsum([p_.numel() for p_ in parts])
        host = R.read(torch.cat(parts))
        detail.update(overlaps=host[:sizes[0]].astype(np.float32), ov_off=fr.ov_off, tp_scores=host[sizes[0]:sizes[1]].reshape(len(combo_cd), -1),
                      tp_count=host[sizes[1]:sizes[2]].astype(np.int64), thresholds=host[sizes[2]:].reshape(len(combo_cd), N_SAMPLE_PTS))
    flat = R.read(torch.cat([table.reshape(-1), num_thresholds.to(torch.float64)]))
    combos = len(combo_cd)
    pr = flat[:combos * N_SAMPLE_PTS * 4].reshape(num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS, 4)
    live = np.arange(N_SAMPLE_PTS) < flat[combos * N_SAMPLE_PTS * 4:].reshape(num_class, num_difficulty, num_minoverlap, 1)
    if detail is not None:
        detail.update(table=pr.reshape(combos, N_SAMPLE_PTS, 4).copy(), num_thresholds=flat[combos * N_SAMPLE_PTS * 4:].astype(np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        recall[live] = (pr[..., 0] / (pr[..., 0] + pr[..., 2]))[live]
        precision[live] = (pr[..., 0] / (pr[..., 0] + pr[..., 1]))[live]
        if compute_aos:
            aos[live] = (pr[..., 3] / (pr[..., 0] + pr[..., 1]))[live]
    for a in (precision, recall) + ((aos,) if compute_aos else ()):        # eval.py:542-547: the maximum over [i:], rows past the thresholds stay 0
        a[...] = np.where(live, np.maximum.accumulate(a[..., ::-1], axis=-1)[..., ::-1], a)
    return ret_dict


def get_mAP(prec):
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def get_mAP_R40(prec):
    sums = 0
    for i in range(1, prec.shape[-1]):
        sums = sums + prec[..., i]
    return sums / 40 * 100


def print_str(value, *arg, sstream=None):
    if sstream is None:
        sstream = sysio.StringIO()
    sstream.truncate(0)
    sstream.seek(0)
    print(value, *arg, file=sstream)
    return sstream.getvalue()


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, PR_detail_dict=None):
    # min_overlaps: [num_minoverlap, metric, num_class]
    difficultys = [0, 1, 2]
    frames = _Frames(gt_annos, dt_annos)          # concatenated once, shared by the three metrics
    ret = eval_class(gt_annos, dt_annos, current_classes, difficultys, 0, min_overlaps, compute_aos, frames=frames)
    # ret: [num_class, num_diff, num_minoverlap, num_sample_points]
    mAP_bbox = get_mAP(ret["precision"])
    mAP_bbox_R40 = get_mAP_R40(ret["precision"])
    if PR_detail_dict is not None:
        PR_detail_dict['bbox'] = ret['precision']
    mAP_aos = mAP_aos_R40 = None
    if compute_aos:
        mAP_aos = get_mAP(ret["orientation"])
        mAP_aos_R40 = get_mAP_R40(ret["orientation"])
        if PR_detail_dict is not None:
            PR_detail_dict['aos'] = ret['orientation']
    ret = eval_class(gt_annos, dt_annos, current_classes, difficultys, 1, min_overlaps, frames=frames)
    mAP_bev = get_mAP(ret["precision"])
    mAP_bev_R40 = get_mAP_R40(ret["precision"])
    if PR_detail_dict is not None:
        PR_detail_dict['bev'] = ret['precision']
    ret = eval_class(gt_annos, dt_annos, current_classes, difficultys, 2, min_overlaps, frames=frames)
    mAP_3d = get_mAP(ret["precision"])
    mAP_3d_R40 = get_mAP_R40(ret["precision"])
    if PR_detail_dict is not None:
        PR_detail_dict['3d'] = ret['precision']
    return mAP_bbox, mAP_bev, mAP_3d, mAP_aos, mAP_bbox_R40, mAP_bev_R40, mAP_3d_R40, mAP_aos_R40


CLASS_TO_NAME = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck'}


def official_min_overlaps():
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])
    return np.stack([overlap_0_7, overlap_0_5], axis=0)  # [2, 3, 6]


def format_official_result(current_classes, min_overlaps, compute_aos, mAPs):
    """The result string and ret_dict of get_official_eval_result from do_eval's eight values."""
    mAPbbox, mAPbev, mAP3d, mAPaos, mAPbbox_R40, mAPbev_R40, mAP3d_R40, mAPaos_R40 = mAPs
    class_to_name = CLASS_TO_NAME
    result = ''
    ret_dict = {}
    for j, curcls in enumerate(current_classes):
        # mAP threshold array: [num_minoverlap, metric, class]
        # mAP result: [num_class, num_diff, num_minoverlap]
        for i in range(min_overlaps.shape[0]):
            result += print_str((f"{class_to_name[curcls]} " "AP@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j])))
            result += print_str((f"bbox AP:{mAPbbox[j, 0, i]:.4f}, " f"{mAPbbox[j, 1, i]:.4f}, " f"{mAPbbox[j, 2, i]:.4f}"))
            result += print_str((f"bev  AP:{mAPbev[j, 0, i]:.4f}, " f"{mAPbev[j, 1, i]:.4f}, " f"{mAPbev[j, 2, i]:.4f}"))
            result += print_str((f"3d   AP:{mAP3d[j, 0, i]:.4f}, " f"{mAP3d[j, 1, i]:.4f}, " f"{mAP3d[j, 2, i]:.4f}"))
            if compute_aos:
                result += print_str((f"aos  AP:{mAPaos[j, 0, i]:.2f}, " f"{mAPaos[j, 1, i]:.2f}, " f"{mAPaos[j, 2, i]:.2f}"))
            result += print_str((f"{class_to_name[curcls]} " "AP_R40@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j])))
            result += print_str((f"bbox AP:{mAPbbox_R40[j, 0, i]:.4f}, " f"{mAPbbox_R40[j, 1, i]:.4f}, " f"{mAPbbox_R40[j, 2, i]:.4f}"))
            result += print_str((f"bev  AP:{mAPbev_R40[j, 0, i]:.4f}, " f"{mAPbev_R40[j, 1, i]:.4f}, " f"{mAPbev_R40[j, 2, i]:.4f}"))
            result += print_str((f"3d   AP:{mAP3d_R40[j, 0, i]:.4f}, " f"{mAP3d_R40[j, 1, i]:.4f}, " f"{mAP3d_R40[j, 2, i]:.4f}"))
            if compute_aos:
                result += print_str((f"aos  AP:{mAPaos_R40[j, 0, i]:.2f}, " f"{mAPaos_R40[j, 1, i]:.2f}, " f"{mAPaos_R40[j, 2, i]:.2f}"))
                if i == 0:
                    ret_dict['%s_aos/easy_R40' % class_to_name[curcls]] = mAPaos_R40[j, 0, 0]
                    ret_dict['%s_aos/moderate_R40' % class_to_name[curcls]] = mAPaos_R40[j, 1, 0]
                    ret_dict['%s_aos/hard_R40' % class_to_name[curcls]] = mAPaos_R40[j, 2, 0]
            if i == 0:
                ret_dict['%s_3d/easy_R40' % class_to_name[curcls]] = mAP3d_R40[j, 0, 0]
                ret_dict['%s_3d/moderate_R40' % class_to_name[curcls]] = mAP3d_R40[j, 1, 0]
                ret_dict['%s_3d/hard_R40' % class_to_name[curcls]] = mAP3d_R40[j, 2, 0]
                ret_dict['%s_bev/easy_R40' % class_to_name[curcls]] = mAPbev_R40[j, 0, 0]
                ret_dict['%s_bev/moderate_R40' % class_to_name[curcls]] = mAPbev_R40[j, 1, 0]
                ret_dict['%s_bev/hard_R40' % class_to_name[curcls]] = mAPbev_R40[j, 2, 0]
                ret_dict['%s_image/easy_R40' % class_to_name[curcls]] = mAPbbox_R40[j, 0, 0]
                ret_dict['%s_image/moderate_R40' % class_to_name[curcls]] = mAPbbox_R40[j, 1, 0]
                ret_dict['%s_image/hard_R40' % class_to_name[curcls]] = mAPbbox_R40[j, 2, 0]
    return result, ret_dict


def resolve_classes(current_classes):
    name_to_class = {v: n for n, v in CLASS_TO_NAME.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    return [name_to_class[c] if isinstance(c, str) else c for c in current_classes]


def detect_compute_aos(dt_annos):
    """AOS is evaluated when the first non-empty detection frame's first alpha is not -10."""
    for anno in dt_annos:
        if anno['alpha'].shape[0] != 0:
            return bool(anno['alpha'][0] != -10)
    return False


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None):
    current_classes = resolve_classes(current_classes)
    min_overlaps = official_min_overlaps()[:, :, current_classes]
    compute_aos = detect_compute_aos(dt_annos)
    mAPs = do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos, PR_detail_dict=PR_detail_dict)
    return format_official_result(current_classes, min_overlaps, compute_aos, mAPs)
