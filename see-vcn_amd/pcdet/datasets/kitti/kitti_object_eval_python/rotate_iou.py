"""Rotated-box overlap of the KITTI evaluation (reference: kitti_object_eval_python/rotate_iou.py, a numba.cuda kernel) on csrc/kitti_eval.hip.

`ragged_overlaps` is the one launch behind every overlap of the package: segment s owns a run of row boxes and a run of column boxes and only
its (rows, cols) block is computed.  `rotate_iou_gpu_eval` is the same entry with one segment.  The intersection follows the reference's fp32
statements; its polygon buffer holds 8 points and a candidate past that is dropped, where the reference writes past its local array.
"""
import numpy as np
import torch

from ..... import _lib as L
from ..... import data_pipeline as P

# library calls and blocking device -> host reads made by this package since the last reset_counters(); neither depends on the number of frames
_counted = P.Counted()
COUNTERS, reset_counters, call, read = _counted.counters, _counted.reset, _counted.call, _counted.read


def device(device_id=0):
    if not torch.cuda.is_available():
        raise L.SeevcnHipError("the KITTI evaluation runs on the GPU only; there is no CPU fallback")
    return torch.device("cuda", device_id)


BOX_WIDTH = {0: 4, 1: 5, 2: 7}


def offsets(counts):
    out = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=out[1:])
    return out


def ragged_overlaps_device(row_boxes, col_boxes, row_off, col_off, out_off, total_pairs, metric, criterion):
    """Device tensors in, the flat fp32 overlap buffer out (block s = (rows_s, cols_s) row-major at out_off[s]).  total_pairs >= 1."""
    if metric not in BOX_WIDTH:
        raise ValueError("unknown metric")
    if criterion not in (-1, 0, 1) + ((2,) if metric else ()):
        raise ValueError(f"criterion {criterion} is not defined for metric {metric}")
    assert row_boxes.dtype == col_boxes.dtype == torch.float32 and row_boxes.shape[1] == col_boxes.shape[1] == BOX_WIDTH[metric]
    assert row_off.dtype == col_off.dtype == out_off.dtype == torch.int64 and row_off.numel() == col_off.numel() == out_off.numel() >= 2
    out = torch.empty(int(total_pairs), dtype=torch.float32, device=row_boxes.device)
    call("sv_kitti_overlaps", L.ptr(row_boxes), L.ptr(col_boxes), L.ptr(row_off), L.ptr(col_off), L.ptr(out_off), row_off.numel() - 1, int(total_pairs),
         int(metric), int(criterion), L.ptr(out))
    return out


def ragged_overlaps(row_boxes, col_boxes, row_counts, col_counts, metric, criterion=-1, device_id=0):
    """numpy in, list of per-segment (rows_s, cols_s) fp32 numpy blocks out: one upload, at most one launch, at most one read."""
    row_counts, col_counts = np.asarray(row_counts, dtype=np.int64), np.asarray(col_counts, dtype=np.int64)
    width = BOX_WIDTH[metric] if metric in BOX_WIDTH else None
    if width is None:
        raise ValueError("unknown metric")
    row_boxes = np.ascontiguousarray(np.asarray(row_boxes, dtype=np.float32).reshape(-1, width))
    col_boxes = np.ascontiguousarray(np.asarray(col_boxes, dtype=np.float32).reshape(-1, width))
    assert row_counts.sum() == len(row_boxes) and col_counts.sum() == len(col_boxes) and len(row_counts) == len(col_counts)
    out_off = offsets(row_counts * col_counts)
    total = int(out_off[-1])
    if total == 0:
        flat = np.zeros(0, dtype=np.float32)
    else:
        dev = device(device_id)
        up = lambda a: torch.from_numpy(a).to(dev)
        flat = read(ragged_overlaps_device(up(row_boxes), up(col_boxes), up(offsets(row_counts)), up(offsets(col_counts)), up(out_off), total, metric,
                                           criterion))
    return [flat[out_off[s]:out_off[s + 1]].reshape(row_counts[s], col_counts[s]) for s in range(len(row_counts))]


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """(N, 5) and (K, 5) boxes (centre, dims, angle) -> (N, K) fp32: out[n, k] = devRotateIoUEval(query_boxes[k], boxes[n], criterion)."""
    boxes = np.asarray(boxes).astype(np.float32)
    query_boxes = np.asarray(query_boxes).astype(np.float32)
    N, K = boxes.shape[0], query_boxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=np.float32)
    return ragged_overlaps(boxes, query_boxes, [N], [K], 1, criterion, device_id)[0]
