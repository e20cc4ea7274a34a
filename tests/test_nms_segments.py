"""sv_nms_segments (segmented class-wise NMS: many box sets, one launch pair) against the oracle's NMS run segment by segment: keep lists and
counts element for element.  The boxes are drawn so that no pair's IoU, rotated or axis-aligned, lies within 1e-3 of the threshold: every
suppression is decided far above fp32 rounding, so no pair is left out of the comparison."""
import functools

import numpy as np
import pytest
import torch

from oracle import boxes as ob

F = np.float32
THRESH = 0.3
MARGIN = 1e-3


def _iou_normal(a, b):
    """iou3d_nms_kernel.cu:304-314 in fp32, a (7,) against b (M, 7)"""
    left, right = np.maximum(a[0] - a[3] / F(2), b[:, 0] - b[:, 3] / F(2)), np.minimum(a[0] + a[3] / F(2), b[:, 0] + b[:, 3] / F(2))
    top, bottom = np.maximum(a[1] - a[4] / F(2), b[:, 1] - b[:, 4] / F(2)), np.minimum(a[1] + a[4] / F(2), b[:, 1] + b[:, 4] / F(2))
    inter = np.maximum(right - left, F(0)) * np.maximum(bottom - top, F(0))
    return inter / np.maximum(a[3] * a[4] + b[:, 3] * b[:, 4] - inter, F(1e-8))


def _draw(rng, n, extent):
    b = np.zeros((n, 7), F)
    b[:, 0:2] = rng.uniform(0, extent, (n, 2))
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3], b[:, 4], b[:, 5] = rng.uniform(3, 5, n), rng.uniform(1.5, 2.2, n), rng.uniform(1.4, 1.8, n)
    b[:, 6] = rng.uniform(-3.1, 3.1, n)
    return b


def decided_boxes(rng, n, extent):
    """n boxes, no pair of which has a rotated or axis-aligned IoU within MARGIN of THRESH.  Only pairs whose bounding circles meet are
    evaluated: apart, both overlaps are exactly 0 in any arithmetic.  A box of an undecided pair is drawn again."""
    b = _draw(rng, n, extent)
    todo = np.arange(n)
    while len(todo):
        again = set()
        radius = F(0.5) * np.sqrt(b[:, 3] ** 2 + b[:, 4] ** 2)
        for i in todo:
            d = np.hypot(b[:, 0] - b[i, 0], b[:, 1] - b[i, 1])
            near = np.nonzero((d <= radius + radius[i] + 0.1) & (np.arange(n) != i))[0]
            if len(near) == 0:
                continue
            rot = ob.boxes_iou_bev(b[i:i + 1], b[near])[0]
            bad = (np.abs(rot - THRESH) <= MARGIN) | (np.abs(_iou_normal(b[i], b[near]) - THRESH) <= MARGIN)
            if bad.any():
                again.add(int(i))
        todo = np.array(sorted(again), dtype=np.int64)
        b[todo] = _draw(rng, len(todo), extent)
    return b


def _segments(counts, stride, extent_of):
    rng = np.random.default_rng(len(counts) * 1000 + stride)
    boxes = np.zeros((len(counts), stride, 7), F)
    for s, n in enumerate(counts):
        if n:
            boxes[s, :n] = decided_boxes(rng, n, extent_of(n))
            boxes[s, n:] = boxes[s, 0]              # padding = copies of the top box: read as a row it would suppress every column, as a column be kept
        else:
            boxes[s] = _draw(rng, 1, 10.0)[0]
    return boxes


@functools.lru_cache(maxsize=None)
def small_case():
    counts = [0, 1, 63, 64, 65, 129, 200, 200]
    boxes = _segments(counts, 200, lambda n: 2.2 * np.sqrt(n) + 4.0)            # dense enough that a good part of every set is suppressed
    ref = {normal: [ob.nms(boxes[s, :n], THRESH, normal=bool(normal)) for s, n in enumerate(counts)] for normal in (0, 1)}
    return counts, boxes, ref


@functools.lru_cache(maxsize=None)
def wide_case():
    counts = [4096, 70]
    boxes = _segments(counts, 4096, lambda n: 2.2 * np.sqrt(n) + 4.0)
    ref = [ob.nms(boxes[s, :n], THRESH) for s, n in enumerate(counts)]
    return counts, boxes, ref


TWIN_SIZES = (1, 64, 65, 130)            # below, at and across a block edge, and a short last block


@functools.lru_cache(maxsize=None)
def twin_case(n):
    """one score-sorted set of n decided boxes for both NMS families, with the oracle's keep list per `normal`"""
    boxes = decided_boxes(np.random.default_rng(7000 + n), n, 2.2 * np.sqrt(n) + 4.0)
    return boxes, {normal: ob.nms(boxes, THRESH, normal=bool(normal)) for normal in (0, 1)}


def run_prefix(hip_lib, cuda, boxes, normal, max_keep):
    import seevcn_amd._lib as L
    n = len(boxes)
    b = torch.from_numpy(boxes).to(cuda)
    keep = torch.full((max_keep,), -7, dtype=torch.int64, device=cuda)
    num = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    scratch = torch.empty((hip_lib.sv_nms_scratch_bytes(n),), dtype=torch.uint8, device=cuda)
    rc = hip_lib.sv_nms_prefix(L.ptr(b), n, THRESH, normal, max_keep, L.ptr(scratch), L.ptr(keep), L.ptr(num), L.stream())
    L.check(rc, "sv_nms_prefix")
    return keep.cpu().numpy(), int(num.cpu().numpy()[0])


def run_segments(hip_lib, cuda, boxes, counts, normal, max_keep):
    import seevcn_amd._lib as L
    S, stride = boxes.shape[:2]
    b = torch.from_numpy(boxes).to(cuda)
    cnt = torch.tensor(counts, dtype=torch.int32, device=cuda)
    keep = torch.full((S, max_keep), -7, dtype=torch.int64, device=cuda)
    num = torch.full((S,), -7, dtype=torch.int32, device=cuda)
    nbytes = hip_lib.sv_nms_segments_scratch_bytes(S, stride)
    assert nbytes == S * stride * ((stride + 63) // 64) * 8
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=cuda)
    rc = hip_lib.sv_nms_segments(L.ptr(b), L.ptr(cnt), S, stride, THRESH, normal, max_keep, L.ptr(scratch), L.ptr(keep), L.ptr(num), L.stream())
    L.check(rc, "sv_nms_segments")
    return keep.cpu().numpy(), num.cpu().numpy()


def check(keep, num, ref, max_keep):
    for s, want in enumerate(ref):
        assert num[s] == min(len(want), max_keep), (s, num[s], len(want))
        assert np.array_equal(keep[s, :num[s]], want[:max_keep]), s
        assert (keep[s, num[s]:] == -7).all(), s                                   # nothing written past the count


def test_cases_are_decided_and_suppress():
    counts, boxes, ref = small_case()
    for normal in (0, 1):
        kept = [len(k) for k in ref[normal]]
        assert kept[0] == 0 and kept[1] == 1 and all(1 < k < n for k, n in zip(kept[2:], counts[2:])), kept
    for s, n in enumerate(counts[2:], start=2):
        iou = ob.boxes_iou_bev(boxes[s, :n], boxes[s, :n])
        assert np.abs(iou - THRESH).min() > MARGIN
    for n in TWIN_SIZES:
        boxes, ref = twin_case(n)
        assert np.abs(ob.boxes_iou_bev(boxes, boxes) - THRESH).min() > MARGIN
        assert min(np.abs(_iou_normal(boxes[i], boxes) - THRESH).min() for i in range(n)) > MARGIN
        for normal in (0, 1):
            assert 1 <= len(ref[normal]) <= n and (n < 64 or len(ref[normal]) < n), (n, normal, len(ref[normal]))


@pytest.mark.gpu
@pytest.mark.parametrize("keep_two", [False, True])
@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("n", TWIN_SIZES)
def test_hip_nms_prefix_and_one_segment_keep_the_same_boxes(cuda, hip_lib, n, normal, keep_two):
    """The two NMS families share the mask tile and the in-block resolve: the same score-sorted boxes through sv_nms_prefix and through
    sv_nms_segments as its only segment (S = 1, seg_stride = n) give the same count and the same keep list, which is the oracle's."""
    boxes, ref = twin_case(n)
    max_keep = 2 if keep_two else n
    keep_p, num_p = run_prefix(hip_lib, cuda, boxes, normal, max_keep)
    keep_s, num_s = run_segments(hip_lib, cuda, boxes[None], [n], normal, max_keep)
    assert num_p == num_s[0]
    assert np.array_equal(keep_p[:num_p], keep_s[0, :num_p])
    check(keep_s, num_s, [ref[normal]], max_keep)
    assert (keep_p[num_p:] == -7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("keep_all", [False, True])
def test_hip_nms_segments_equal_the_oracle_segment_by_segment(cuda, hip_lib, normal, keep_all):
    counts, boxes, ref = small_case()
    survivors = [len(k) for k in ref[normal]]
    max_keep = 256 if keep_all else min(k for k in survivors if k > 1) - 1          # >= seg_stride, or below the smallest non-trivial count
    assert max_keep >= 2
    keep, num = run_segments(hip_lib, cuda, boxes, counts, normal, max_keep)
    check(keep, num, ref[normal], max_keep)


@pytest.mark.gpu
def test_hip_nms_segments_at_the_widest_stride(cuda, hip_lib):
    """seg_stride 4096 = 64 column blocks, one full segment beside a short one, in one launch pair"""
    counts, boxes, ref = wide_case()
    keep, num = run_segments(hip_lib, cuda, boxes, counts, 0, 4096)
    check(keep, num, ref, 4096)
    assert 64 < len(ref[0]) < 4096
