"""Box helpers with the reference's names (detector3d/pcdet/utils/box_utils.py)."""
import torch

from . import common_utils


def enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    """boxes (N,7+C): dims grow by extra_width (box_utils.py:182-195)."""
    boxes3d, is_numpy = common_utils.check_numpy_to_torch(boxes3d)
    large = boxes3d.clone()
    large[:, 3:6] += common_utils.const_tensor(extra_width, boxes3d.device, boxes3d.dtype)[None, :]
    return large


def boxes_to_corners_3d(boxes3d):
    """(N,7) -> (N,8,3) corners in the reference's order (box_utils.py:28-52)."""
    boxes3d, is_numpy = common_utils.check_numpy_to_torch(boxes3d)
    template = common_utils.const_tensor(([1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1],
                                          [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]), boxes3d.device, boxes3d.dtype) / 2
    corners3d = boxes3d[:, None, 3:6].repeat(1, 8, 1) * template[None, :, :]
    corners3d = common_utils.rotate_points_along_z(corners3d.view(-1, 8, 3), boxes3d[:, 6]).view(-1, 8, 3)
    corners3d += boxes3d[:, None, 0:3]
    return corners3d.numpy() if is_numpy else corners3d


def mask_boxes_outside_range(boxes, limit_range, min_num_corners=1):
    """mask_boxes_outside_range_numpy (box_utils.py:93-109) on the device: boxes (N, 7 + C) fp32 -> (N,) bool, true where at least
    min_num_corners of the 8 corners lie inside limit_range (both bounds inclusive).  No host read."""
    from ..datasets.augmentor import augmentor_utils as A
    import numpy as np
    n, per = len(boxes), A.MAX_BOXES_PER_SCENE                     # the kernel's unit is a scene of at most 256 boxes
    sizes = [min(per, n - i) for i in range(0, n, per)] or [0]
    batch = A.DeviceBatch(boxes.new_zeros(0, 3), boxes, np.zeros(n, np.int32), [0] * len(sizes), sizes)
    return A.launch_compact(batch, None, limit_range, min_num_corners)[3][:len(boxes)].bool()


def remove_points_in_boxes3d(points, boxes3d):
    """box_utils.py:112-126 on the device: the points (N, 3 + C) that lie in none of boxes3d (M <= 256, 7 + C) by the CPU matrix test (margin 1e-2
    in x / y, none in z), in order.  The one kernel GT sampling removes covered scene points with, every box taken as accepted."""
    from ..datasets.augmentor import augmentor_utils as A
    import numpy as np
    from ... import _lib as L
    n, m, dev = len(points), len(boxes3d), points.device
    if n == 0 or m == 0:
        return points
    batch = A.DeviceBatch(points, boxes3d[:, :7].contiguous(), np.zeros(m, np.int32), [n], [m])
    zeros = torch.zeros(m + 2, dtype=torch.int64, device=dev)
    idx = torch.arange(m, dtype=torch.int32, device=dev)
    ones = torch.ones(m, dtype=torch.int32, device=dev)
    start = torch.tensor([0, m], dtype=torch.int32, device=dev)
    z32 = zeros.to(torch.int32)
    A.call("sv_gt_sample_paste", *batch._pt_args(), L.ptr(z32[:1]), L.ptr(batch.keep), 1, n, None, L.ptr(zeros), L.ptr(batch.boxes), 7, L.ptr(idx),
           L.ptr(start), L.ptr(z32[:m + 1]), L.ptr(z32[:m]), L.ptr(ones), m, 0, 0.0, 0.0, 0.0)
    return points[batch.keep[:n].bool()]
