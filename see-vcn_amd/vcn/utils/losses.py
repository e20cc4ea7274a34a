import torch


def geodesic_distance(m1, m2):
    """Rotation angle between two batches of rotation matrices (reference utils/losses.py:7-22)."""
    m = torch.bmm(m1, m2.transpose(1, 2))
    cos = (m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2
    cos = torch.min(cos, torch.ones_like(cos))
    cos = torch.max(cos, -torch.ones_like(cos))
    return torch.acos(cos)


def get_oob_error(pc, gt_box):
    """pc (B,N,3), gt_box (B,7) -> (B,) fp32: distinct rows of pc[b] outside the box over the distinct scalars among pc[b]'s coordinates
    (reference utils/losses.py:90-103, which loops over the objects on the host through open3d and Python sets).  One library call, no read: the
    out-of-box columns of sv_vc_metrics_objects with the Chamfer pass skipped."""
    from . import metrics
    return metrics.objects_table(pc, None, gt_box)[:, metrics.COL_OOB].contiguous()
