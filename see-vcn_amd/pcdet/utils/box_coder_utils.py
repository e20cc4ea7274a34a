"""ResidualCoder with the reference's interface (detector3d/pcdet/utils/box_coder_utils.py:5-77)."""
import torch


class ResidualCoder(object):
    def __init__(self, code_size=7, encode_angle_by_sincos=False, **kwargs):
        super().__init__()
        self.code_size = code_size
        self.encode_angle_by_sincos = encode_angle_by_sincos
        if self.encode_angle_by_sincos:
            self.code_size += 1

    def encode_torch(self, boxes, anchors):
        """boxes (N,7+C) ground truth, anchors (N,7+C') -> residual targets (N, code_size); extras pair up like the reference's zip (the
        anchors of a sin/cos coder carry one zero column more than the boxes: anchor_ndim = code_size)"""
        a_dims = torch.clamp_min(anchors[:, 3:6], min=1e-5)
        g_dims = torch.clamp_min(boxes[:, 3:6], min=1e-5)
        diagonal = torch.sqrt(a_dims[:, 0:1] ** 2 + a_dims[:, 1:2] ** 2)
        xyz_t = torch.cat([(boxes[:, 0:1] - anchors[:, 0:1]) / diagonal, (boxes[:, 1:2] - anchors[:, 1:2]) / diagonal,
                           (boxes[:, 2:3] - anchors[:, 2:3]) / a_dims[:, 2:3]], dim=-1)
        dims_t = torch.log(g_dims / a_dims)
        rg, ra = boxes[:, 6:7], anchors[:, 6:7]
        rts = [torch.cos(rg) - torch.cos(ra), torch.sin(rg) - torch.sin(ra)] if self.encode_angle_by_sincos else [rg - ra]
        n_extra = min(boxes.shape[-1], anchors.shape[-1]) - 7
        extra = boxes[:, 7:7 + n_extra] - anchors[:, 7:7 + n_extra]
        return torch.cat([xyz_t, dims_t, *rts, extra], dim=-1)

    def decode_torch(self, box_encodings, anchors):
        """box_encodings (...,code_size+C), anchors (...,7+C) -> boxes (...,7+C)"""
        xa, ya, za, dxa, dya, dza, ra = (anchors[..., i:i + 1] for i in range(7))
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        xg = box_encodings[..., 0:1] * diagonal + xa
        yg = box_encodings[..., 1:2] * diagonal + ya
        zg = box_encodings[..., 2:3] * dza + za
        dxg = torch.exp(box_encodings[..., 3:4]) * dxa
        dyg = torch.exp(box_encodings[..., 4:5]) * dya
        dzg = torch.exp(box_encodings[..., 5:6]) * dza
        if self.encode_angle_by_sincos:
            rg = torch.atan2(box_encodings[..., 7:8] + torch.sin(ra), box_encodings[..., 6:7] + torch.cos(ra))
            cts = box_encodings[..., 8:]
        else:
            rg = box_encodings[..., 6:7] + ra
            cts = box_encodings[..., 7:]
        n_extra = min(cts.shape[-1], anchors.shape[-1] - 7)
        rest = cts[..., :n_extra] + anchors[..., 7:7 + n_extra]
        return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg, rest], dim=-1)


class PointResidualCoder(object):
    """Boxes coded against a point and (optionally) its class's mean size (reference box_coder_utils.py:144-222): 8 numbers
    [xt, yt, zt, dxt, dyt, dzt, cos, sin] + extras.  mean_size stays a CPU tensor and moves to the input's device on first use there (the
    reference calls .cuda() in the constructor); encode_torch clamps a copy of the sizes, never the caller's boxes."""

    def __init__(self, code_size=8, use_mean_size=True, **kwargs):
        super().__init__()
        self.code_size = code_size
        self.use_mean_size = use_mean_size
        if self.use_mean_size:
            self.mean_size = torch.tensor(kwargs['mean_size'], dtype=torch.float32)
            assert self.mean_size.min() > 0

    def _anchor_sizes(self, classes, like):
        """mean size rows (N, 3) of classes (N) in 1..num_classes, on like's device"""
        if self.mean_size.device != like.device:
            self.mean_size = self.mean_size.to(like.device)
        return self.mean_size[classes - 1]

    def encode_torch(self, gt_boxes, points, gt_classes=None):
        """gt_boxes (N, 7 + C), points (N, 3), gt_classes (N) in 1..num_classes -> (N, 8 + C)"""
        xyz, sizes, rg, extra = gt_boxes[:, 0:3], torch.clamp_min(gt_boxes[:, 3:6], min=1e-5), gt_boxes[:, 6:7], gt_boxes[:, 7:]
        if self.use_mean_size:
            anchor = self._anchor_sizes(gt_classes, gt_boxes)
            diagonal = torch.sqrt(anchor[:, 0:1] ** 2 + anchor[:, 1:2] ** 2)
            xyz_t = torch.cat([(xyz[:, 0:2] - points[:, 0:2]) / diagonal, (xyz[:, 2:3] - points[:, 2:3]) / anchor[:, 2:3]], dim=-1)
            sizes_t = torch.log(sizes / anchor)
        else:
            xyz_t = xyz - points
            sizes_t = torch.log(sizes)
        return torch.cat([xyz_t, sizes_t, torch.cos(rg), torch.sin(rg), extra], dim=-1)

    def decode_torch(self, box_encodings, points, pred_classes=None):
        """box_encodings (N, 8 + C), points (N, 3), pred_classes (N) in 1..num_classes -> boxes (N, 7 + C)"""
        xyz_t, sizes_t, cost, sint, extra = (box_encodings[..., 0:3], box_encodings[..., 3:6], box_encodings[..., 6:7], box_encodings[..., 7:8],
                                             box_encodings[..., 8:])
        if self.use_mean_size:
            anchor = self._anchor_sizes(pred_classes, box_encodings)
            diagonal = torch.sqrt(anchor[..., 0:1] ** 2 + anchor[..., 1:2] ** 2)
            xyz = torch.cat([xyz_t[..., 0:2] * diagonal + points[..., 0:2], xyz_t[..., 2:3] * anchor[..., 2:3] + points[..., 2:3]], dim=-1)
            sizes = torch.exp(sizes_t) * anchor
        else:
            xyz = xyz_t + points
            sizes = torch.exp(sizes_t)
        return torch.cat([xyz, sizes, torch.atan2(sint, cost), extra], dim=-1)
