"""DDNLoss (reference ffn/ddn_loss/ddn_loss.py:15-75): softmax focal loss of the depth-bin logits against the binned depth map, balanced between
foreground and background.  kornia's FocalLoss(alpha, gamma, reduction="none") is restated (UNPINNED): -alpha * (1 - p_t)^gamma * log p_t with
log p from log_softmax over the bin axis.  The reference's self.device (torch.cuda.current_device() at construction) is dropped."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .balancer import Balancer
from .......utils import transform_utils
from .......utils.common_utils import tb_value


def softmax_focal_loss(logits, target, alpha, gamma):
    """logits (B, K, ...), target (B, ...) int64 in [0, K) -> (B, ...)"""
    log_pt = F.log_softmax(logits, dim=1).gather(1, target.unsqueeze(1)).squeeze(1)
    return -alpha * torch.pow(1.0 - log_pt.exp(), gamma) * log_pt


class DDNLoss(nn.Module):
    def __init__(self, weight, alpha, gamma, disc_cfg, fg_weight, bg_weight, downsample_factor):
        super().__init__()
        self.disc_cfg = dict(disc_cfg)
        self.balancer = Balancer(downsample_factor=downsample_factor, fg_weight=fg_weight, bg_weight=bg_weight)
        self.alpha = alpha
        self.gamma = gamma
        self.weight = weight

    def loss_func(self, depth_logits, depth_target):
        return softmax_focal_loss(depth_logits, depth_target, self.alpha, self.gamma)

    def forward(self, depth_logits, depth_maps, gt_boxes2d):
        """depth_logits (B, D + 1, H, W), depth_maps (B, H, W) [m], gt_boxes2d (B, N, 4) -> (loss, tb_dict)"""
        depth_target = transform_utils.bin_depths(depth_maps, **self.disc_cfg, target=True)
        loss = self.loss_func(depth_logits, depth_target)
        loss, tb_dict = self.balancer(loss=loss, gt_boxes2d=gt_boxes2d)
        loss = loss * self.weight
        tb_dict.update({"ddn_loss": tb_value(loss)})
        return loss, tb_dict
