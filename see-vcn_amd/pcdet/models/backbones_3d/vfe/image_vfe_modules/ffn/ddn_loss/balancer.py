"""Balancer (reference ffn/ddn_loss/balancer.py:7-50): fixed foreground / background weighting of the pixel-wise depth loss."""
import torch
import torch.nn as nn

from .......utils import loss_utils
from .......utils.common_utils import tb_value


class Balancer(nn.Module):
    def __init__(self, fg_weight, bg_weight, downsample_factor=1):
        super().__init__()
        self.fg_weight = fg_weight
        self.bg_weight = bg_weight
        self.downsample_factor = downsample_factor

    def forward(self, loss, gt_boxes2d):
        """loss (B, H, W), gt_boxes2d (B, N, 4) -> (scalar loss, tb_dict).  The masked sums are taken with where() instead of boolean indexing:
        the same terms, no host read for the number of selected pixels."""
        fg_mask = loss_utils.compute_fg_mask(gt_boxes2d=gt_boxes2d, shape=loss.shape, downsample_factor=self.downsample_factor, device=loss.device)
        bg_mask = ~fg_mask
        weights = self.fg_weight * fg_mask + self.bg_weight * bg_mask
        num_pixels = fg_mask.numel()                                       # fg_mask.sum() + bg_mask.sum()
        loss = loss * weights
        zero = torch.zeros((), dtype=loss.dtype, device=loss.device)
        fg_loss = torch.where(fg_mask, loss, zero).sum() / num_pixels
        bg_loss = torch.where(bg_mask, loss, zero).sum() / num_pixels
        loss = fg_loss + bg_loss
        tb_dict = {"balancer_loss": tb_value(loss), "fg_loss": tb_value(fg_loss), "bg_loss": tb_value(bg_loss)}
        return loss, tb_dict
