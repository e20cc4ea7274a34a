import torch
import torch.nn as nn
import torch.nn.functional as F


class FocalLoss(nn.Module):
    """The reference's FocalLoss (focal_sparse_conv/focal_sparse_utils.py:7-37): softmax over the class scores, clamp to [eps, 1 - eps], cross entropy
    weighted by (1 - p)^gamma, mean over ALL (row, class) elements.  A few values per voxel: torch ops."""

    def __init__(self, gamma=2.0, eps=1e-7):
        super().__init__()
        self.gamma = gamma
        self.eps = eps

    def forward(self, input, target):
        y = F.one_hot(target.long(), input.size(-1)).to(input.dtype)
        p = F.softmax(input, dim=-1).clamp(self.eps, 1. - self.eps)
        loss = -1 * y * torch.log(p)
        loss = loss * (1 - p) ** self.gamma
        return loss.mean()
