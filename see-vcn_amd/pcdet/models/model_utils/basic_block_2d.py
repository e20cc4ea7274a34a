"""BasicBlock2D (reference model_utils/basic_block_2d.py:4-34): Conv2d -> BatchNorm2d -> ReLU; the keywords go to nn.Conv2d."""
import torch.nn as nn


class BasicBlock2D(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, features):
        """(B, C_in, H, W) -> (B, C_out, H, W)"""
        return self.relu(self.bn(self.conv(features)))
