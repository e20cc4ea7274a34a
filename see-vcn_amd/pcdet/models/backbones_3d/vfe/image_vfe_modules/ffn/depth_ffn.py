"""DepthFFN (reference ffn/depth_ffn.py:8-103): depth distribution network -> channel reduction -> the image's depth-feature volume.  On the fused
route (`self.fused`, which ImageVFE sets from its FrustumToVoxel) the volume is not built: image_features and depth_probs = softmax(depth_logits)
with all D + 1 bins go into batch_dict, both channels_last so that the sampling kernel reads them as they lie.  create_frustum_features stays a
method for the module-tree route."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ddn, ddn_loss
from .....model_utils.basic_block_2d import BasicBlock2D
from ......utils.common_utils import cfg_get


class DepthFFN(nn.Module):
    def __init__(self, model_cfg, downsample_factor):
        super().__init__()
        self.model_cfg = model_cfg
        self.disc_cfg = dict(cfg_get(model_cfg, 'DISCRETIZE'))
        self.downsample_factor = downsample_factor
        ddn_cfg, loss_cfg = cfg_get(model_cfg, 'DDN'), cfg_get(model_cfg, 'LOSS')
        self.ddn = ddn.__all__[cfg_get(ddn_cfg, 'NAME')](num_classes=self.disc_cfg["num_bins"] + 1, backbone_name=cfg_get(ddn_cfg, 'BACKBONE_NAME'),
                                                        **dict(cfg_get(ddn_cfg, 'ARGS')))
        self.channel_reduce = BasicBlock2D(**dict(cfg_get(model_cfg, 'CHANNEL_REDUCE')))
        self.ddn_loss = ddn_loss.__all__[cfg_get(loss_cfg, 'NAME')](disc_cfg=self.disc_cfg, downsample_factor=downsample_factor,
                                                                    **dict(cfg_get(loss_cfg, 'ARGS')))
        self.forward_ret_dict = {}
        self.fused = False

    def get_output_feature_dim(self):
        return self.channel_reduce.out_channels

    def forward(self, batch_dict):
        """images (N, 3, H_in, W_in) -> frustum_features (N, C, D, H_out, W_out), or on the fused route image_features (N, C, H_out, W_out) and
        depth_probs (N, D + 1, H_out, W_out)"""
        ddn_result = self.ddn(batch_dict["images"])
        image_features = ddn_result["features"]
        depth_logits = ddn_result["logits"]
        if self.channel_reduce is not None:
            image_features = self.channel_reduce(image_features)
        if self.fused:
            batch_dict["image_features"] = image_features.contiguous(memory_format=torch.channels_last)
            batch_dict["depth_probs"] = F.softmax(depth_logits.contiguous(memory_format=torch.channels_last), dim=1)
        else:
            batch_dict["frustum_features"] = self.create_frustum_features(image_features=image_features, depth_logits=depth_logits)
        if self.training:
            self.forward_ret_dict["depth_maps"] = batch_dict["depth_maps"]
            self.forward_ret_dict["gt_boxes2d"] = batch_dict["gt_boxes2d"]
            self.forward_ret_dict["depth_logits"] = depth_logits
        return batch_dict

    def create_frustum_features(self, image_features, depth_logits):
        """image_features (N, C, H, W), depth_logits (N, D + 1, H, W) -> (N, C, D, H, W): softmax over the bins, the last bin (beyond the maximum
        range) dropped, times the features"""
        depth_probs = F.softmax(depth_logits.unsqueeze(1), dim=2)[:, :, :-1]
        return depth_probs * image_features.unsqueeze(2)

    def get_loss(self):
        """(loss, tb_dict) of the depth distribution network"""
        return self.ddn_loss(**self.forward_ret_dict)
