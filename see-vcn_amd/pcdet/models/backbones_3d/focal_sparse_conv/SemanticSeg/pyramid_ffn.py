"""PyramidFeat2D (reference focal_sparse_conv/SemanticSeg/pyramid_ffn.py:6-77): SemDeepLabV3 features of the requested layers, each through a
channel-reducing BasicBlock2D.  state_dict keys ifn.model.backbone.*, reduce_blocks.<i>.{conv,bn}.* as in the reference.  model_cfg: a dict or an
object with num_class, backbone, args (feat_extract_layer, pretrained_path) and channel_reduce."""
import torch.nn as nn

from ....model_utils.basic_block_2d import BasicBlock2D
from .sem_deeplabv3 import SemDeepLabV3


class PyramidFeat2D(nn.Module):
    def __init__(self, optimize, model_cfg):
        super().__init__()
        self.model_cfg = model_cfg
        self.is_optimize = optimize
        cfg = model_cfg.__getitem__ if isinstance(model_cfg, dict) else (lambda key: getattr(model_cfg, key))
        args, reduce = cfg('args'), cfg('channel_reduce')
        self.feat_extract_layer = list(args['feat_extract_layer'])
        self.ifn = SemDeepLabV3(num_classes=cfg('num_class'), backbone_name=cfg('backbone'), **args)
        self.reduce_blocks = nn.ModuleList()
        self.out_channels = {}
        for idx, channel in enumerate(reduce["in_channels"]):
            channel_out = reduce["out_channels"][idx]
            self.out_channels[self.feat_extract_layer[idx]] = channel_out
            self.reduce_blocks.append(BasicBlock2D(in_channels=channel, out_channels=channel_out, kernel_size=reduce["kernel_size"][idx],
                                                   stride=reduce["stride"][idx], bias=reduce["bias"][idx]))

    def get_output_feature_dim(self):
        return self.out_channels

    def forward(self, images):
        """images (N, 3, H_in, W_in) -> {'<layer>_feat2d': (N, C_out, H_out, W_out)}"""
        out = {}
        ifn_result = self.ifn(images)
        for idx, layer in enumerate(self.feat_extract_layer):
            image_features = self.reduce_blocks[idx](ifn_result[layer])
            if self.training and not self.is_optimize:                   # :60-65: cut from the graph unless the image network is trained
                image_features = image_features.detach()
            out[layer + "_feat2d"] = image_features
        return out

    def get_loss(self):
        return None, None
