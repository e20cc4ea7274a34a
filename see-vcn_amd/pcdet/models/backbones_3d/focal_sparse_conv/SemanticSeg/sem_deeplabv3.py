"""SegTemplate / SemDeepLabV3 (reference focal_sparse_conv/SemanticSeg/sem_deeplabv3.py:11-160) on the plain-torch DeepLabV3 restatement that came
with CaDDN (vfe/image_vfe_modules/ffn/ddn/deeplabv3.py): image features of the layers in `feat_extract_layer`.  The attribute names are the
reference's, so a checkpoint's `model.backbone.*` keys load.  The reference's forward returns right after the backbone (:119-122); here the ResNet
stops at the last requested layer -- the outputs are the same, and the stages that are not run keep their parameters.  The reference downloads a
checkpoint that is missing (:59-65); this project fetches nothing, so a pretrained_path that does not exist raises FileNotFoundError."""
from collections import OrderedDict
from pathlib import Path

import torch
import torch.nn as nn

from ...vfe.image_vfe_modules.ffn.ddn import deeplabv3


class SegTemplate(nn.Module):
    def __init__(self, constructor, feat_extract_layer, num_classes, pretrained_path=None, aux_loss=None):
        super().__init__()
        self.num_classes = num_classes
        self.pretrained_path = pretrained_path
        self.pretrained = pretrained_path is not None
        self.aux_loss = aux_loss
        if self.pretrained:                                              # normalised only for a pretrained backbone, as the reference (:28-31, :113-114)
            self.norm_mean = torch.Tensor([0.485, 0.456, 0.406])
            self.norm_std = torch.Tensor([0.229, 0.224, 0.225])
        self.model = self.get_model(constructor=constructor)
        self.feat_extract_layer = list(feat_extract_layer)
        self.model.backbone.return_layers = {layer: layer for layer in self.feat_extract_layer}

    def get_model(self, constructor):
        model = constructor(pretrained=False, pretrained_backbone=False, num_classes=self.num_classes, aux_loss=self.aux_loss)
        if self.pretrained_path is not None:
            checkpoint_path = Path(self.pretrained_path)
            if not checkpoint_path.exists():
                raise FileNotFoundError(f"DeepLabV3 checkpoint {checkpoint_path} does not exist (nothing is downloaded)")
            model_dict = model.state_dict()
            model_dict.update(torch.load(str(checkpoint_path), map_location="cpu"))
            model.load_state_dict(model_dict, strict=False)               # :72-73: keys the model lacks (the auxiliary classifier) are ignored
        return model

    def forward(self, images):
        """images (N, 3, H_in, W_in) -> {layer: (N, C, H_out, W_out)} for every layer in feat_extract_layer"""
        if self.pretrained:
            images = (images - self.norm_mean[None, :, None, None].to(images.device, images.dtype)) \
                / self.norm_std[None, :, None, None].to(images.device, images.dtype)
        features = self.model.backbone(images)
        return OrderedDict((layer, features[layer]) for layer in self.feat_extract_layer)


class SemDeepLabV3(SegTemplate):
    def __init__(self, backbone_name, **kwargs):
        if backbone_name == "ResNet50":
            constructor = deeplabv3.deeplabv3_resnet50
        elif backbone_name == "ResNet101":
            constructor = deeplabv3.deeplabv3_resnet101
        else:
            raise NotImplementedError(f"SemDeepLabV3: backbone {backbone_name}")
        super().__init__(constructor=constructor, **kwargs)
