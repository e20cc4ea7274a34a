"""DDNTemplate (reference ffn/ddn/ddn_template.py:16-162): the depth distribution network around a segmentation model -- image features from
`feat_extract_layer`, depth-bin logits from the classifier resized to the features' grid.  kornia's normalize is restated (UNPINNED:
(x - mean) / std per channel).  The reference downloads a checkpoint that is missing; this project fetches nothing, so a pretrained_path that
does not exist raises FileNotFoundError."""
from collections import OrderedDict
from pathlib import Path

import torch
import torch.nn as nn
import torch.nn.functional as F


class DDNTemplate(nn.Module):
    def __init__(self, constructor, feat_extract_layer, num_classes, pretrained_path=None, aux_loss=None):
        super().__init__()
        self.num_classes = num_classes
        self.pretrained_path = pretrained_path
        self.pretrained = pretrained_path is not None
        self.aux_loss = aux_loss
        if self.pretrained:
            self.norm_mean = torch.Tensor([0.485, 0.456, 0.406])          # ImageNet statistics, as the pretrained ResNet expects
            self.norm_std = torch.Tensor([0.229, 0.224, 0.225])
        self.model = self.get_model(constructor=constructor)
        self.feat_extract_layer = feat_extract_layer
        self.model.backbone.return_layers = {feat_extract_layer: 'features', **self.model.backbone.return_layers}

    def get_model(self, constructor):
        model = constructor(pretrained=False, pretrained_backbone=False, num_classes=self.num_classes, aux_loss=self.aux_loss)
        if self.pretrained_path is not None:
            checkpoint_path = Path(self.pretrained_path)
            if not checkpoint_path.exists():
                raise FileNotFoundError(f"DDN checkpoint {checkpoint_path} does not exist (nothing is downloaded)")
            model_dict = model.state_dict()
            pretrained_dict = torch.load(str(checkpoint_path), map_location="cpu")
            model_dict.update(self.filter_pretrained_dict(model_dict=model_dict, pretrained_dict=pretrained_dict))
            model.load_state_dict(model_dict)
        return model

    def filter_pretrained_dict(self, model_dict, pretrained_dict):
        """drops what the model does not have (the auxiliary classifier) or has in another size (the last convolution when the class count differs)"""
        if "aux_classifier.0.weight" in pretrained_dict and "aux_classifier.0.weight" not in model_dict:
            pretrained_dict = {key: value for key, value in pretrained_dict.items() if "aux_classifier" not in key}
        if model_dict["classifier.4.weight"].shape[0] != pretrained_dict["classifier.4.weight"].shape[0]:
            pretrained_dict.pop("classifier.4.weight")
            pretrained_dict.pop("classifier.4.bias")
        return pretrained_dict

    def forward(self, images):
        """images (N, 3, H_in, W_in) -> features (N, C, H_out, W_out), logits (N, num_classes, H_out, W_out) [, aux]"""
        x = self.preprocess(images)
        result = OrderedDict()
        features = self.model.backbone(x)
        result['features'] = features['features']
        feat_shape = features['features'].shape[-2:]
        result["logits"] = F.interpolate(self.model.classifier(features["out"]), size=feat_shape, mode='bilinear', align_corners=False)
        if self.model.aux_classifier is not None:
            result["aux"] = F.interpolate(self.model.aux_classifier(features["aux"]), size=feat_shape, mode='bilinear', align_corners=False)
        return result

    def preprocess(self, images):
        """ImageNet normalisation for a pretrained backbone; the padded pixels (exact zeros) are zero again afterwards"""
        x = images
        if self.pretrained:
            mask = (x == 0)
            mean = self.norm_mean.to(x.device, x.dtype).view(1, -1, 1, 1)
            std = self.norm_std.to(x.device, x.dtype).view(1, -1, 1, 1)
            x = ((x - mean) / std).masked_fill(mask, 0)
        return x
