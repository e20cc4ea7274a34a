"""Plain-torch restatement of the part of torchvision that CaDDN's depth distribution network uses: deeplabv3_resnet50 / deeplabv3_resnet101
(torchvision.models.segmentation: a Bottleneck ResNet whose layer3 / layer4 trade their stride for dilation, ASPP with rates 12 / 24 / 36, the
classifier, the optional FCN auxiliary head on layer3).  torchvision is not a dependency and its version is UNPINNED in the reference; the
architecture below is the one every torchvision release since 0.3 builds.  Parameter and buffer names equal torchvision's
(backbone.layer1.0.conv1.weight, classifier.0.convs.1.0.weight, classifier.0.project.0.weight, classifier.4.weight, aux_classifier.0.weight, ...),
so a torchvision checkpoint loads into it.  Nothing here fetches weights."""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)      # the stride sits on the 3x3
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


class ResNetBackbone(nn.Module):
    """conv1 .. layer4 of a Bottleneck ResNet (no avgpool / fc: IntermediateLayerGetter drops them), run up to the last layer in return_layers;
    `return_layers` maps a child's name to the key its output is returned under, and may be extended after construction as DDNTemplate does."""

    def __init__(self, layers, replace_stride_with_dilation=(False, True, True)):
        super().__init__()
        self.inplanes = 64
        self.dilation = 1
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2, dilate=replace_stride_with_dilation[0])
        self.layer3 = self._make_layer(256, layers[2], stride=2, dilate=replace_stride_with_dilation[1])
        self.layer4 = self._make_layer(512, layers[3], stride=2, dilate=replace_stride_with_dilation[2])
        self.return_layers = {'layer4': 'out'}
        for m in self.modules():                                           # torchvision's ResNet initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride=1, dilate=False):
        previous_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * Bottleneck.expansion, 1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * Bottleneck.expansion))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample, previous_dilation)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes, dilation=self.dilation) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x):
        out = OrderedDict()
        pending = set(self.return_layers)
        for name, module in self.named_children():
            x = module(x)
            if name in pending:
                out[self.return_layers[name]] = x
                pending.discard(name)
                if not pending:
                    break
        return out


class ASPPConv(nn.Sequential):
    def __init__(self, in_channels, out_channels, dilation):
        super().__init__(nn.Conv2d(in_channels, out_channels, 3, padding=dilation, dilation=dilation, bias=False), nn.BatchNorm2d(out_channels),
                         nn.ReLU())


class ASPPPooling(nn.Sequential):
    def __init__(self, in_channels, out_channels):
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU())

    def forward(self, x):
        size = x.shape[-2:]
        for mod in self:
            x = mod(x)
        return F.interpolate(x, size=size, mode='bilinear', align_corners=False)


class ASPP(nn.Module):
    def __init__(self, in_channels, atrous_rates, out_channels=256):
        super().__init__()
        modules = [nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU())]
        modules += [ASPPConv(in_channels, out_channels, rate) for rate in atrous_rates]
        modules.append(ASPPPooling(in_channels, out_channels))
        self.convs = nn.ModuleList(modules)
        self.project = nn.Sequential(nn.Conv2d(len(self.convs) * out_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(),
                                     nn.Dropout(0.5))

    def forward(self, x):
        return self.project(torch.cat([conv(x) for conv in self.convs], dim=1))


class DeepLabHead(nn.Sequential):
    def __init__(self, in_channels, num_classes):
        super().__init__(ASPP(in_channels, [12, 24, 36]), nn.Conv2d(256, 256, 3, padding=1, bias=False), nn.BatchNorm2d(256), nn.ReLU(),
                         nn.Conv2d(256, num_classes, 1))


class FCNHead(nn.Sequential):
    def __init__(self, in_channels, channels):
        inter = in_channels // 4
        super().__init__(nn.Conv2d(in_channels, inter, 3, padding=1, bias=False), nn.BatchNorm2d(inter), nn.ReLU(), nn.Dropout(0.1),
                         nn.Conv2d(inter, channels, 1))


class DeepLabV3(nn.Module):
    def __init__(self, backbone, classifier, aux_classifier=None):
        super().__init__()
        self.backbone = backbone
        self.classifier = classifier
        self.aux_classifier = aux_classifier

    def forward(self, x):
        size = x.shape[-2:]
        features = self.backbone(x)
        result = OrderedDict(out=F.interpolate(self.classifier(features["out"]), size=size, mode='bilinear', align_corners=False))
        if self.aux_classifier is not None:
            result["aux"] = F.interpolate(self.aux_classifier(features["aux"]), size=size, mode='bilinear', align_corners=False)
        return result


def _deeplabv3_resnet(layers, num_classes, aux_loss):
    backbone = ResNetBackbone(layers)
    if aux_loss:
        backbone.return_layers = {'layer3': 'aux', 'layer4': 'out'}
    return DeepLabV3(backbone, DeepLabHead(2048, num_classes), FCNHead(1024, num_classes) if aux_loss else None)


def deeplabv3_resnet50(pretrained=False, pretrained_backbone=False, num_classes=21, aux_loss=None, **kwargs):
    if pretrained or pretrained_backbone:
        raise ValueError("this project fetches nothing: load a checkpoint from a local pretrained_path")
    return _deeplabv3_resnet([3, 4, 6, 3], num_classes, aux_loss)


def deeplabv3_resnet101(pretrained=False, pretrained_backbone=False, num_classes=21, aux_loss=None, **kwargs):
    if pretrained or pretrained_backbone:
        raise ValueError("this project fetches nothing: load a checkpoint from a local pretrained_path")
    return _deeplabv3_resnet([3, 4, 23, 3], num_classes, aux_loss)
