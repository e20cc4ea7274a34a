import os
from functools import partial

import torch.nn as nn

from ...utils import common_utils
from ...utils.spconv_utils import spconv
from .focal_sparse_conv import FocalSparseConv
from .focal_sparse_conv.focal_sparse_conv import FocalSparseConvMultimodal
from .focal_sparse_conv.SemanticSeg import PyramidFeat2D
from .spconv_backbone import post_act_block


class SparseSequentialBatchdict(spconv.SparseSequential):
    """SparseSequential whose FocalSparseConv members also take and return the batch_dict and add a loss (reference
    spconv_backbone_focal.py:23-37); its other members are sparse modules (the conv -> norm -> ReLU blocks, which fuse inside themselves)."""

    def forward(self, input, batch_dict=None):
        loss = 0
        for module in self._modules.values():
            if module is None:
                continue
            if isinstance(module, FocalSparseConv):
                input, batch_dict, _loss = module(input, batch_dict)
                loss = loss + _loss
            else:
                input = module(input)
        return input, batch_dict, loss


class VoxelBackBone8xFocal(nn.Module):
    """Drop-in for the reference VoxelBackBone8xFocal (backbones_3d/spconv_backbone_focal.py:101-269): same config keys (USE_IMG, IMG_PRETRAIN,
    TOPK, THRESHOLD, KERNEL_SIZE, MASK_MULTI, SKIP_MASK_KERNEL, SKIP_MASK_KERNEL_IMG, ENLARGE_VOXEL_CHANNELS, last_pad), submodule and indice_key
    names, backbone_channels, get_loss and batch_dict outputs.  USE_IMG: True builds `semseg` (DeepLabV3 layer1 features reduced to 16 channels)
    and `conv_focal_multimodal`, run between conv1 and conv2 on batch_dict['images'] and batch_dict['calib'].  IMG_PRETRAIN: None initialises the
    image network at random and does not normalise; an existing file is loaded; a path that does not exist is refused -- the reference would
    download the checkpoint, and downloading is not built.  It walks its module tree: the launch-list chains and EVAL_DTYPE of VoxelBackBone8x
    do not apply to this class."""

    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        cfg = model_cfg.get if hasattr(model_cfg, 'get') else (lambda key, default=None: default)
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        self.sparse_shape = [int(g) for g in list(grid_size)[::-1]]
        self.sparse_shape[0] += 1                     # grid_size[::-1] + [1, 0, 0]  (spconv_backbone_focal.py:108)
        self.conv_input = spconv.SparseSequential(
            spconv.SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key='subm1'), norm_fn(16), nn.ReLU())
        block = post_act_block
        use_img = cfg('USE_IMG', False)
        topk = cfg('TOPK', True)
        threshold = cfg('THRESHOLD', 0.5)
        kernel_size = cfg('KERNEL_SIZE', 3)
        mask_multi = cfg('MASK_MULTI', False)
        skip_mask_kernel = cfg('SKIP_MASK_KERNEL', False)
        enlarge_voxel_channels = cfg('ENLARGE_VOXEL_CHANNELS', -1)
        if use_img:
            img_pretrain = cfg('IMG_PRETRAIN', "../checkpoints/deeplabv3_resnet50_coco-cd0a2569.pth")
            if img_pretrain is not None and not os.path.exists(img_pretrain):
                raise NotImplementedError(f"VoxelBackBone8xFocal(USE_IMG=True): the DeepLabV3 checkpoint IMG_PRETRAIN={img_pretrain!r} does not exist; "
                                          f"the reference would download it (sem_deeplabv3.py:59-65) and downloading is not built.  Point "
                                          f"IMG_PRETRAIN at a local file, or set it to None for a randomly initialised image network")
            image_channel = 16
            seg_cfg = dict(name='SemDeepLabV3', backbone='ResNet50', num_class=21,            # spconv_backbone_focal.py:129-142
                           args={"feat_extract_layer": ["layer1"], "pretrained_path": img_pretrain},
                           channel_reduce={"in_channels": [256], "out_channels": [image_channel], "kernel_size": [1], "stride": [1], "bias": [False]})
            self.semseg = PyramidFeat2D(optimize=True, model_cfg=seg_cfg)
            self.conv_focal_multimodal = FocalSparseConvMultimodal(16, 16, image_channel=image_channel, topk=topk, threshold=threshold,
                                                                   skip_mask_kernel=cfg('SKIP_MASK_KERNEL_IMG', False), voxel_stride=1,
                                                                   norm_fn=norm_fn, indice_key='spconv_focal_multimodal')
        special_spconv_fn = partial(FocalSparseConv, mask_multi=mask_multi, enlarge_voxel_channels=enlarge_voxel_channels, topk=topk,
                                    threshold=threshold, kernel_size=kernel_size, padding=kernel_size // 2, skip_mask_kernel=skip_mask_kernel)
        self.use_img = use_img
        self.conv1 = SparseSequentialBatchdict(
            block(16, 16, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'),
            special_spconv_fn(16, 16, voxel_stride=1, norm_fn=norm_fn, indice_key='focal1'))
        self.conv2 = SparseSequentialBatchdict(
            block(16, 32, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv2', conv_type='spconv'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'),
            special_spconv_fn(32, 32, voxel_stride=2, norm_fn=norm_fn, indice_key='focal2'))
        self.conv3 = SparseSequentialBatchdict(
            block(32, 64, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv3', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'),
            special_spconv_fn(64, 64, voxel_stride=4, norm_fn=norm_fn, indice_key='focal3'))
        self.conv4 = SparseSequentialBatchdict(
            block(64, 64, 3, norm_fn=norm_fn, stride=2, padding=(0, 1, 1), indice_key='spconv4', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'))
        last_pad = cfg('last_pad', 0)
        self.conv_out = spconv.SparseSequential(
            spconv.SparseConv3d(64, 128, (3, 1, 1), stride=(2, 1, 1), padding=last_pad, bias=False, indice_key='spconv_down2'),
            norm_fn(128), nn.ReLU())
        self.num_point_features = 128
        self.backbone_channels = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}
        self.forward_ret_dict = {}

    def get_loss(self, tb_dict=None):
        loss = self.forward_ret_dict['loss_box_of_pts']
        if tb_dict is None:
            tb_dict = {}
        tb_dict['loss_box_of_pts'] = common_utils.tb_value(loss)
        return loss, tb_dict

    def forward(self, batch_dict):
        voxel_features, voxel_coords = batch_dict['voxel_features'], batch_dict['voxel_coords']
        input_sp_tensor = spconv.SparseConvTensor(features=voxel_features, indices=voxel_coords.int(), spatial_shape=self.sparse_shape,
                                                  batch_size=batch_dict['batch_size'])
        x = self.conv_input(input_sp_tensor)
        x_conv1, batch_dict, loss1 = self.conv1(x, batch_dict)
        loss_img = 0
        if self.use_img:
            x_image = self.semseg(batch_dict['images'])['layer1_feat2d']
            x_conv1, batch_dict, loss_img = self.conv_focal_multimodal(x_conv1, batch_dict, x_image)
        x_conv2, batch_dict, loss2 = self.conv2(x_conv1, batch_dict)
        x_conv3, batch_dict, loss3 = self.conv3(x_conv2, batch_dict)
        x_conv4, batch_dict, loss4 = self.conv4(x_conv3, batch_dict)
        self.forward_ret_dict['loss_box_of_pts'] = loss1 + loss2 + loss3 + loss4 + loss_img
        out = self.conv_out(x_conv4)
        batch_dict.update({'encoded_spconv_tensor': out, 'encoded_spconv_tensor_stride': 8})
        batch_dict.update({'multi_scale_3d_features': {'x_conv1': x_conv1, 'x_conv2': x_conv2, 'x_conv3': x_conv3, 'x_conv4': x_conv4}})
        batch_dict.update({'multi_scale_3d_strides': {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}})
        return batch_dict
