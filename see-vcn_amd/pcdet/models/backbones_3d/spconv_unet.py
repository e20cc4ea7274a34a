from functools import partial

import torch
import torch.nn as nn

from ....spconv import norm
from ...utils import common_utils
from ...utils.spconv_utils import replace_feature, spconv
from .spconv_backbone import post_act_block


class SparseBasicBlock(spconv.SparseModule):
    """The UNet's residual block (reference spconv_unet.py:11-46): two bias-free submanifold convolutions on one table, the identity added to
    the second one's normalised output.  (spconv_backbone.SparseBasicBlock is VoxelResBackBone8x's: its convolutions carry a bias.)"""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, indice_key=None, norm_fn=None):
        super().__init__()
        self.conv1 = spconv.SubMConv3d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False, indice_key=indice_key)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv3d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False, indice_key=indice_key)
        self.bn2 = norm_fn(planes)
        self.downsample = downsample
        self.stride = stride

    def _conv_bn(self, conv, bn, x, relu):
        if conv.fusable_with(bn, x) and not (conv._forward_hooks or conv._forward_pre_hooks or bn._forward_hooks or bn._forward_pre_hooks):
            return conv.forward_bn_relu(x, bn, relu)                  # conv -> BatchNorm1d (-> ReLU) as one autograd node
        out = conv(x)
        if norm.fusable(bn, out.features):
            return replace_feature(out, norm.batch_norm_relu(bn, out.features, relu))
        f = bn(out.features)
        return replace_feature(out, self.relu(f) if relu else f)

    def forward(self, x):
        identity = x.features
        assert x.features.dim() == 2, 'x.features.dim()=%d' % x.features.dim()
        out = self._conv_bn(self.conv1, self.bn1, x, True)
        out = self._conv_bn(self.conv2, self.bn2, out, False)
        if self.downsample is not None:
            identity = self.downsample(x)
        return replace_feature(out, self.relu(out.features + identity))


class UNetV2(nn.Module):
    """Drop-in for the reference's UNetV2 (backbones_3d/spconv_unet.py:49-212), the sparse UNet of Part-A2: same constructor keywords,
    submodule names (state_dict keys), indice_keys and batch_dict contract.  The encoder's tables come from ONE build_network_index call (one
    device -> host read); the decoder owns none: its submanifold layers reuse the encoder's keys and its three SparseInverseConv3d mirror the
    strided layers' tables.  The forward walks the module tree -- there is no launch-list or fp16 route for this backbone."""

    def __init__(self, model_cfg, input_channels, grid_size, voxel_size, point_cloud_range, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.sparse_shape = [int(g) for g in list(grid_size)[::-1]]
        self.sparse_shape[0] += 1                     # grid_size[::-1] + [1, 0, 0]  (spconv_unet.py:59)
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        self.conv_input = spconv.SparseSequential(
            spconv.SubMConv3d(input_channels, 16, 3, padding=1, bias=False, indice_key='subm1'), norm_fn(16), nn.ReLU())
        block = post_act_block
        self.conv1 = spconv.SparseSequential(block(16, 16, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'))
        self.conv2 = spconv.SparseSequential(
            block(16, 32, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv2', conv_type='spconv'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'),
            block(32, 32, 3, norm_fn=norm_fn, padding=1, indice_key='subm2'))
        self.conv3 = spconv.SparseSequential(
            block(32, 64, 3, norm_fn=norm_fn, stride=2, padding=1, indice_key='spconv3', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3'))
        self.conv4 = spconv.SparseSequential(
            block(64, 64, 3, norm_fn=norm_fn, stride=2, padding=(0, 1, 1), indice_key='spconv4', conv_type='spconv'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'),
            block(64, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4'))
        get = self.model_cfg.get if hasattr(self.model_cfg, 'get') else (lambda k, d=None: d)
        if get('RETURN_ENCODED_TENSOR', True):
            self.conv_out = spconv.SparseSequential(
                spconv.SparseConv3d(64, 128, (3, 1, 1), stride=(2, 1, 1), padding=get('last_pad', 0), bias=False, indice_key='spconv_down2'),
                norm_fn(128), nn.ReLU())
        else:
            self.conv_out = None
        # decoder: lateral block, merge, inverse convolution back to the finer level
        self.conv_up_t4 = SparseBasicBlock(64, 64, indice_key='subm4', norm_fn=norm_fn)
        self.conv_up_m4 = block(128, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm4')
        self.inv_conv4 = block(64, 64, 3, norm_fn=norm_fn, indice_key='spconv4', conv_type='inverseconv')
        self.conv_up_t3 = SparseBasicBlock(64, 64, indice_key='subm3', norm_fn=norm_fn)
        self.conv_up_m3 = block(128, 64, 3, norm_fn=norm_fn, padding=1, indice_key='subm3')
        self.inv_conv3 = block(64, 32, 3, norm_fn=norm_fn, indice_key='spconv3', conv_type='inverseconv')
        self.conv_up_t2 = SparseBasicBlock(32, 32, indice_key='subm2', norm_fn=norm_fn)
        self.conv_up_m2 = block(64, 32, 3, norm_fn=norm_fn, indice_key='subm2')
        self.inv_conv2 = block(32, 16, 3, norm_fn=norm_fn, indice_key='spconv2', conv_type='inverseconv')
        self.conv_up_t1 = SparseBasicBlock(16, 16, indice_key='subm1', norm_fn=norm_fn)
        self.conv_up_m1 = block(32, 16, 3, norm_fn=norm_fn, indice_key='subm1')
        self.conv5 = spconv.SparseSequential(block(16, 16, 3, norm_fn=norm_fn, padding=1, indice_key='subm1'))
        self.num_point_features = 16

    def _encoder(self):
        stages = [self.conv_input, self.conv1, self.conv2, self.conv3, self.conv4]
        return stages + [self.conv_out] if self.conv_out is not None else stages

    def UR_block_forward(self, x_lateral, x_bottom, conv_t, conv_m, conv_inv):
        x_trans = conv_t(x_lateral)
        x = replace_feature(x_trans, torch.cat((x_bottom.features, x_trans.features), dim=1))
        x_m = conv_m(x)
        x = self.channel_reduction(x, x_m.features.shape[1])
        x = replace_feature(x, x_m.features + x.features)
        return conv_inv(x)

    @staticmethod
    def channel_reduction(x, out_channels):
        """x.features (N, C1) -> (N, C2): the sum over the C1 / C2 consecutive channels of every output channel."""
        features = x.features
        n, in_channels = features.shape
        assert (in_channels % out_channels == 0) and (in_channels >= out_channels)
        return replace_feature(x, features.view(n, out_channels, -1).sum(dim=2))

    def forward(self, batch_dict):
        voxel_features, voxel_coords = batch_dict['voxel_features'], batch_dict['voxel_coords']
        input_sp_tensor = spconv.SparseConvTensor(features=voxel_features, indices=voxel_coords.int(), spatial_shape=self.sparse_shape,
                                                  batch_size=batch_dict['batch_size'], indice_dict=batch_dict.get('spconv_indice_dict'))
        # every table of the network (they are the encoder's) and its plans before the first layer runs, with one device -> host read
        spconv.prebuild_rulebooks(self._encoder(), input_sp_tensor, with_backward=self.training and torch.is_grad_enabled())
        spconv.refresh_weight_fragments(self)
        x = self.conv_input(input_sp_tensor)
        x_conv1 = self.conv1(x)
        x_conv2 = self.conv2(x_conv1)
        x_conv3 = self.conv3(x_conv2)
        x_conv4 = self.conv4(x_conv3)
        if self.conv_out is not None:
            batch_dict['encoded_spconv_tensor'] = self.conv_out(x_conv4)
            batch_dict['encoded_spconv_tensor_stride'] = 8
        x_up4 = self.UR_block_forward(x_conv4, x_conv4, self.conv_up_t4, self.conv_up_m4, self.inv_conv4)
        x_up3 = self.UR_block_forward(x_conv3, x_up4, self.conv_up_t3, self.conv_up_m3, self.inv_conv3)
        x_up2 = self.UR_block_forward(x_conv2, x_up3, self.conv_up_t2, self.conv_up_m2, self.inv_conv2)
        x_up1 = self.UR_block_forward(x_conv1, x_up2, self.conv_up_t1, self.conv_up_m1, self.conv5)
        batch_dict['point_features'] = x_up1.features
        point_coords = common_utils.get_voxel_centers(x_up1.indices[:, 1:], downsample_times=1, voxel_size=self.voxel_size,
                                                      point_cloud_range=self.point_cloud_range)
        batch_dict['point_coords'] = torch.cat((x_up1.indices[:, 0:1].float(), point_coords), dim=1)
        return batch_dict
