import torch
import torch.nn as nn
import torch.nn.functional as F

from .....spconv import focal, modules, norm
from .....spconv import functional as Fsp
from ....ops.roiaware_pool3d.roiaware_pool3d_utils import points_in_boxes_gpu
from ....utils.spconv_utils import spconv
from .focal_sparse_utils import FocalLoss


class FocalSparseConv(spconv.SparseModule):
    """Drop-in for the reference's FocalSparseConv (backbones_3d/focal_sparse_conv/focal_sparse_conv.py:9-224) without the image branch: same
    constructor signature, attribute names (state_dict keys conv, bn1, conv_imp, conv_enlarge.{0,1}) and indice_keys, same order of operations --
    optional enlarge, conv_imp, expansion of the active set, conv under indice_key, bn1, ReLU.  The expansion (the reference's split_voxels /
    check_repeat / combine_out loops) is one autograd node over the sv_focal_* kernels (seevcn_amd/spconv/focal.py); it keys cells by the true
    linear key where the reference's key merges distinct voxels once one has y = 0 or x = 0, and lets a scene without voxels contribute
    nothing where the reference raises."""
    expansion = 1
    # conv_imp has 27 output channels, which only the VALU gather-GEMM takes; with the weight zero-padded to 32 output rows at launch time the planned MFMA
    # kernel runs it (the parameter keeps its shape, autograd slices the gradient back).  Measured at voxel_rcnn_car sizes (tools/focal_conv_micro.py,
    # profiles/focal_conv.txt): 0.02 / 0.09 / 0.14 ms padded against 0.33 / 6.9 / 12.7 ms on the VALU route at C = 16 / 32 / 64.  False: the VALU route (A/B).
    IMP_PAD32 = True

    def __init__(self, inplanes, planes, voxel_stride, norm_fn=None, indice_key=None,
                 image_channel=3, kernel_size=3, padding=1, mask_multi=False, use_img=False,
                 topk=False, threshold=0.5, skip_mask_kernel=False, enlarge_voxel_channels=-1,
                 point_cloud_range=[-3, -40, 0, 1, 40, 70.4],
                 voxel_size=[0.1, 0.05, 0.05]):
        super().__init__()
        if use_img:
            raise NotImplementedError("FocalSparseConv(use_img=True): the image branch (DeepLabV3 features sampled at the projected voxels, "
                                      "focal_sparse_conv.py:50-113) is the subclass FocalSparseConvMultimodal")
        if kernel_size != 3:
            raise NotImplementedError(f"FocalSparseConv(kernel_size={kernel_size}): the expansion gathers through the K = 27 submanifold table; no "
                                      f"config sets another kernel size")
        self.conv = spconv.SubMConv3d(inplanes, planes, kernel_size=kernel_size, stride=1, bias=False, indice_key=indice_key)
        self.bn1 = norm_fn(planes)
        self.relu = nn.ReLU(True)
        offset_channels = kernel_size ** 3
        self.topk = topk
        self.threshold = threshold
        self.voxel_stride = voxel_stride
        self.focal_loss = FocalLoss()
        self.mask_multi = mask_multi
        self.skip_mask_kernel = skip_mask_kernel
        self.use_img = use_img
        voxel_channel = enlarge_voxel_channels if enlarge_voxel_channels > 0 else inplanes
        self.conv_enlarge = spconv.SparseSequential(
            spconv.SubMConv3d(inplanes, enlarge_voxel_channels, kernel_size=3, stride=1, padding=1, bias=False, indice_key=indice_key + '_enlarge'),
            norm_fn(enlarge_voxel_channels),
            nn.ReLU(True)) if enlarge_voxel_channels > 0 else None
        self.conv_imp = spconv.SubMConv3d(voxel_channel, offset_channels, kernel_size=3, stride=1, padding=1, bias=False, indice_key=indice_key + '_imp')
        # z-first, as the reference keeps them (focal_sparse_conv.py:15-16, :47-48); plain attributes there, so no state_dict entry here either
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]

    def _importance(self, x_predict):
        """(imps (n, 27), the k = 3 submanifold table of these coordinates): conv_imp, on a table the tensor already carries for these very indices
        when there is one (conv_enlarge's, or the stage's 'subm1' / 'subm2' / 'subm3': same coordinates, 3x3x3 kernel, dilation 1 -- the same table)."""
        conv = self.conv_imp
        if x_predict.find_indice_pair(conv.indice_key) is None:
            for shared in list(x_predict.indice_dict.values()):
                if (getattr(shared, 'subm', False) and shared.ksize == conv.kernel_size and getattr(shared, 'dilation', None) == conv.dilation
                        and shared.in_indices is x_predict.indices):
                    x_predict.indice_dict[conv.indice_key] = shared
                    break
        rb = conv.get_rulebook(x_predict)
        w = conv.weight_kio()
        if self.IMP_PAD32:
            imps = Fsp.SparseConvFunction.apply(x_predict.features, F.pad(w, (0, 32 - w.shape[2])), rb)[:, :w.shape[2]]
        else:
            imps = Fsp.SparseConvFunction.apply(x_predict.features, w, rb)
        return imps, rb

    def _box_of_pts_loss(self, x, mask_voxel, batch_dict):
        """The training-only auxiliary loss (focal_sparse_conv.py:134-143, :162-167): voxel positions without a half-voxel shift against the ground-truth
        boxes, two-class focal loss on [1 - mv, mv].  Every scene's boxes are tested against all rows and the answer kept for its own: no per-scene
        boolean indexing, so no host read."""
        dev = x.features.device
        voxel_size = torch.tensor(self.voxel_size, dtype=torch.float32, device=dev)
        origin = torch.tensor(self.point_cloud_range[:3], dtype=torch.float32, device=dev)
        voxels_zyx = (x.indices[:, 1:] * self.voxel_stride) * voxel_size + origin
        xyz = voxels_zyx.flip(1).unsqueeze(0)
        scene = x.indices[:, 0]
        inside = torch.zeros_like(scene, dtype=torch.bool)
        gt_boxes = batch_dict['gt_boxes']
        for b in range(x.batch_size):
            hit = points_in_boxes_gpu(xyz, gt_boxes[b:b + 1, :, :-1])[0] >= 0
            inside |= hit & (scene == b)
        two = torch.stack([1 - mask_voxel, mask_voxel], dim=1)
        return self.focal_loss(two, inside.long())

    def _conv_bn_relu(self, x):
        if (modules.FUSE_CONV_BN and x.indices.shape[0] != 0 and self.conv.fusable_with(self.bn1, x)
                and not modules._hooked(self.conv, self.bn1, self.relu)):
            return self.conv.forward_bn_relu(x, self.bn1, True)
        out = self.conv(x)
        if out.indices.shape[0] == 0:
            return out
        if norm.fusable(self.bn1, out.features) and not modules._hooked(self.bn1, self.relu):
            return out.replace_feature(norm.batch_norm_relu(self.bn1, out.features, True))
        return out.replace_feature(self.relu(self.bn1(out.features)))

    def forward(self, x, batch_dict, x_rgb=None):
        x_predict = self.conv_enlarge(x) if self.conv_enlarge is not None else x
        imps_3d, rb = self._importance(x_predict)
        s = imps_3d.sigmoid()          # torch's sigmoid: the kernels decide >= / > on the very numbers autograd differentiates
        loss_box_of_pts = 0
        if self.training:
            loss_box_of_pts = self._box_of_pts_loss(x, s[:, -1], batch_dict)
        out, _, _ = focal.focal_expand(x, s, rb.nbr_out, topk=self.topk, threshold=self.threshold, mask_multi=self.mask_multi,
                                       skip_mask_kernel=self.skip_mask_kernel)
        out = self._conv_bn_relu(out)
        return out, batch_dict, loss_box_of_pts


class FocalSparseConvMultimodal(FocalSparseConv):
    """The reference's FocalSparseConv(use_img=True) (focal_sparse_conv.py:199-224): conv_imp reads [image features | voxel features] of the input
    set, and the image features of the EXPANDED set are added behind conv, in front of bn1.  Same constructor signature and state_dict keys
    (conv_imp.weight has image_channel + voxel_channel input channels).  construct_multimodal_features (:50-113) -- a per-scene loop with the
    projection on the host and a full-resolution F.interpolate in the reference -- is seevcn_amd/spconv/focal.py's focal_image_pixels /
    focal_image_fuse: per call site one launch for the pixels and one for the fused rows whatever the batch, no host read."""

    def __init__(self, inplanes, planes, voxel_stride, norm_fn=None, indice_key=None,
                 image_channel=3, kernel_size=3, padding=1, mask_multi=False, use_img=True,
                 topk=False, threshold=0.5, skip_mask_kernel=False, enlarge_voxel_channels=-1,
                 point_cloud_range=[-3, -40, 0, 1, 40, 70.4],
                 voxel_size=[0.1, 0.05, 0.05]):
        if enlarge_voxel_channels > 0:
            raise NotImplementedError("FocalSparseConvMultimodal(enlarge_voxel_channels > 0): the reference sizes conv_imp for the enlarged channels "
                                      "and feeds it the plain ones (focal_sparse_conv.py:32-33, :204); no config sets both")
        super().__init__(inplanes, planes, voxel_stride, norm_fn=norm_fn, indice_key=indice_key, image_channel=image_channel,
                         kernel_size=kernel_size, padding=padding, mask_multi=mask_multi, use_img=False, topk=topk, threshold=threshold,
                         skip_mask_kernel=skip_mask_kernel, enlarge_voxel_channels=enlarge_voxel_channels, point_cloud_range=point_cloud_range,
                         voxel_size=voxel_size)
        self.use_img = True
        self.image_channel = image_channel
        self.conv_imp = spconv.SubMConv3d(image_channel + inplanes, kernel_size ** 3, kernel_size=3, stride=1, padding=1, bias=False,
                                          indice_key=indice_key + '_imp')

    def _image_context(self, x, batch_dict, x_rgb):
        """What both call sites share: the channel-last image features, the per-scene tables (made once per batch and kept in batch_dict) and the
        image size.  One upload (the calibrations), no read."""
        from ....utils import calibration_kitti
        dev = x.features.device
        if 'focal_image_tables' not in batch_dict:
            batch_dict['focal_image_tables'] = (calibration_kitti.pack_calib(batch_dict['calib'], dev),
                                                focal.image_aug_table(batch_dict, x.batch_size, dev))
        calib_table, aug_table = batch_dict['focal_image_tables']
        return x_rgb.permute(0, 2, 3, 1).contiguous(), calib_table, aug_table, tuple(batch_dict['images'].shape[2:])

    def construct_multimodal_features(self, x, image_ctx, fuse_sum=False):
        """[image features | x.features] (n, C_img + C), or x.features + image features under fuse_sum (:50-113)"""
        features_nhwc, calib_table, aug_table, image_hw = image_ctx
        pix = focal.focal_image_pixels(x.indices, x.batch_size, self.voxel_stride, self.voxel_size, self.point_cloud_range[:3], calib_table,
                                       aug_table, image_hw)
        return focal.focal_image_fuse(x.features, features_nhwc, x.indices, pix, image_hw, fuse_sum)

    def forward(self, x, batch_dict, x_rgb=None):
        image_ctx = self._image_context(x, batch_dict, x_rgb)
        x_predict = x.replace_feature(self.construct_multimodal_features(x, image_ctx))
        imps_3d, rb = self._importance(x_predict)
        s = imps_3d.sigmoid()
        loss_box_of_pts = 0
        if self.training:
            loss_box_of_pts = self._box_of_pts_loss(x, s[:, -1], batch_dict)
        out, _, _ = focal.focal_expand(x, s, rb.nbr_out, topk=self.topk, threshold=self.threshold, mask_multi=self.mask_multi,
                                       skip_mask_kernel=self.skip_mask_kernel)
        out = self.conv(out)
        if out.indices.shape[0] == 0:
            return out, batch_dict, loss_box_of_pts
        fused = self.construct_multimodal_features(out, image_ctx, True)
        if norm.fusable(self.bn1, fused) and not modules._hooked(self.bn1, self.relu):
            return out.replace_feature(norm.batch_norm_relu(self.bn1, fused, True)), batch_dict, loss_box_of_pts
        return out.replace_feature(self.relu(self.bn1(fused))), batch_dict, loss_box_of_pts
