"""ImageVFE (reference backbones_3d/vfe/image_vfe.py:7-85): CaDDN's image branch -- the frustum feature network (ffn) estimates a depth
distribution per pixel, the frustum-to-voxel transformation (f2v) samples image features * depth probabilities into the voxel grid."""
from .image_vfe_modules import f2v, ffn
from .vfe_template import VFETemplate
from ....utils.common_utils import cfg_get


class ImageVFE(VFETemplate):
    def __init__(self, model_cfg, grid_size, point_cloud_range, depth_downsample_factor, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.grid_size = grid_size
        self.pc_range = point_cloud_range
        self.downsample_factor = depth_downsample_factor
        self.module_topology = ['ffn', 'f2v']
        self.build_modules()

    def build_modules(self):
        for module_name in self.module_topology:
            self.add_module(module_name, getattr(self, 'build_%s' % module_name)())

    def build_ffn(self):
        cfg = cfg_get(self.model_cfg, 'FFN')
        ffn_module = ffn.__all__[cfg_get(cfg, 'NAME')](model_cfg=cfg, downsample_factor=self.downsample_factor)
        self.disc_cfg = ffn_module.disc_cfg
        return ffn_module

    def build_f2v(self):
        cfg = cfg_get(self.model_cfg, 'F2V')
        return f2v.__all__[cfg_get(cfg, 'NAME')](model_cfg=cfg, grid_size=self.grid_size, pc_range=self.pc_range, disc_cfg=self.disc_cfg)

    def get_output_feature_dim(self):
        return self.ffn.get_output_feature_dim()

    def forward(self, batch_dict, **kwargs):
        """images (N, 3, H_in, W_in) -> voxel_features (B, C, Z, Y, X)"""
        self.ffn.fused = bool(getattr(self.f2v, 'fused', False))           # the fused sampling needs no frustum volume
        batch_dict = self.ffn(batch_dict)
        batch_dict = self.f2v(batch_dict)
        return batch_dict

    def get_loss(self):
        """(loss, tb_dict) of the depth distribution network"""
        return self.ffn.get_loss()
