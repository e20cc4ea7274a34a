import os

import torch
import torch.nn as nn

from ..... import _lib
from ....ops.pointnet2.pointnet2_stack import pointnet2_modules as pointnet2_stack_modules
from ....ops.pointnet2.pointnet2_stack import pointnet2_utils as pointnet2_stack_utils
from ....utils import common_utils
from ....utils.common_utils import cfg_get

# 1: a channels_last fp32 map is read, and its gradient written, in place by the channel-last entries.  Opt-in until the route has been run and timed on
# a GPU ("BEV keypoint features on the channels_last map"); 0 / unset: the map is copied to NCHW and back around the NCHW entries.
BEV_INTERP_NHWC = os.environ.get("SEEVCN_BEV_INTERP_NHWC", "0") == "1"


class _BevInterp(torch.autograd.Function):
    """Bilinear BEV features at the keypoints.  With BEV_INTERP_NHWC a channels_last fp32 map (what HeightCompression hands a BaseBEVBackbone from 8
    scenes on) is read and its gradient written in that layout by the library's channel-last entries: no copy of the map either way, and a gradient
    whose summation order is fixed.  Every other map takes the NCHW entries -- except that under the order-fixed gradient switch
    (ordered.ordered_gradients()) its gradient, too, is summed by the channel-last entry and copied to NCHW: the NCHW gradient entry adds with float
    atomics.  last_bev_layout names the FORWARD entries."""

    @staticmethod
    def forward(ctx, bev, keypoints, x0, y0, vx, vy, stride):
        kp = keypoints.contiguous().float()
        B, C, H, W = bev.shape
        ctx.nhwc = (BEV_INTERP_NHWC and bev.dtype == torch.float32 and bev.is_contiguous(memory_format=torch.channels_last)
                    and not bev.is_contiguous())
        VoxelSetAbstraction.last_bev_layout = 'nhwc' if ctx.nhwc else 'nchw'
        out = torch.empty((kp.shape[0], C), dtype=torch.float32, device=bev.device)
        if ctx.nhwc:
            _lib.launch("sv_bev_interpolate_nhwc", _lib.ptr(kp), kp.shape[0], _lib.ptr(bev.permute(0, 2, 3, 1)), B, C, H, W, x0, y0, vx, vy, float(stride),
                        _lib.ptr(out))
        else:
            bev = bev.contiguous().float()
            _lib.launch("sv_bev_interpolate", _lib.ptr(kp), kp.shape[0], _lib.ptr(bev), B, C, H, W, x0, y0, vx, vy, float(stride), _lib.ptr(out))
        ctx.save_for_backward(kp)
        ctx.meta = (B, C, H, W, x0, y0, vx, vy, float(stride))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        (kp,) = ctx.saved_tensors
        B, C, H, W, x0, y0, vx, vy, stride = ctx.meta
        g = grad_out.contiguous().float()
        from ..... import ordered
        if ctx.nhwc or ordered.ordered_gradients():           # the channel-last entry sums in a fixed order; the NCHW entry adds with float atomics
            gbev = torch.empty((B, H, W, C), dtype=torch.float32, device=g.device)
            scratch = _lib.workspace.scratch("bev_interp_grad_nhwc", lib.sv_bev_interpolate_grad_nhwc_scratch_bytes(kp.shape[0], B, H, W), g.device)
            _lib.launch("sv_bev_interpolate_grad_nhwc", _lib.ptr(kp), kp.shape[0], _lib.ptr(g), B, C, H, W, x0, y0, vx, vy, stride, _lib.ptr(scratch),
                        _lib.ptr(gbev))
            gbev = gbev.permute(0, 3, 1, 2)                                          # (B, C, H, W) with channels_last strides
            return (gbev if ctx.nhwc else gbev.contiguous()), None, None, None, None, None, None
        gbev = torch.empty((B, C, H, W), dtype=torch.float32, device=g.device)
        scratch = _lib.workspace.scratch("bev_interp_grad", lib.sv_bev_interpolate_grad_scratch_bytes(B, C, H, W), g.device)
        _lib.launch("sv_bev_interpolate_grad", _lib.ptr(kp), kp.shape[0], _lib.ptr(g), B, C, H, W, x0, y0, vx, vy, stride, _lib.ptr(scratch), _lib.ptr(gbev))
        return gbev, None, None, None, None, None, None


def _one_scene_cnt(points):
    return torch.full((1,), points.shape[0], dtype=torch.int32, device=points.device)


def sample_points_with_roi(rois, points, sample_radius_with_roi, num_max_points_of_part=200000):
    """rois (M, 7 + C), points (N, 3) of one scene -> (sampled_points (N_out, 3), point_mask (N,) bool), reference :45-75.  One sv_spc_select launch
    in mask mode; num_max_points_of_part is accepted and ignored (the chunking of the reference's distance matrix does not change its result)."""
    xyz = points[:, 0:3].contiguous().float()
    sector = pointnet2_stack_utils.pointnet2.spc_select(xyz, _one_scene_cnt(xyz), rois.unsqueeze(0), sample_radius_with_roi, 0, xyz.shape[0])
    point_mask = sector >= 0
    sampled_points = points[point_mask, :]
    if sampled_points.shape[0] == 0:
        sampled_points = points[:1]
    return sampled_points, point_mask


def sector_fps(points, num_sampled_points, num_sectors):
    """points (N, 3) of one scene -> (N_out, 3): farthest point sampling per azimuth sector with quotas by share, reference :78-121.  Three launches
    (every point passes the selection: one RoI of infinite radius) and one read, the number of samples."""
    ops = pointnet2_stack_utils.pointnet2
    xyz = points[:, 0:3].contiguous().float()
    cnt = _one_scene_cnt(xyz)
    everything = torch.zeros((1, 1, 7), dtype=torch.float32, device=xyz.device)
    sector = ops.spc_select(xyz, cnt, everything, float('inf'), num_sectors, xyz.shape[0])
    rows, _ = _spc_rows(xyz, cnt, sector, num_sampled_points, num_sectors, xyz.shape[0])
    return points[rows.long()]


def _spc_rows(xyz, cnt, sector, num_keypoints, num_sectors, max_n):
    """partition + ragged FPS + the one read: -> (keypoint rows of all scenes (sum kp,) int32, kp_cnt (B,) int32 on the device)"""
    ops = pointnet2_stack_utils.pointnet2
    B, stride = cnt.shape[0], num_keypoints + num_sectors
    order, tables = ops.spc_partition(sector, xyz, cnt, num_keypoints, num_sectors)
    idx = torch.empty((B * stride,), dtype=torch.int32, device=xyz.device)      # a scene's quotas sum to at most K + S
    ops.stack_farthest_point_sampling_ragged(xyz, order, tables[0], tables[1], tables[2], tables[3], idx, max_n)
    kp_cnt = tables[4][:B]
    kp = _lib.host_ints([kp_cnt])
    return torch.cat([idx[b * stride:b * stride + k] for b, k in enumerate(kp)]), kp_cnt


def _selected_rows(xyz, cnt, rois, radius):
    """The rows of stacked xyz inside `radius` of their nearest RoI, scene by scene in row order, and their count per scene (device int32):
    one sv_spc_select in mask mode, one sv_spc_partition, one read."""
    ops = pointnet2_stack_utils.pointnet2
    B = cnt.shape[0]
    sector = ops.spc_select(xyz, cnt, rois, radius, 0)
    order, tables = ops.spc_partition(sector, None, cnt, 0, 0)
    vals = _lib.host_ints([cnt, tables[4][:B]])
    start, rows = 0, []
    for n, k in zip(vals[:B], vals[B:]):
        rows.append(order[start:start + k])
        start += n
    return torch.cat(rows).long(), tables[4][:B]


class VoxelSetAbstraction(nn.Module):
    """Drop-in for the reference VoxelSetAbstraction (backbones_3d/pfe/voxel_set_abstraction.py:122-411).  SAMPLE_METHOD FPS
    (POINT_SOURCE raw_points | voxel_centers): all scenes are sampled in ONE stacked FPS launch; SAMPLE_METHOD SPC (PV-RCNN++): the
    sectorized proposal-centric sampling of all scenes in three launches and one read (csrc/spc_sampling.hip), ragged keypoint counts.  BEV
    features are interpolated in place from the NCHW or the channels_last map (last_bev_layout says which forward entry the most recent
    interpolation took), every SA source runs the HIP ball query / grouping."""

    last_bev_layout = None      # 'nhwc' | 'nchw': written by _BevInterp.forward, so it is one value for the process

    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None, num_rawpoint_features=None, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        SA_cfg = cfg_get(model_cfg, 'SA_LAYER')
        self.SA_layers = nn.ModuleList()
        self.SA_layer_names = []
        self.downsample_times_map = {}
        c_in = 0
        self.sources = list(cfg_get(model_cfg, 'FEATURES_SOURCE'))
        for src in self.sources:
            if src in ['bev', 'raw_points']:
                continue
            sc = SA_cfg[src]
            self.downsample_times_map[src] = cfg_get(sc, 'DOWNSAMPLE_FACTOR')
            inp = cfg_get(sc, 'INPUT_CHANNELS', None)
            if inp is None:
                m0 = cfg_get(sc, 'MLPS')[0]
                inp = m0[0] if isinstance(m0, list) else m0
            layer, c_out = pointnet2_stack_modules.build_local_aggregation_module(input_channels=inp, config=sc)
            self.SA_layers.append(layer)
            self.SA_layer_names.append(src)
            c_in += c_out
        if 'bev' in self.sources:
            c_in += num_bev_features
        if 'raw_points' in self.sources:
            self.SA_rawpoints, c_out = pointnet2_stack_modules.build_local_aggregation_module(
                input_channels=num_rawpoint_features - 3, config=SA_cfg['raw_points'])
            c_in += c_out
        nout = cfg_get(model_cfg, 'NUM_OUTPUT_FEATURES')
        self.vsa_point_feature_fusion = nn.Sequential(nn.Linear(c_in, nout, bias=False), nn.BatchNorm1d(nout), nn.ReLU())
        self.num_point_features = nout
        self.num_point_features_before_fusion = c_in

    def interpolate_from_bev_features(self, keypoints, bev_features, batch_size, bev_stride):
        return _BevInterp.apply(bev_features, keypoints, self.point_cloud_range[0], self.point_cloud_range[1], self.voxel_size[0],
                                self.voxel_size[1], bev_stride)

    def _fps_inputs(self, batch_dict):
        """inputs of the FPS route; SPC keypoints depend on the RoIs and are sampled by sectorized_proposal_centric_sampling"""
        if cfg_get(self.model_cfg, 'SAMPLE_METHOD') != 'FPS':
            raise NotImplementedError("_fps_inputs serves SAMPLE_METHOD FPS only")
        return self._source_points(batch_dict)

    def _source_points(self, batch_dict):
        """(xyz (N, 3) fp32 stacked scene by scene, rows per scene (B,) int32 on the device, the same counts as a host list or None)"""
        batch_size = batch_dict['batch_size']
        src = cfg_get(self.model_cfg, 'POINT_SOURCE')
        if src == 'raw_points':
            src_points = batch_dict['points'][:, 1:4]
            batch_indices = batch_dict['points'][:, 0].long()
            counts = batch_dict.get('points_per_scene')                  # host list from collate_batch (seevcn extension), or absent
        elif src == 'voxel_centers':
            src_points = common_utils.get_voxel_centers(batch_dict['voxel_coords'][:, 1:4], downsample_times=1, voxel_size=self.voxel_size,
                                                        point_cloud_range=self.point_cloud_range)
            batch_indices = batch_dict['voxel_coords'][:, 0].long()
            counts = None
        else:
            raise NotImplementedError
        cnt = common_utils.batch_counts(batch_indices, batch_size)
        return src_points.contiguous().float(), cnt, counts

    def prefetch_keypoints(self, batch_dict):
        """Start the farthest point sampling on a side stream (seevcn extension; Detector3DTemplate.run_modules calls it before the first
        module).  The keypoints depend on the raw points only (voxel_set_abstraction.py:227-281), the sampling is M dependent rounds on 16
        workgroups per scene (7.6 ms for 4 x 20 k points -> 4096): it runs beside the VFE / sparse backbone / BEV backbone instead of in front
        of the set abstraction.  Needs the per-scene point counts on the host (batch_dict['points_per_scene']): without them nothing is
        prefetched and get_sampled_points samples in line."""
        if cfg_get(self.model_cfg, 'SAMPLE_METHOD') != 'FPS':             # SPC keypoints depend on the RoIs: nothing to start early
            return
        if cfg_get(self.model_cfg, 'POINT_SOURCE') != 'raw_points' or batch_dict.get('points_per_scene') is None or not batch_dict['points'].is_cuda:
            return
        xyz, cnt, counts = self._fps_inputs(batch_dict)
        main = torch.cuda.current_stream()
        if getattr(self, '_fps_stream', None) is None or self._fps_stream.device != xyz.device:
            self._fps_stream = torch.cuda.Stream(device=xyz.device, priority=-1)
        side = self._fps_stream
        side.wait_stream(main)                                           # the points were produced on the main stream
        with torch.cuda.stream(side):
            handle = pointnet2_stack_utils.pointnet2.stack_farthest_point_sampling_async(xyz, cnt, cfg_get(self.model_cfg, 'NUM_KEYPOINTS'), max(counts))
            done = side.record_event()
        for t in (xyz, cnt):
            t.record_stream(side)
        batch_dict['_fps_prefetch'] = (handle, done, xyz, cnt, counts)

    def get_sampled_points(self, batch_dict):
        """(B*M, 4) [bs_idx, x, y, z] keypoints by farthest point sampling of every scene (reference :227-281)."""
        batch_size = batch_dict['batch_size']
        m = cfg_get(self.model_cfg, 'NUM_KEYPOINTS')
        method = cfg_get(self.model_cfg, 'SAMPLE_METHOD')
        if method == 'SPC':
            return self.sectorized_proposal_centric_sampling(batch_dict)
        if method != 'FPS':
            raise NotImplementedError
        pre = batch_dict.pop('_fps_prefetch', None)
        if pre is not None:
            handle, done, xyz, cnt, counts = pre
            idx = handle.result()                                        # waits for the side stream only
            torch.cuda.current_stream().wait_event(done)
            idx.record_stream(torch.cuda.current_stream())
            cnt_l = list(counts)
        else:
            xyz, cnt, counts = self._fps_inputs(batch_dict)
            cnt_l = list(counts) if counts is not None else cnt.tolist()
            # points are stacked scene by scene (collate_batch), so the stacked FPS can index them directly
            idx = pointnet2_stack_utils.stack_farthest_point_sample(xyz, cnt, m, max(cnt_l))     # (B, m) global rows
        if min(cnt_l) < m:  # fewer points than keypoints: repeat the valid picks (reference :258-261)
            for b, n in enumerate(cnt_l):
                if n < m:
                    valid = idx[b, :n]
                    idx[b] = valid.repeat(int(m / n) + 1)[:m]
        keypoints = xyz[idx.long().view(-1)]
        bcol = torch.arange(batch_size, device=xyz.device).view(-1, 1).repeat(1, m).view(-1, 1).float()
        batch_dict['point_coords_per_scene'] = m                         # host-side fact for the heads: every scene has exactly m keypoints
        return torch.cat((bcol, keypoints), dim=1)

    def sectorized_proposal_centric_sampling(self, batch_dict):
        """(N1 + N2 + ..., 4) [bs_idx, x, y, z] keypoints of every scene (reference :206-225, 265-270): per scene the sectors ascending, inside a
        sector in pick order.  batch_dict['rois'] (B, M, 7 + C); the per-scene counts stay on the device in batch_dict['_keypoint_batch_cnt']."""
        xyz, cnt, counts = self._source_points(batch_dict)
        spc = cfg_get(self.model_cfg, 'SPC_SAMPLING')
        S = cfg_get(spc, 'NUM_SECTORS')
        max_n = max(counts) if counts is not None else xyz.shape[0]
        sector = pointnet2_stack_utils.pointnet2.spc_select(xyz, cnt, batch_dict['rois'], cfg_get(spc, 'SAMPLE_RADIUS_WITH_ROI'), S, max_n)
        rows, kp_cnt = _spc_rows(xyz, cnt, sector, cfg_get(self.model_cfg, 'NUM_KEYPOINTS'), S, max_n)
        bcol = torch.repeat_interleave(torch.arange(cnt.shape[0], device=xyz.device), kp_cnt.long(), output_size=rows.shape[0])
        batch_dict['_keypoint_batch_cnt'] = kp_cnt
        batch_dict.pop('point_coords_per_scene', None)                 # ragged: the heads count the keypoints per scene themselves
        return torch.cat((bcol.view(-1, 1).float(), xyz[rows.long()]), dim=1)

    @staticmethod
    def aggregate_keypoint_features_from_one_source(batch_size, aggregate_func, xyz, xyz_features, xyz_bs_idxs, new_xyz, new_xyz_batch_cnt,
                                                    filter_neighbors_with_roi=False, radius_of_neighbor=None, num_max_points_of_part=200000,
                                                    rois=None):
        """Reference :283-332.  filter_neighbors_with_roi: only the rows within radius_of_neighbor of their nearest RoI are handed to the aggregation
        (num_max_points_of_part is accepted and ignored); the features reach it through index_select, every row named once."""
        xyz_batch_cnt = common_utils.batch_counts(xyz_bs_idxs, batch_size)
        if filter_neighbors_with_roi:
            rows, xyz_batch_cnt = _selected_rows(xyz.contiguous().float(), xyz_batch_cnt, rois, radius_of_neighbor)
            xyz = xyz.index_select(0, rows)
            xyz_features = xyz_features.index_select(0, rows) if xyz_features is not None else None
        _, pooled = aggregate_func(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt,
                                   features=xyz_features.contiguous() if xyz_features is not None else None)
        return pooled

    def forward(self, batch_dict):
        keypoints = self.get_sampled_points(batch_dict)
        batch_size = batch_dict['batch_size']
        feats = []
        if 'bev' in self.sources:
            feats.append(self.interpolate_from_bev_features(keypoints, batch_dict['spatial_features'], batch_size,
                                                            bev_stride=batch_dict['spatial_features_stride']))
        new_xyz = keypoints[:, 1:4].contiguous()
        new_xyz_batch_cnt = batch_dict.pop('_keypoint_batch_cnt', None)                                # SPC: ragged, counted by the sampler
        if new_xyz_batch_cnt is None:
            new_xyz_batch_cnt = torch.full((batch_size,), keypoints.shape[0] // batch_size, dtype=torch.int32, device=keypoints.device)   # NUM_KEYPOINTS each
        SA_cfg, rois = cfg_get(self.model_cfg, 'SA_LAYER'), batch_dict.get('rois', None)

        def roi_filter(src):
            return dict(filter_neighbors_with_roi=cfg_get(SA_cfg[src], 'FILTER_NEIGHBOR_WITH_ROI', False),
                        radius_of_neighbor=cfg_get(SA_cfg[src], 'RADIUS_OF_NEIGHBOR_WITH_ROI', None), rois=rois)

        if 'raw_points' in self.sources:
            raw = batch_dict['points']
            feats.append(self.aggregate_keypoint_features_from_one_source(
                batch_size, self.SA_rawpoints, raw[:, 1:4], raw[:, 4:].contiguous() if raw.shape[1] > 4 else None, raw[:, 0], new_xyz,
                new_xyz_batch_cnt, **roi_filter('raw_points')))
        for k, src in enumerate(self.SA_layer_names):
            t = batch_dict['multi_scale_3d_features'][src]
            xyz = common_utils.get_voxel_centers(t.indices[:, 1:4], downsample_times=self.downsample_times_map[src], voxel_size=self.voxel_size,
                                                 point_cloud_range=self.point_cloud_range)
            feats.append(self.aggregate_keypoint_features_from_one_source(batch_size, self.SA_layers[k], xyz.contiguous(), t.features.contiguous(),
                                                                          t.indices[:, 0], new_xyz, new_xyz_batch_cnt, **roi_filter(src)))
        point_features = torch.cat(feats, dim=-1)
        point_features = point_features.view(-1, point_features.shape[-1])
        batch_dict['point_features_before_fusion'] = point_features     # the tensor the fusion reads: its gradient is the fusion's input gradient
        from .....dense_ops import run_sequential                       # Linear + BatchNorm1d + ReLU on the library's own GEMM / BatchNorm kernels
        batch_dict['point_features'] = run_sequential(self.vsa_point_feature_fusion, point_features)
        batch_dict['point_coords'] = keypoints
        return batch_dict
