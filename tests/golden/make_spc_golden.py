"""Generate tests/golden/spc_sampling.npz by running the REFERENCE's own sample_points_with_roi, sector_fps and VoxelSetAbstraction (SAMPLE_METHOD SPC,
FILTER_NEIGHBOR_WITH_ROI, sources bev + raw_points with the vector-pool layer shrunk; backbones_3d/pfe/voxel_set_abstraction.py) on the CPU, eval mode,
seeded weights, on the inputs of spc_inputs.py.  The compiled extension under them is replaced by functions over the numpy restatements with the
extension's own call signatures: stack_farthest_point_sampling_wrapper over tests/spc_reference.py, the vector-pool entries over
tests/vector_pool_reference.py (as make_vector_pool_golden.py does).  Recorded: the inputs, per scene the selection mask, what sector_fps handed
to the sampler (points by sector, counts, quotas), the keypoints, and the module's outputs.

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_spc_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refimport as R  # noqa: E402

R.import_pcdet()
import spc_inputs as I  # noqa: E402
import spc_reference as SR  # noqa: E402
import vector_pool_reference as VR  # noqa: E402

ext = sys.modules["pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"]
handed = []          # what sector_fps hands to the sampler, call by call


def stack_farthest_point_sampling_wrapper(xyz, temp, xyz_batch_cnt, output, npoint):
    handed.append((xyz.numpy().copy(), xyz_batch_cnt.numpy().copy(), npoint.numpy().copy()))
    output.copy_(torch.from_numpy(SR.stack_fps(xyz.numpy(), xyz_batch_cnt.numpy(), npoint.numpy()).astype(np.int32)))
    return 1


def query_stacked_local_neighbor_idxs_wrapper_stack(support_xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, stack_neighbor_idxs, start_len, cumsum,
                                                    avg_length_of_neighbor_idxs, max_neighbour_distance, nsample, neighbor_type):
    xyz, q = support_xyz.numpy(), new_xyz.numpy()
    total = 0
    for (qs, qn), (ps, pn) in zip(VR.scene_ranges(new_xyz_batch_cnt.numpy()), VR.scene_ranges(xyz_batch_cnt.numpy())):
        for m in range(qs, qs + qn):
            rows = ps + VR.neighbour_list(xyz[ps:ps + pn], q[m], np.float32(max_neighbour_distance), nsample, neighbor_type)
            start_len[m, 0], start_len[m, 1] = total, len(rows)
            if total + len(rows) <= stack_neighbor_idxs.shape[0]:
                stack_neighbor_idxs[total:total + len(rows)] = torch.from_numpy(rows.astype(np.int32))
            total += len(rows)
    cumsum[0] = total


def query_three_nn_by_stacked_local_idxs_wrapper_stack(support_xyz, new_xyz, new_xyz_grid_centers, new_xyz_grid_idxs, new_xyz_grid_dist2,
                                                       stack_neighbor_idxs, start_len, M, num_total_grids):
    xyz, centers, stack, sl = support_xyz.numpy(), new_xyz_grid_centers.numpy(), stack_neighbor_idxs.numpy(), start_len.numpy()
    for m in range(M):
        idx, d2 = VR.three_nn_of_list(xyz, stack[sl[m, 0]:sl[m, 0] + sl[m, 1]], centers[m])
        new_xyz_grid_idxs[m] = torch.from_numpy(idx)
        new_xyz_grid_dist2[m] = torch.from_numpy(d2)


def three_interpolate_wrapper(features, idx, weight, out):
    out.copy_(torch.from_numpy(VR.interpolate(features.detach().numpy(), idx.numpy(), weight.detach().numpy())))


for fn in (stack_farthest_point_sampling_wrapper, query_stacked_local_neighbor_idxs_wrapper_stack, query_three_nn_by_stacked_local_idxs_wrapper_stack,
           three_interpolate_wrapper):
    setattr(ext, fn.__name__, fn)

from easydict import EasyDict  # noqa: E402
from pcdet.models.backbones_3d.pfe import voxel_set_abstraction as ref_vsa  # noqa: E402

torch.set_num_threads(8)
inp = I.make_inputs()
out = {k: inp[k] for k in ("xyz", "cnt", "rois", "feats", "bev")}
masks, kps, kp_cnt, filt = [], [], [], []
seg_xyz, seg_cnt, seg_npoint, seg_scene = [], [], [], []
for b, (s, n) in enumerate(zip(inp["start"], inp["cnt"])):
    pts, rois = torch.from_numpy(inp["xyz"][s:s + n]), torch.from_numpy(inp["rois"][b])
    sampled, mask = ref_vsa.sample_points_with_roi(rois=rois, points=pts, sample_radius_with_roi=I.RADIUS)
    handed.clear()
    kp = ref_vsa.sector_fps(points=sampled, num_sampled_points=I.K, num_sectors=I.S)
    (x, c, m), = handed
    seg_xyz.append(x), seg_cnt.append(c), seg_npoint.append(m), seg_scene.append(np.full(len(c), b))
    masks.append(mask.numpy()), kps.append(kp.numpy()), kp_cnt.append(len(kp))
    filt.append(int(ref_vsa.sample_points_with_roi(rois=rois, points=pts, sample_radius_with_roi=I.FILTER_RADIUS, num_max_points_of_part=1000)[1].sum()))
out.update(point_mask=np.concatenate(masks), keypoints=np.concatenate(kps), kp_cnt=np.array(kp_cnt, np.int32), filter_mask_cnt=np.array(filt, np.int32),
           seg_xyz=np.concatenate(seg_xyz), seg_cnt=np.concatenate(seg_cnt).astype(np.int32), seg_npoint=np.concatenate(seg_npoint).astype(np.int32),
           seg_scene=np.concatenate(seg_scene).astype(np.int32))
print("selected", [int(m.sum()) for m in masks], "keypoints", kp_cnt, "filter", filt, "segments", out["seg_cnt"], out["seg_npoint"])

# ---- the module
vsa = ref_vsa.VoxelSetAbstraction(EasyDict(I.module_cfg()), voxel_size=I.VOXEL_SIZE, point_cloud_range=np.array(I.PC_RANGE, np.float32), num_bev_features=16,
                                  num_rawpoint_features=7)
vsa.load_state_dict(R.seeded_state_dict(vsa, seed=I.MODULE_SEED))
vsa.eval()
sd = vsa.state_dict()
out["module_names"] = np.array(list(sd.keys()))
out["module_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
with torch.no_grad():
    bd = vsa({"batch_size": 2, "points": torch.from_numpy(I.points_tensor(inp)), "rois": torch.from_numpy(inp["rois"]),
              "spatial_features": torch.from_numpy(inp["bev"]), "spatial_features_stride": I.BEV_STRIDE})
out.update(point_coords=bd["point_coords"].numpy(), point_features=bd["point_features"].numpy(),
           point_features_before_fusion=bd["point_features_before_fusion"].numpy())
print("module", bd["point_features"].shape, float(bd["point_features"].abs().mean()), "zero rows before fusion:",
      int((bd["point_features_before_fusion"][:, 16:].abs().sum(1) == 0).sum()))
path = os.path.join(HERE, "spc_sampling.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")

# ---- the yaml's MODEL section as data, for the key-by-key check of model_cfgs.pvrcnnpp_model_cfg (tests/test_pvrcnn_plusplus.py)
import json  # noqa: E402

import yaml  # noqa: E402

with open(os.path.join(R.REF, "detector3d", "tools", "cfgs", "waymo_models", "pv_rcnn_plusplus.yaml")) as f:
    model = yaml.safe_load(f)["MODEL"]
with open(os.path.join(HERE, "pv_rcnn_plusplus_model.json"), "w") as f:
    json.dump(model, f, indent=1, sort_keys=True)
