"""Generate tests/golden/vector_pool_modules.npz by running the REFERENCE's own VectorPoolAggregationModuleMSG (pointnet2_stack/pointnet2_modules.py)
on the CPU, in eval mode with seeded weights, for the two small layers of vector_pool_inputs.py: one `local_interpolation`, one
`voxel_random_choice`.  The compiled extension under it is replaced here by functions over the numpy restatement (tests/vector_pool_reference.py)
with the extension's own call signatures -- the host-sized buffers, the returned counts and the retry loops of the reference's Python are
served as they are.  Recorded: state_dict keys and shapes, the inputs and the eval-mode outputs.

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_vector_pool_golden.py
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
import vector_pool_reference as VR  # noqa: E402
import vector_pool_inputs as I  # noqa: E402

ext = sys.modules["pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"]


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


def vector_pool_wrapper(support_xyz, xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, new_features, new_local_xyz, point_cnt_of_grid,
                        grouped_idxs, num_grid_x, num_grid_y, num_grid_z, max_neighbour_distance, use_xyz, num_max_sum_points, nsample,
                        neighbor_type, pooling_type):
    assert pooling_type == 1
    G = num_grid_x * num_grid_y * num_grid_z
    ch, cnt, loc, nf = VR.choice(support_xyz.numpy(), xyz_batch_cnt.numpy(), support_features.detach().numpy(), new_xyz.numpy(),
                                 new_xyz_batch_cnt.numpy(), (num_grid_x, num_grid_y, num_grid_z), max_neighbour_distance, nsample, neighbor_type,
                                 new_features.shape[1] // G)
    new_features.copy_(torch.from_numpy(nf))
    new_local_xyz.copy_(torch.from_numpy(loc))
    point_cnt_of_grid.copy_(torch.from_numpy(cnt))
    m, g = np.nonzero(ch >= 0)
    n = min(len(m), grouped_idxs.shape[0])
    grouped_idxs[:n] = torch.from_numpy(np.stack([ch[m, g], m, g], 1)[:n].astype(np.int32))
    return len(m)


for fn in (query_stacked_local_neighbor_idxs_wrapper_stack, query_three_nn_by_stacked_local_idxs_wrapper_stack, three_interpolate_wrapper,
           vector_pool_wrapper):
    setattr(ext, fn.__name__, fn)

from easydict import EasyDict  # noqa: E402
from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as ref_modules  # noqa: E402

torch.set_num_threads(8)
out = {}
for tag, c in I.CONFIGS.items():
    layer, num_c_out = ref_modules.build_local_aggregation_module(input_channels=c["input_channels"], config=EasyDict(c["cfg"]))
    layer.load_state_dict(R.seeded_state_dict(layer, seed=I.WEIGHT_SEED))
    layer.eval()
    sd = layer.state_dict()
    out[tag + "_names"] = np.array(list(sd.keys()))
    out[tag + "_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    inp = I.make_inputs(tag)
    with torch.no_grad():
        new_xyz, feats = layer(xyz=torch.from_numpy(inp["xyz"]), xyz_batch_cnt=torch.from_numpy(inp["xyz_batch_cnt"]),
                               new_xyz=torch.from_numpy(inp["new_xyz"]), new_xyz_batch_cnt=torch.from_numpy(inp["new_xyz_batch_cnt"]),
                               features=torch.from_numpy(inp["features"]))
    assert feats.shape == (len(inp["new_xyz"]), num_c_out)
    out.update({f"{tag}_{k}": v for k, v in inp.items()})
    out[tag + "_out"] = feats.numpy()
    print(tag, len(sd), feats.shape, float(feats.abs().mean()), "zero rows:", int((feats.abs().sum(1) == 0).sum()))
path = os.path.join(HERE, "vector_pool_modules.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
