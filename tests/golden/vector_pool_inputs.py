"""Seeded inputs and the two small VectorPoolAggregationModuleMSG configurations shared by make_vector_pool_golden.py and tests/test_vector_pool*.py.
Data and settings only."""
import numpy as np

# one layer per aggregation type, at sizes a CPU restatement walks in a blink (pv_rcnn_plusplus.yaml's shapes: 90 -> 30 and 64 -> 32 channels)
CONFIGS = {
    "interp": {"input_channels": 4, "seed": 31, "support": (53, 68), "queries": (7, 5), "cfg": {
        "NAME": "VectorPoolAggregationModuleMSG", "NUM_GROUPS": 2, "LOCAL_AGGREGATION_TYPE": "local_interpolation", "NUM_REDUCED_CHANNELS": 2,
        "NUM_CHANNELS_OF_LOCAL_AGGREGATION": 8, "MSG_POST_MLPS": [16],
        "GROUP_CFG_0": {"NUM_LOCAL_VOXEL": [2, 2, 2], "MAX_NEIGHBOR_DISTANCE": 0.5, "NEIGHBOR_NSAMPLE": -1, "POST_MLPS": [16, 16]},
        "GROUP_CFG_1": {"NUM_LOCAL_VOXEL": [3, 3, 3], "MAX_NEIGHBOR_DISTANCE": 0.9, "NEIGHBOR_NSAMPLE": 6, "POST_MLPS": [16, 16]}}},
    "choice": {"input_channels": 6, "seed": 32, "support": (44, 70), "queries": (9, 6), "cfg": {
        "NAME": "VectorPoolAggregationModuleMSG", "NUM_GROUPS": 2, "LOCAL_AGGREGATION_TYPE": "voxel_random_choice", "NUM_REDUCED_CHANNELS": 3,
        "NUM_CHANNELS_OF_LOCAL_AGGREGATION": 8, "MSG_POST_MLPS": [16],
        "GROUP_CFG_0": {"NUM_LOCAL_VOXEL": [3, 3, 3], "MAX_NEIGHBOR_DISTANCE": 0.6, "NEIGHBOR_NSAMPLE": 4, "POST_MLPS": [16, 16]},
        "GROUP_CFG_1": {"NUM_LOCAL_VOXEL": [3, 3, 3], "MAX_NEIGHBOR_DISTANCE": 1.2, "NEIGHBOR_NSAMPLE": 4, "POST_MLPS": [16, 16]}}},
}
WEIGHT_SEED = 23


def make_inputs(tag):
    """xyz (N, 3), xyz_batch_cnt (2,), new_xyz (M, 3), new_xyz_batch_cnt (2,), features (N, C): two ragged scenes in a cube of edge 2; the
    queries are support points moved a little, and the last query of the first scene sits far from every point (empty cells everywhere)."""
    c = CONFIGS[tag]
    rng = np.random.default_rng(c["seed"])
    xyz, new_xyz = [], []
    for n, m in zip(c["support"], c["queries"]):
        p = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        q = (p[rng.choice(n, m, replace=False)] + rng.normal(0, 0.05, (m, 3))).astype(np.float32)
        xyz.append(p)
        new_xyz.append(q)
    new_xyz[0][-1] = np.float32(9.0)
    N = sum(c["support"])
    features = rng.normal(0, 1, (N, c["input_channels"])).astype(np.float32)
    return {"xyz": np.concatenate(xyz), "xyz_batch_cnt": np.array(c["support"], np.int32), "new_xyz": np.concatenate(new_xyz),
            "new_xyz_batch_cnt": np.array(c["queries"], np.int32), "features": features}
