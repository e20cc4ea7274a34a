"""Vector pool without a GPU: the numpy restatement (tests/vector_pool_reference.py) pinned on cases small enough to read, and this repository's
VectorPoolAggregationModuleMSG held to the state_dict names and shapes of the reference's own class (tests/golden/vector_pool_modules.npz,
made by tests/golden/make_vector_pool_golden.py)."""
import os

import numpy as np
import pytest

import vector_pool_inputs as I
import vector_pool_reference as VR

F = np.float32
Q0 = np.zeros((1, 3), F)


def _choice(points, grid, R, nsample, neighbor_type=0, feats=None, c_each=1):
    points = np.asarray(points, F).reshape(-1, 3)
    feats = np.arange(len(points), dtype=F).reshape(-1, 1) + 1 if feats is None else np.asarray(feats, F)
    return VR.choice(points, [len(points)], feats, Q0, [1], grid, R, nsample, neighbor_type, c_each)


def test_rows_on_the_boundary_are_in_range_and_alias():
    """local == +-R is not rejected (the test is '>'); the per-axis index at +R is n, one past the last, and only the COMBINED index is clamped."""
    pts = [[-1, 0, 0],          # ix 0, iy 1, iz 1 -> 3
           [1, -1, -1],         # ix 2 -> 8, clamped to 7: the (+, +, +) cell although y and z sit at -R
           [-0.5, 1, -0.5],     # iy 2 -> 0 * 4 + 2 * 2 + 0 = 4: aliases into cell (ix 1, iy 0, iz 0) without any clamp
           [1.0000001, 0, 0]]   # beyond R: rejected
    for neighbor_type in (0, 1):
        use = pts if neighbor_type == 0 else [pts[0], [1, 0, 0], [0, 0, -1], pts[3]]
        ch, cnt, loc, nf = _choice(use, [2, 2, 2], 1.0, -1, neighbor_type)
        if neighbor_type == 0:
            assert ch.tolist() == [[-1, -1, -1, 0, 2, -1, -1, 1]]
            assert nf.tolist() == [[0, 0, 0, 1, 3, 0, 0, 2]]
            assert loc.reshape(8, 3)[7].tolist() == [1, -1, -1] and loc.reshape(8, 3)[0].tolist() == [0, 0, 0]
        else:
            # (1, 0, 0): 1 > 1 is false -> in range; ix 2, iy 1, iz 1 -> 11 -> 7.  (0, 0, -1): ix 1, iy 1, iz 0 -> 6
            assert ch.tolist() == [[-1, -1, -1, 0, -1, -1, 2, 1]]
        assert np.array_equal(cnt, (ch >= 0).astype(np.int32))
    # the ball rejects a cube corner that the cube keeps
    assert _choice([[0.7, 0.7, 0.7]], [1, 1, 1], 1.0, -1, 0)[0].tolist() == [[0]]
    assert _choice([[0.7, 0.7, 0.7]], [1, 1, 1], 1.0, -1, 1)[0].tolist() == [[-1]]


def test_non_cubic_grid_and_the_combined_clamp():
    """grid [3, 2, 1], R = 1.5: gs = (1, 1.5, 3); G = 6.  x == +R gives ix 3 -> 3 * 2 + ... >= 6, clamped to 5."""
    pts = [[-1.2, -1, 0], [-1.2, 1, 0], [0, -1, 0], [1.2, 1, 0], [1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]
    ch = _choice(pts, [3, 2, 1], 1.5, -1)[0]
    # rows 0..3 -> cells 0, 1, 2, 5; row 4: ix 3, iy 0, iz 0 -> 6 -> 5 (taken already); row 5: ix 3, iy 2 (y == +R), iz 1 -> 6 + 2 + 1 -> 5
    assert ch.tolist() == [[0, 1, 2, -1, -1, 3]]


def test_nsample_counts_taken_rows_only_and_the_last_channel_group_wins():
    pts = [[-0.5, -0.5, -0.5], [-0.4, -0.4, -0.4], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5]]
    feats = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]]
    ch, cnt, loc, nf = _choice(pts, [2, 2, 2], 1.0, 2, 0, feats, 2)
    # row 1 shares row 0's cell: skipped and NOT counted, so row 2 is the second taken row and the walk stops before row 3
    assert ch.tolist() == [[0, -1, -1, -1, -1, -1, -1, 2]]
    assert nf.reshape(8, 2)[0].tolist() == [3, 4] and nf.reshape(8, 2)[7].tolist() == [11, 12]        # channels c_in - c_each ..
    assert _choice(pts, [2, 2, 2], 1.0, -1, 0, feats, 2)[0].tolist() == [[0, -1, -1, -1, -1, 3, -1, 2]]
    # duplicate points: the lower row is taken
    assert _choice([pts[2], pts[2]], [2, 2, 2], 1.0, -1)[0][0, 7] == 0
    # every cell filled: the walk ends at G taken rows
    corners = [[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]
    assert _choice(corners + corners, [2, 2, 2], 1.0, -1)[0].tolist() == [list(range(8))]


def test_choice_gradient_reaches_every_channel_group():
    ch = np.array([[1, -1], [1, 0]], np.int32)
    g = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], F)                              # (M 2, G 2 * c_each 2)
    terms = VR.choice_grad_terms(g, ch, (ch >= 0).astype(np.int32), 3, 4, 2)
    assert [len(t) for t in terms] == [1, 2, 0]
    assert terms[1].tolist() == [[1, 2, 1, 2], [5, 6, 5, 6]] and terms[0].tolist() == [[7, 8, 7, 8]]      # keys 0 and 2 name row 1, ascending
    assert VR.ordered_sum(terms, 4).tolist() == [[7, 8, 7, 8], [6, 8, 6, 8], [0, 0, 0, 0]]


def test_three_nn_short_lists_ties_and_the_cap():
    xyz = np.array([[0.1, 0, 0], [0.1, 0, 0], [0.3, 0, 0], [5, 5, 5]], F)
    centre = np.zeros((1, 1, 3), F)

    def nn(rows, nsample=-1):
        return VR.three_nn(xyz[rows], [len(rows)], Q0, centre, [1], F(1.0), nsample, 0)

    idx, d2 = nn([3])                                                          # nothing in range
    assert idx.tolist() == [[[-1, -1, -1]]] and np.all(np.isposinf(d2))
    idx, d2 = nn([2, 3])                                                       # one entry: slots 2 and 3 repeat it
    assert idx.tolist() == [[[0, 0, 0]]] and d2[0, 0].tolist() == [F(0.3) * F(0.3)] * 3
    idx, d2 = nn([2, 0])                                                       # two entries: slot 3 repeats slot ONE
    assert idx.tolist() == [[[1, 0, 1]]]
    idx, d2 = nn([2, 0, 1])                                                    # duplicates tie: the lower row first
    assert idx.tolist() == [[[1, 2, 0]]]
    idx, _ = nn([2, 0, 1], nsample=2)                                          # the list is cut BEFORE the search: row 2 is never seen
    assert idx.tolist() == [[[1, 0, 1]]]
    many = np.concatenate([np.full((VR.LIST_CAP, 3), 0.5, F), np.zeros((1, 3), F)])
    idx, _ = VR.three_nn(many, [len(many)], Q0, centre, [1], F(1.0), -1, 0)     # row 1000 is nearer and ignored
    assert idx.tolist() == [[[0, 1, 2]]]


def test_interpolate_statement():
    f = np.array([[1, 10], [2, 20], [4, 40]], F)
    idx = np.array([[0, 1, 2], [1, 1, 1], [0, -1, 7], [2, 1, 0]], np.int32)
    w = np.array([[0.5, 0.25, 0.25], [0.2, 0.3, 0.5], [1, 1, 1], [0, 0, 0]], F)
    out = VR.interpolate(f, idx, w)
    assert out[0].tolist() == [2, 20] and out[2].tolist() == [1, 10] and out[3].tolist() == [0, 0]
    assert out[1, 0] == F(F(F(F(0.2) * 2) + F(F(0.3) * 2)) + F(F(0.5) * 2))
    terms = VR.interpolate_grad_terms(np.ones((4, 2), F), idx, w, 3)
    assert [len(t) for t in terms] == [3, 5, 2]


@pytest.mark.parametrize("tag", sorted(I.CONFIGS))
def test_module_state_dict_matches_the_reference(golden_dir, tag):
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm
    gold = np.load(os.path.join(golden_dir, "vector_pool_modules.npz"))
    c = I.CONFIGS[tag]
    layer, num_c_out = pm.build_local_aggregation_module(input_channels=c["input_channels"], config=c["cfg"])
    assert isinstance(layer, pm.VectorPoolAggregationModuleMSG) and num_c_out == c["cfg"]["MSG_POST_MLPS"][-1]
    sd = layer.state_dict()
    assert list(sd.keys()) == list(gold[tag + "_names"])
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(gold[tag + "_shapes"])
    assert gold[tag + "_out"].shape == (int(sum(c["queries"])), num_c_out)
    for k in ("local_interpolate_module", "separate_local_aggregation_layer", "post_mlps"):
        assert hasattr(layer.layer_0, k)
    assert layer.layer_0.num_mean_points_per_grid == 20
    if tag == "interp":
        assert layer.layer_1.local_interpolate_module.num_avg_length_of_neighbor_idxs == 1000


def test_unbuilt_corners_raise():
    from seevcn_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm, pointnet2_stack_cuda as ext
    with pytest.raises(NotImplementedError):
        pm.VectorPoolAggregationModule(input_channels=4, local_aggregation_type='voxel_avg_pool', num_reduced_channels=2, max_neighbor_distance=1.0)
    for name in ("vector_pool_wrapper", "vector_pool_grad_wrapper", "query_stacked_local_neighbor_idxs_wrapper_stack",
                 "query_three_nn_by_stacked_local_idxs_wrapper_stack", "three_nn_wrapper"):
        with pytest.raises(NotImplementedError):
            getattr(ext, name)()
    import seevcn_amd
    assert {"three_interpolate", "vector_pool"} <= set(seevcn_amd.ordered_gradient_calls())
