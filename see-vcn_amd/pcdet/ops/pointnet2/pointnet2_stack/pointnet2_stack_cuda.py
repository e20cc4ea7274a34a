"""Same entry-point names and argument order as the reference's compiled extension `pointnet2_stack_cuda`
(detector3d/pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp:12-31), bound to libseevcn_hip.so.
Outputs are caller-allocated torch tensors, every function returns 1 like the reference wrappers."""
import os

import torch

from ..... import _lib, ordered


def _version(t):
    try:
        return t._version
    except RuntimeError:                                  # inference tensors keep no version counter: nothing is cached on them
        return None


def _starts(cnt):
    """(first row of every scene, rows per scene) as int32 device tensors.  A step asks for the same few count tensors again and again (every
    scale of every source: 25 cumsum + 25 sub launches per PV-RCNN step), so the pair is kept on the count tensor OBJECT, keyed by its
    version counter (an in-place change invalidates it)."""
    ver = _version(cnt)
    hit = getattr(cnt, "_sv_starts", None) if ver is not None else None
    if hit is not None and hit[0] == ver:
        return hit[1], hit[2]
    c32 = cnt.to(torch.int32).contiguous()
    st = (torch.cumsum(c32, 0, dtype=torch.int32) - c32).contiguous()
    if ver is not None:
        try:
            cnt._sv_starts = (ver, st, c32)
        except Exception:                                 # a tensor subclass without instance attributes: no cache
            pass
    return st, c32


BALL_HASH_MIN_POINTS = int(os.environ.get("SEEVCN_BALL_HASH_MIN", "2048"))   # support sets below this (or nsample > 64) are scanned like the reference does


def ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx):
    lib = _lib.load()
    qs, qc = _starts(new_xyz_batch_cnt)
    ps, pc = _starts(xyz_batch_cnt)
    n = int(xyz.shape[0])
    if n >= BALL_HASH_MIN_POINTS and nsample <= 64 and radius > 0:
        # the same idx, element for element, from a cell hash of the support points (sv_ball_query_stack_hashed) instead of the O(M N) scan
        scratch = _lib.workspace.scratch("ball_hash", lib.sv_ball_query_hash_scratch_bytes(n), xyz.device)
        _lib.launch("sv_ball_query_stack_hashed", int(B), int(M), n, float(radius), int(nsample), _lib.ptr(new_xyz), _lib.ptr(qs), _lib.ptr(qc), _lib.ptr(xyz),
                    _lib.ptr(ps), _lib.ptr(pc), _lib.ptr(scratch), _lib.ptr(idx))
        return 1
    max_q = int(M)  # upper bound of queries per scene without a host sync
    _lib.launch("sv_ball_query_stack", int(B), int(M), max_q, float(radius), int(nsample), _lib.ptr(new_xyz), _lib.ptr(qs), _lib.ptr(qc), _lib.ptr(xyz),
                _lib.ptr(ps), _lib.ptr(pc), _lib.ptr(idx))
    return 1


def _row_start(idx_batch_cnt, features_batch_cnt, M):
    """first feature row of the scene each query belongs to (M,) int32"""
    vf, vi = _version(features_batch_cnt), _version(idx_batch_cnt)
    cacheable = vf is not None and vi is not None
    cache = getattr(idx_batch_cnt, "_sv_row_start", None) if cacheable else None
    key = (id(features_batch_cnt), vf, vi, int(M))
    if cache is not None and cache[0] == key and cache[1] is features_batch_cnt:
        return cache[2]
    fs, _ = _starts(features_batch_cnt)
    rs = torch.repeat_interleave(fs, idx_batch_cnt.long(), output_size=int(M)).contiguous()
    if cacheable:
        try:
            idx_batch_cnt._sv_row_start = (key, features_batch_cnt, rs)  # the last support set asked for with these queries (scales come in a row)
        except Exception:
            pass
    return rs


def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, out):
    rs = _row_start(idx_batch_cnt, features_batch_cnt, M)
    _lib.launch("sv_group_points_stack", int(M), int(C), int(nsample), _lib.ptr(features), _lib.ptr(idx), _lib.ptr(rs), _lib.ptr(out))
    return 1


def group_points_grad_wrapper(B, M, C, N, nsample, grad_out, idx, idx_batch_cnt, features_batch_cnt, grad_features):
    lib = _lib.load()
    rs = _row_start(idx_batch_cnt, features_batch_cnt, M)
    if ordered.ordered_gradients():                       # same terms in ascending (query, slot) order, no float atomics
        nbytes = lib.sv_group_points_grad_stack_ordered_scratch_bytes(int(M), int(N), int(nsample))
        scratch = _lib.workspace.scratch("group_grad_ordered", nbytes, grad_out.device)
        _lib.launch("sv_group_points_grad_stack_ordered", int(M), int(C), int(N), int(nsample), _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(rs),
                    _lib.ptr(scratch), _lib.ptr(grad_features))
        ordered.count_call("group_points")
        return 1
    _lib.launch("sv_group_points_grad_stack", int(M), int(C), int(N), int(nsample), _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(rs), _lib.ptr(grad_features))
    return 1


def fps_bucketed(points, starts, cnt, batch, fixed_n, max_n, m, idx):
    """One workgroup per scene on spatial buckets (csrc/fps_bucket.hip) where it applies -> True; False: the caller takes the exhaustive kernels.
    Same indices either way."""
    lib = _lib.load()
    if not lib.sv_fps_bucket_applies(int(batch), int(max_n), int(m)):
        return False
    if cnt is not None:
        # the kernels size their scene slabs from the HOST's max_n: a scene longer than that (a stale points-per-scene bound) would be cut short without a
        # word -- the exhaustive kernels had their error word for this.  Parked: raised at the stream's next host read, no read of its own.
        def _check(v, max_n=int(max_n)):
            if v > max_n:
                raise _lib.SeevcnHipError(f"farthest_point_sampling: a scene has {v} points, the caller's max_n is {max_n}")
        _lib.defer_check(cnt.max(), _check)
    scratch = torch.empty((int(lib.sv_fps_bucket_scratch_bytes(int(batch), int(max_n))),), dtype=torch.uint8, device=points.device)
    _lib.launch("sv_farthest_point_sampling_bucketed", _lib.ptr(points), _lib.ptr(starts), _lib.ptr(cnt), int(batch), int(fixed_n), int(max_n), int(m),
                _lib.ptr(scratch), _lib.ptr(idx))
    return True


def farthest_point_sampling_wrapper(b, n, m, points, temp, idx):
    """The fixed-layout call, (b, n, 3) -> (b, m), of both pointnet2 wrappers and vcn.utils.misc.fps.  temp None: the (b, n) buffer of the exhaustive
    kernels is allocated here, only when they run."""
    if fps_bucketed(points, None, None, b, n, n, m, idx):
        return 1
    if temp is None:
        temp = torch.empty((int(b), int(n)), dtype=torch.float32, device=points.device)
    _lib.launch("sv_farthest_point_sampling", _lib.ptr(points), int(b), int(n), int(m), _lib.ptr(temp), _lib.ptr(idx))
    return 1


def _exhaustive_scratch(lib, points, batch, max_n):
    """(temp past the register path, records + error word of several workgroups per scene: the library decides whether it uses them; same indices)"""
    temp = torch.empty((points.shape[0],), dtype=torch.float32, device=points.device) if max_n > 24576 else None
    scratch = torch.empty((int(lib.sv_fps_multi_scratch_bytes(batch)),), dtype=torch.uint8, device=points.device)
    return temp, scratch


def stack_farthest_point_sampling(points, xyz_batch_cnt, npoint, max_n=None, bucketed=True):
    """All ragged scenes in one launch -> (batch, npoint) int32 GLOBAL row indices (seevcn extension; replaces the
    per-scene loop of voxel_set_abstraction.py:250-256).  bucketed=False: the exhaustive kernels only (tests, A/B runs)."""
    lib = _lib.load()
    starts, cnt = _starts(xyz_batch_cnt)
    batch = cnt.shape[0]
    if max_n is None:
        max_n = int(cnt.max().item())
    idx = torch.empty((batch, npoint), dtype=torch.int32, device=points.device)
    if bucketed and fps_bucketed(points, starts, cnt, batch, 0, max_n, npoint, idx):
        return idx
    temp, scratch = _exhaustive_scratch(lib, points, batch, max_n)
    _lib.launch("sv_stack_farthest_point_sampling_multi", _lib.ptr(points), _lib.ptr(starts), _lib.ptr(cnt), batch, int(max_n), int(npoint), _lib.ptr(temp),
                _lib.ptr(scratch), _lib.ptr(idx))
    return idx


class FpsHandle:
    """A stacked farthest point sampling in flight (stack_farthest_point_sampling_async).  result() returns the (batch, npoint) int32 GLOBAL row
    indices; it reads the kernel's error word on the stream the sampling ran on (so only that stream is waited for) and samples once more with
    write-through records if a partner workgroup did not arrive."""

    def __init__(self, idx, err, stream, rerun):
        self.idx, self.err, self.stream, self._rerun = idx, err, stream, rerun
        self.done = torch.cuda.Event()         # behind the sampling on its stream: what result() orders the caller's stream after when there is no error word to read
        self.done.record(stream)

    def result(self):
        if self.err is None:                   # sampled by the one-workgroup bucket kernel: nothing that could have gone missing
            torch.cuda.current_stream().wait_event(self.done)      # no host wait: the caller's stream goes behind the sampling stream
            return self.idx
        with torch.cuda.stream(self.stream):
            bad = int(self.err.item())
            if bad:
                self._rerun()
                bad = int(self.err.item())
        if bad:
            raise _lib.SeevcnHipError("farthest_point_sampling: a partner workgroup never arrived (GPU shared with another process?); "
                                      "SEEVCN_FPS_MULTI=0 selects one workgroup per scene")
        return self.idx


def stack_farthest_point_sampling_async(points, xyz_batch_cnt, npoint, max_n):
    """stack_farthest_point_sampling without the read-back: enqueues on the current stream and returns an FpsHandle (seevcn extension, used to
    sample the keypoints on a side stream while the backbone runs).  max_n (largest scene) must come from the host."""
    lib = _lib.load()
    starts, cnt = _starts(xyz_batch_cnt)
    batch = cnt.shape[0]
    idx = torch.empty((batch, npoint), dtype=torch.int32, device=points.device)
    if fps_bucketed(points, starts, cnt, batch, 0, max_n, npoint, idx):
        return FpsHandle(idx, None, torch.cuda.current_stream(), None)
    temp, scratch = _exhaustive_scratch(lib, points, batch, max_n)
    off = int(lib.sv_fps_multi_error_offset(batch))
    err = scratch[off:off + 4].view(torch.int32)
    stream = torch.cuda.current_stream()

    def launch(write_through):
        _lib.launch("sv_stack_farthest_point_sampling_multi_async", _lib.ptr(points), _lib.ptr(starts), _lib.ptr(cnt), batch, int(max_n), int(npoint),
                    _lib.ptr(temp), _lib.ptr(scratch), _lib.ptr(idx), int(write_through))

    launch(0)
    return FpsHandle(idx, err, stream, lambda: launch(1))


def spc_select(xyz, xyz_batch_cnt, rois, radius, num_sectors, max_n=None):
    """sample_points_with_roi + the sector expression of sector_fps for every scene in one launch (seevcn extension; voxel_set_abstraction.py:45-75,
    88-90).  xyz (N, 3) stacked, rois (B, M, 7 + C) -> sector (N,) int32: -1 not selected | 0..num_sectors; num_sectors == 0: 0 selected | -1.
    max_n: an upper bound of the largest scene known on the host (None: N)."""
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and rois.dim() == 3
    starts, cnt = _starts(xyz_batch_cnt)
    rois = rois.contiguous().float()
    assert rois.shape[0] == cnt.shape[0], "one set of RoIs per scene"
    sector = torch.empty((xyz.shape[0],), dtype=torch.int32, device=xyz.device)
    _lib.launch("sv_spc_select", _lib.ptr(xyz), _lib.ptr(starts), _lib.ptr(cnt), cnt.shape[0], int(xyz.shape[0] if max_n is None else max_n), _lib.ptr(rois),
                rois.shape[1], rois.shape[2], float(radius), int(num_sectors), _lib.ptr(sector))
    return sector


def spc_partition(sector, xyz, xyz_batch_cnt, num_keypoints, num_sectors):
    """The stable (scene, sector) row lists, quotas and output offsets of sector_fps (voxel_set_abstraction.py:91-113) for every scene in one launch
    -> (order (N,), tables (5, B * max(S, 1)) int32 rows seg_start / seg_cnt / seg_m / seg_out_start / kp_cnt -- kp_cnt fills the first B entries of
    its row).  Nothing is read back."""
    assert sector.dtype == torch.int32 and sector.is_contiguous()
    starts, cnt = _starts(xyz_batch_cnt)
    B, nseg = cnt.shape[0], cnt.shape[0] * max(int(num_sectors), 1)
    order = torch.empty((sector.shape[0],), dtype=torch.int32, device=sector.device)
    tables = torch.empty((5, nseg), dtype=torch.int32, device=sector.device)      # the kernel writes every entry it defines
    _lib.launch("sv_spc_partition", _lib.ptr(sector), _lib.ptr(xyz), _lib.ptr(starts), _lib.ptr(cnt), B, int(num_keypoints), int(num_sectors), _lib.ptr(order),
                _lib.ptr(tables[0]), _lib.ptr(tables[1]), _lib.ptr(tables[2]), _lib.ptr(tables[3]), _lib.ptr(tables[4]))
    return order, tables


def stack_farthest_point_sampling_ragged(xyz, order, seg_start, seg_cnt, seg_m, seg_out_start, idx, max_n=None):
    """One workgroup per segment of the device tables; GLOBAL rows into idx (int32, caller-allocated) at seg_out_start (stack_farthest_point_sampling_
    wrapper, src/sampling.cpp, with the counts left on the device).  order None: segment g is the rows seg_start[g] ... of xyz.  max_n: an upper bound
    of the largest segment known on the host (None: N)."""
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and idx.dtype == torch.int32
    for t in (order, seg_start, seg_cnt, seg_m, seg_out_start):
        assert t is None or t.dtype == torch.int32
    N = xyz.shape[0]
    max_n = N if max_n is None else min(int(max_n), N)
    temp = torch.empty((N,), dtype=torch.float32, device=xyz.device) if max_n > 24576 else None
    _lib.launch("sv_stack_farthest_point_sampling_ragged", _lib.ptr(xyz), N, _lib.ptr(order), _lib.ptr(seg_start), _lib.ptr(seg_cnt), _lib.ptr(seg_m),
                _lib.ptr(seg_out_start), seg_cnt.shape[0], max_n, _lib.ptr(temp), _lib.ptr(idx), idx.numel())
    return idx


def voxel_query_wrapper(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx):
    """src/voxel_query.cpp: new_coords (M, 4) int32 [b, z, y, x], point_indices (B, R1, R2, R3) int32, idx (M, nsample) int32 zero-filled by the caller."""
    assert new_coords.dtype == torch.int32 and point_indices.dtype == torch.int32 and idx.dtype == torch.int32
    cells = int(R1) * int(R2) * int(R3)
    B = point_indices.numel() // cells if cells else 0
    _lib.launch("sv_voxel_query_stack", int(M), B, int(R1), int(R2), int(R3), int(xyz.shape[0]), int(nsample), float(radius), int(z_range), int(y_range),
                int(x_range), _lib.ptr(new_xyz), _lib.ptr(xyz), _lib.ptr(new_coords), _lib.ptr(point_indices), _lib.ptr(idx))
    return 1


def three_interpolate_wrapper(features, idx, weight, out):
    """src/interpolate.cpp three_interpolate_wrapper_stack: features (M, C), idx / weight (N, 3) -> out (N, C), every element written."""
    assert idx.dtype == torch.int32 and features.dtype == weight.dtype == out.dtype == torch.float32
    _lib.launch("sv_three_interpolate_stack", int(idx.shape[0]), int(features.shape[1]), int(features.shape[0]), _lib.ptr(features), _lib.ptr(idx),
                _lib.ptr(weight), _lib.ptr(out))
    return 1


def three_interpolate_grad_wrapper(grad_out, idx, weight, grad_features):
    """src/interpolate.cpp three_interpolate_grad_wrapper_stack: grad_out (N, C) -> grad_features (M, C), every element written (the plain
    route zero-fills and adds with float atomics; the ordered route sums in ascending key 3 r + t)."""
    lib = _lib.load()
    assert idx.dtype == torch.int32 and grad_out.dtype == weight.dtype == grad_features.dtype == torch.float32
    rows, C, n = int(idx.shape[0]), int(grad_out.shape[1]), int(grad_features.shape[0])
    if ordered.ordered_gradients():
        nbytes = lib.sv_three_interpolate_grad_stack_ordered_scratch_bytes(rows, n)
        scratch = _lib.workspace.scratch("three_interp_grad_ordered", nbytes, grad_out.device)
        _lib.launch("sv_three_interpolate_grad_stack_ordered", rows, C, n, _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(scratch),
                    _lib.ptr(grad_features))
        ordered.count_call("three_interpolate")
        return 1
    _lib.launch("sv_three_interpolate_grad_stack", rows, C, n, _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(grad_features))
    return 1


def vector_pool_choice(support_xyz, xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, num_grid_x, num_grid_y, num_grid_z,
                       max_neighbour_distance, num_c_out_each_grid, nsample, neighbor_type):
    """`voxel_random_choice` vector pooling in one launch (seevcn entry; the reference's vector_pool_wrapper sizes grouped_idxs on the host
    and is re-run until it fits).  -> choice (M, G) int32 global support row or -1, point_cnt (M, G) int32, new_local_xyz (M, 3 G),
    new_features (M, G * c_each); all final, nothing is read back."""
    assert support_xyz.dtype == support_features.dtype == new_xyz.dtype == torch.float32
    qs, qc = _starts(new_xyz_batch_cnt)
    ps, pc = _starts(xyz_batch_cnt)
    M, N = int(new_xyz.shape[0]), int(support_xyz.shape[0])
    G = int(num_grid_x) * int(num_grid_y) * int(num_grid_z)
    c_in, c_each = int(support_features.shape[1]), int(num_c_out_each_grid)
    dev = new_xyz.device
    choice = torch.empty((M, G), dtype=torch.int32, device=dev)
    point_cnt = torch.empty((M, G), dtype=torch.int32, device=dev)
    new_local_xyz = torch.empty((M, 3 * G), dtype=torch.float32, device=dev)
    new_features = torch.empty((M, G * c_each), dtype=torch.float32, device=dev)
    _lib.launch("sv_vector_pool_choice", int(qc.shape[0]), M, N, M, _lib.ptr(new_xyz), _lib.ptr(qs), _lib.ptr(qc), _lib.ptr(support_xyz),
                _lib.ptr(support_features), _lib.ptr(ps), _lib.ptr(pc), c_in, c_each, int(num_grid_x), int(num_grid_y), int(num_grid_z),
                float(max_neighbour_distance), int(nsample), int(neighbor_type), _lib.ptr(choice), _lib.ptr(point_cnt), _lib.ptr(new_local_xyz),
                _lib.ptr(new_features))
    return choice, point_cnt, new_local_xyz, new_features


def vector_pool_choice_grad(grad_new_features, choice, point_cnt, N, num_c_in):
    """grad_new_features (M, G * c_each) -> grad_support_features (N, c_in), every element written."""
    lib = _lib.load()
    M, G = int(choice.shape[0]), int(choice.shape[1])
    c_each = int(grad_new_features.shape[1]) // G
    grad_support = torch.empty((int(N), int(num_c_in)), dtype=torch.float32, device=grad_new_features.device)
    if ordered.ordered_gradients():
        nbytes = lib.sv_vector_pool_choice_grad_ordered_scratch_bytes(M, int(N), G)
        scratch = _lib.workspace.scratch("vector_pool_grad_ordered", nbytes, grad_new_features.device)
        _lib.launch("sv_vector_pool_choice_grad_ordered", M, int(N), G, int(num_c_in), c_each, _lib.ptr(grad_new_features), _lib.ptr(choice),
                    _lib.ptr(point_cnt), _lib.ptr(scratch), _lib.ptr(grad_support))
        ordered.count_call("vector_pool")
        return grad_support
    _lib.launch("sv_vector_pool_choice_grad", M, int(N), G, int(num_c_in), c_each, _lib.ptr(grad_new_features), _lib.ptr(choice), _lib.ptr(point_cnt),
                _lib.ptr(grad_support))
    return grad_support


def vector_pool_three_nn(support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt, max_neighbour_distance, nsample,
                         neighbor_type):
    """The local neighbour list and the 3-NN of every grid centre over it in one launch (seevcn entry; the reference's two wrappers pass a
    host-sized stack_neighbor_idxs between them).  -> idx (M, G, 3) int32 global rows or -1, dist2 (M, G, 3) (+inf where idx is -1)."""
    assert support_xyz.dtype == new_xyz.dtype == new_xyz_grid_centers.dtype == torch.float32
    qs, qc = _starts(new_xyz_batch_cnt)
    ps, pc = _starts(xyz_batch_cnt)
    M, N, G = int(new_xyz.shape[0]), int(support_xyz.shape[0]), int(new_xyz_grid_centers.shape[1])
    idx = torch.empty((M, G, 3), dtype=torch.int32, device=new_xyz.device)
    dist2 = torch.empty((M, G, 3), dtype=torch.float32, device=new_xyz.device)
    _lib.launch("sv_vector_pool_three_nn", int(qc.shape[0]), M, N, M, _lib.ptr(new_xyz), _lib.ptr(new_xyz_grid_centers), _lib.ptr(qs), _lib.ptr(qc),
                _lib.ptr(support_xyz), _lib.ptr(ps), _lib.ptr(pc), G, float(max_neighbour_distance), int(nsample), int(neighbor_type), _lib.ptr(idx),
                _lib.ptr(dist2))
    return idx, dist2


def _raising(name, why):
    def stub(*args, **kwargs):
        raise NotImplementedError(f"pointnet2_stack_cuda.{name} is not built: {why}; see INTEGRATION.md 'Unsupported surface'")
    stub.__name__ = name
    return stub


# Names the reference's extension exports (src/pointnet2_api.cpp:12-31) that stay raising.  The vector-pool four take a host-sized buffer and
# return a count for the caller's retry loop -- the contract vector_pool_choice / vector_pool_three_nn above remove; the stacked three_nn
# belongs to StackPointnetFPModule, which no configuration reaches.
_VP = "its host-sized buffer and returned count are replaced by pointnet2_stack_cuda.vector_pool_choice / vector_pool_three_nn"
three_nn_wrapper = _raising("three_nn_wrapper", "the stacked three_nn (StackPointnetFPModule) is outside every built configuration")
vector_pool_wrapper = _raising("vector_pool_wrapper", _VP)
vector_pool_grad_wrapper = _raising("vector_pool_grad_wrapper", _VP)
query_stacked_local_neighbor_idxs_wrapper_stack = _raising("query_stacked_local_neighbor_idxs_wrapper_stack", _VP)
query_three_nn_by_stacked_local_idxs_wrapper_stack = _raising("query_three_nn_by_stacked_local_idxs_wrapper_stack", _VP)
