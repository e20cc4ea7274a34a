"""`pointnet2_batch_cuda` with the reference's wrapper names and argument order
(detector3d/pcdet/ops/pointnet2/pointnet2_batch/src/pointnet2_api.cpp:12-27) over libseevcn_hip.so.

The three gradient wrappers (group_points_grad_wrapper, gather_points_grad_wrapper, three_interpolate_grad_wrapper) add with float atomics by
default; with seevcn_amd.set_ordered_gradients(True) or torch.use_deterministic_algorithms(True) they call the *_batch_ordered entries, which
sum every element in ascending key order (include/seevcn_hip.h).  The switch is read when the wrapper is CALLED, i.e. when the backward runs."""
from ..... import _lib, ordered


def ball_query_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx):
    _lib.launch("sv_ball_query_batch", int(b), int(n), int(m), float(radius), int(nsample), _lib.ptr(new_xyz), _lib.ptr(xyz), _lib.ptr(idx))
    return 1


def group_points_wrapper(b, c, n, npoints, nsample, points, idx, out):
    _lib.launch("sv_group_points_batch", int(b), int(c), int(n), int(npoints), int(nsample), _lib.ptr(points), _lib.ptr(idx), _lib.ptr(out))
    return 1


def _call_ordered(name, counter, sizes, args, device):
    """The order-fixed twin of entry `name`: scratch sized by its *_scratch_bytes(sizes), passed in front of the output pointer."""
    nbytes = getattr(_lib.load(), name + "_scratch_bytes")(*sizes)
    scratch = _lib.workspace.scratch(counter + "_grad_ordered", nbytes, device)
    _lib.launch(name, *args[:-1], _lib.ptr(scratch), args[-1])
    ordered.count_call(counter)
    return 1


def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out, idx, grad_points):
    """grad_points (B,c,n) from grad_out (B,c,npoints,nsample); order-fixed (ascending slot npoints * nsample) when the switch is on"""
    if ordered.ordered_gradients():
        return _call_ordered("sv_group_points_grad_batch_ordered", "group_points_batch", (int(b), int(n), int(npoints), int(nsample)),
                             (int(b), int(c), int(n), int(npoints), int(nsample), _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(grad_points)),
                             grad_out.device)
    _lib.launch("sv_group_points_grad_batch", int(b), int(c), int(n), int(npoints), int(nsample), _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(grad_points))
    return 1


def gather_points_wrapper(b, c, n, npoints, points, idx, out):
    _lib.launch("sv_gather_points_batch", int(b), int(c), int(n), int(npoints), _lib.ptr(points), _lib.ptr(idx), _lib.ptr(out))
    return 1


def gather_points_grad_wrapper(b, c, n, npoints, grad_out, idx, grad_points):
    """grad_points (B,c,n) from grad_out (B,c,npoints); order-fixed (ascending slot) when the switch is on"""
    if ordered.ordered_gradients():
        return _call_ordered("sv_gather_points_grad_batch_ordered", "gather_points_batch", (int(b), int(n), int(npoints)),
                             (int(b), int(c), int(n), int(npoints), _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(grad_points)), grad_out.device)
    _lib.launch("sv_gather_points_grad_batch", int(b), int(c), int(n), int(npoints), _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(grad_points))
    return 1


def farthest_point_sampling_wrapper(b, n, m, points, temp, idx):
    from ..pointnet2_stack import pointnet2_stack_cuda
    return pointnet2_stack_cuda.farthest_point_sampling_wrapper(b, n, m, points, temp, idx)


def three_nn_wrapper(b, n, m, unknown, known, dist2, idx):
    _lib.launch("sv_three_nn_batch", int(b), int(n), int(m), _lib.ptr(unknown), _lib.ptr(known), _lib.ptr(dist2), _lib.ptr(idx))
    return 1


def three_interpolate_wrapper(b, c, m, n, points, idx, weight, out):
    _lib.launch("sv_three_interpolate_batch", int(b), int(c), int(m), int(n), _lib.ptr(points), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(out))
    return 1


def three_interpolate_grad_wrapper(b, c, n, m, grad_out, idx, weight, grad_points):
    """grad_points (B,c,m) from grad_out (B,c,n); order-fixed (ascending key 3 p + t) when the switch is on"""
    if ordered.ordered_gradients():
        return _call_ordered("sv_three_interpolate_grad_batch_ordered", "three_interpolate_batch", (int(b), int(n), int(m)),
                             (int(b), int(c), int(n), int(m), _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(grad_points)),
                             grad_out.device)
    _lib.launch("sv_three_interpolate_grad_batch", int(b), int(c), int(n), int(m), _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(grad_points))
    return 1
