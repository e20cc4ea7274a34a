"""The package-level switch of the order-fixed gradient route.

The scatter-add gradients of the Chamfer loss (sv_chamfer_backward), of the stacked grouping (sv_group_points_grad_stack) and of the SA-MSG
training backward (sv_sa_train_backward) and of the RoI-aware pooling (sv_roiaware_pool_backward), of the stacked three-point interpolation (sv_three_interpolate_grad_stack) and of the
vector-pool choice (sv_vector_pool_choice_grad), and the dense-batch point ops of PointRCNN (sv_group_points_grad_batch, sv_gather_points_grad_batch,
sv_three_interpolate_grad_batch: every PointnetSAModule(MSG) and PointnetFPModule) add with float atomics by default: two runs differ in the last bits.  With the switch on -- or with
torch.use_deterministic_algorithms(True) -- their autograd functions and pybind-shaped wrappers call the *_ordered entries instead, which sum
every element in a stated order.  The switch is read when the BACKWARD runs, not when the graph was built."""
import collections

_flag = False
_calls = collections.Counter()


class _Restore:
    """What set_ordered_gradients returns: leaving a `with` block puts the earlier value back."""

    def __init__(self, previous):
        self.previous = previous

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _flag
        _flag = self.previous
        return False


def set_ordered_gradients(flag):
    """Switch the order-fixed gradient route on or off for the whole process.  Takes effect at once; used as
    `with set_ordered_gradients(True): ...` the earlier value comes back at the end of the block."""
    global _flag
    previous, _flag = _flag, bool(flag)
    return _Restore(previous)


def ordered_gradients():
    """True when the next backward takes the order-fixed route: the switch, or torch's deterministic-algorithms mode."""
    if _flag:
        return True
    import torch
    return torch.are_deterministic_algorithms_enabled()


def ordered_gradient_calls():
    """How often each order-fixed entry has run in this process: {"chamfer": n, "group_points": n, "sa_train": n,
    "roiaware_pool": n, "three_interpolate": n, "vector_pool": n, "group_points_batch": n, "gather_points_batch": n,
    "three_interpolate_batch": n} -- the last three are the dense-batch (B, C, N) entries, the unsuffixed ones the stacked entries."""
    return {k: _calls[k] for k in ("chamfer", "group_points", "sa_train", "roiaware_pool", "three_interpolate", "vector_pool",
                                   "group_points_batch", "gather_points_batch", "three_interpolate_batch")}


def count_call(name):
    _calls[name] += 1
