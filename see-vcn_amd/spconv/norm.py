"""Fused BatchNorm1d(+ReLU) over voxel feature matrices, used by SparseSequential / SparseBasicBlock in place of the separate
torch kernels for the `norm_fn -> ReLU` tail of the reference's post_act_block (spconv_backbone.py:9-27).  The modules stay
plain `nn.BatchNorm1d` / `nn.ReLU` (same state_dict keys, same running-statistics semantics); only the arithmetic moves.
A model converted with `nn.SyncBatchNorm.convert_sync_batchnorm` (the reference's --sync_bn) stays on the same kernels: route() says which
modules exchange their per-channel sums between the ranks (process_group and buffers stay torch's own)."""
import os

import torch
import torch.nn as nn

from .. import _lib


_SCRATCH_BYTES = {}


def _scratch(channels, device):
    n = _SCRATCH_BYTES.get(channels)
    if n is None:
        n = _SCRATCH_BYTES[channels] = _lib.load().sv_batchnorm_scratch_bytes(channels)
    return _lib.workspace.scratch(f"bn{channels}", n, device)


STATS_IN_CONV = os.environ.get("SEEVCN_BN_STATS_IN_CONV", "1") != "0"      # 0: the fused conv + BatchNorm node runs the separate statistics pass (A/B runs)


def partial_address(channels, device):
    """Device address where the producer of a BatchNorm input leaves its partial sums: behind the 4 * C coefficient floats of the norm's scratch."""
    return _scratch(channels, device).data_ptr() + 16 * channels


def bn_forward_raw(x, gamma, beta, running_mean, running_var, momentum, eps, training, relu, num_batches_tracked=None, n_partials=0):
    """y, save_mean, save_invstd (the last two None in eval mode) of the fused BatchNorm(+ReLU) forward on a contiguous (N, C) matrix.  n_partials > 0:
    the statistics' first pass is already in the scratch (partial_address), written by the kernel that produced x."""
    n, c = x.shape
    y = torch.empty_like(x)
    if training:
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        invstd = torch.empty(c, dtype=torch.float32, device=x.device)
    else:
        mean = invstd = None
    if training and n_partials:
        _lib.launch("sv_batchnorm_relu_forward_partial", _lib.ptr(x), n, c, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(running_mean), _lib.ptr(running_var),
                    float(momentum), float(eps), int(relu), _lib.ptr(_scratch(c, x.device)), int(n_partials), _lib.ptr(y), _lib.ptr(mean), _lib.ptr(invstd),
                    _lib.ptr(num_batches_tracked))
        return y, mean, invstd
    _lib.launch("sv_batchnorm_relu_forward", _lib.ptr(x), n, c, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(running_mean), _lib.ptr(running_var), float(momentum),
                float(eps), int(training), int(relu), _lib.ptr(_scratch(c, x.device)), _lib.ptr(y), _lib.ptr(mean), _lib.ptr(invstd),
                _lib.ptr(num_batches_tracked))
    return y, mean, invstd


def bn_backward_raw(x, dy, gamma, beta, mean, invstd, relu):
    """dx, dgamma, dbeta of the training-mode fused BatchNorm(+ReLU); x is the BatchNorm INPUT (the ReLU mask is recomputed from it)."""
    n, c = x.shape
    dx = torch.empty_like(x)
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    _lib.launch("sv_batchnorm_relu_backward", _lib.ptr(x), _lib.ptr(dy), n, c, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean), _lib.ptr(invstd), int(relu),
                _lib.ptr(_scratch(c, x.device)), _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta))
    return dx, dgamma, dbeta


PLAIN, SYNCED = "plain", "synced"
# smallest world size that takes the synced route.  torch's SyncBatchNorm exchanges nothing in a world of one (it falls back to F.batch_norm) and so does the
# plain route here; tests and measurements set this to 1 to drive the cut lists and the exchange with a single rank.
MIN_SYNC_WORLD = 2


def route(bn, subclasses=False):
    """How the fused kernels take a norm module: PLAIN (nn.BatchNorm1d; subclasses=True: or a subclass of it), SYNCED (exactly torch.nn.SyncBatchNorm
    in training mode with torch.distributed initialised and more than one rank in its process group: the per-channel sums are exchanged between the
    ranks in the middle of the combine), or None (the module runs as it is).  A SyncBatchNorm in eval mode, or in a world of one, computes what
    BatchNorm1d computes (torch falls back to F.batch_norm there): PLAIN."""
    if type(bn) is nn.BatchNorm1d or (subclasses and isinstance(bn, nn.BatchNorm1d)):
        return PLAIN
    if type(bn) is not nn.SyncBatchNorm:
        return None
    if bn.training and sync_world(bn) >= MIN_SYNC_WORLD:
        return SYNCED
    return PLAIN


def sync_world(bn):
    """Number of ranks a SyncBatchNorm exchanges its statistics with (its process_group, or the default group); 0 without torch.distributed."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    return dist.get_world_size(bn.process_group)


def exchange(local, gathered, group=None):
    """All-gather of a rank's fp64 sums `local` (m,) into `gathered` (world, m), rank-major, on the current stream like any torch collective.  All-gather and
    not all-reduce, in both directions: the kernels add the ranks in rank order, so every rank gets the same bits whatever the backend's reduction order."""
    import torch.distributed as dist
    if dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(gathered.view(-1), local, group=group)
    else:                                                                            # gloo has no all_gather_into_tensor for device tensors
        dist.all_gather(list(gathered.unbind(0)), local, group=group)


def sync_buffers(bn, channels, device, backward=False):
    """-> (local (m,), gathered (world, m), group) fp64 buffers of one exchange of `bn`: m = 2 C + 1 forward (sums | sums of squares | row count), 2 C backward."""
    world, m = sync_world(bn), 2 * channels + (0 if backward else 1)
    buf = torch.empty(((world + 1) * m,), dtype=torch.float64, device=device)
    return buf[:m], buf[m:].view(world, m), bn.process_group


def bn_forward_synced(x, bn, relu, n_partials=0):
    """y, save_mean, save_invstd, total_rows of a SYNCED norm on a contiguous (N, C) matrix: this rank's sums (from x, or from the n_partials partials
    its producer left in the scratch), the exchange, the combine over all ranks, the elementwise pass."""
    n, c = x.shape
    dev = x.device
    local, gathered, group = sync_buffers(bn, c, dev)
    _lib.launch("sv_batchnorm_stats_local", None if n_partials else _lib.ptr(x), n, c, _lib.ptr(_scratch(c, dev)), int(n_partials), _lib.ptr(local))
    exchange(local, gathered, group)
    stats = torch.empty(4 * c, dtype=torch.float32, device=dev)                      # scale | shift | batch mean | batch invstd
    total = torch.empty(1, dtype=torch.float64, device=dev)
    mean, invstd = stats[2 * c:3 * c], stats[3 * c:]
    rs = bn.track_running_stats
    _lib.launch("sv_batchnorm_finalize_global", _lib.ptr(gathered), gathered.shape[0], c, _lib.ptr(bn.weight), _lib.ptr(bn.bias),
                _lib.ptr(bn.running_mean if rs else None), _lib.ptr(bn.running_var if rs else None), float(bn.momentum), float(bn.eps), _lib.ptr(stats),
                _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(bn.num_batches_tracked if rs else None), _lib.ptr(total))
    y = torch.empty_like(x)
    _lib.launch("sv_batchnorm_apply", _lib.ptr(x), n, c, _lib.ptr(stats), int(relu), _lib.ptr(y))
    return y, mean, invstd, total


def bn_backward_synced(x, dy, bn, gamma, beta, mean, invstd, total, relu):
    """dx, dgamma, dbeta of a SYNCED norm: this rank's two sums, the exchange, the elementwise pass with the sums and the row count of all ranks.
    dgamma / dbeta are this rank's own sums (the data-parallel wrapper averages them like any other parameter gradient)."""
    n, c = x.shape
    dev = x.device
    dx = torch.empty_like(x)
    dgb = torch.empty(2 * c, dtype=torch.float32, device=dev)
    local, gathered, group = sync_buffers(bn, c, dev, backward=True)
    scratch = _scratch(c, dev)
    _lib.launch("sv_batchnorm_backward_sums_local", _lib.ptr(x), _lib.ptr(dy), n, c, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean), _lib.ptr(invstd),
                int(relu), _lib.ptr(scratch), 0, _lib.ptr(dgb), dgb.data_ptr() + 4 * c, _lib.ptr(local))
    exchange(local, gathered, group)
    _lib.launch("sv_batchnorm_backward_apply_global", _lib.ptr(x), _lib.ptr(dy), n, c, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean), _lib.ptr(invstd),
                int(relu), _lib.ptr(gathered), gathered.shape[0], _lib.ptr(total), _lib.ptr(scratch), _lib.ptr(dx))
    return dx, dgb[:c], dgb[c:]


class _BatchNormReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, training, relu, num_batches_tracked=None, sync_bn=None):
        x = x.contiguous()
        ctx.sync_bn, total = sync_bn, None
        if sync_bn is not None:                                                       # SYNCED: the module carries the process group and the buffers
            y, mean, invstd, total = bn_forward_synced(x, sync_bn, relu)
        else:
            y, mean, invstd = bn_forward_raw(x, gamma, beta, running_mean, running_var, momentum, eps, training, relu, num_batches_tracked)
        ctx.relu, ctx.training = relu, training
        ctx.save_for_backward(x, gamma, beta, mean, invstd, total)
        return y

    @staticmethod
    def backward(ctx, dy):
        assert ctx.training, "fused BatchNorm backward is only defined for training mode"
        x, gamma, beta, mean, invstd, total = ctx.saved_tensors
        if ctx.sync_bn is not None:
            dx, dgamma, dbeta = bn_backward_synced(x, dy.contiguous(), ctx.sync_bn, gamma, beta, mean, invstd, total, ctx.relu)
        else:
            dx, dgamma, dbeta = bn_backward_raw(x, dy.contiguous(), gamma, beta, mean, invstd, ctx.relu)
        return dx, (dgamma if gamma is not None else None), (dbeta if beta is not None else None), None, None, None, None, None, None, None, None


def channels_fusable(c):
    return 4 <= c <= 512 and c % 4 == 0 and 256 % (c // 4) == 0


def fusable(bn, x):
    return (route(bn, subclasses=True) is not None and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] > 0
            and channels_fusable(x.shape[1]) and bn.momentum is not None
            and (bn.training or bn.track_running_stats) and (not x.requires_grad or bn.training))


def batch_norm_relu(bn, x, relu):
    """y = [relu](bn(x)) with bn an nn.BatchNorm1d (training or eval) or a torch.nn.SyncBatchNorm (see route()), x (N,C) float32 CUDA."""
    training = bn.training or not bn.track_running_stats
    synced = route(bn, subclasses=True) == SYNCED
    if training and x.shape[0] == 1 and not synced:                                   # SYNCED: the other ranks bring the second value (torch checks the total)
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    nbt = bn.num_batches_tracked if (training and bn.track_running_stats) else None   # incremented inside the kernel chain
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    return _BatchNormReLU.apply(x, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps, training, relu, nbt, bn if synced else None)
