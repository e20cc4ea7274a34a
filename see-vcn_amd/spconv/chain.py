"""Chains of sparse conv blocks over the launch-list executor (sv_run_ops, csrc/sequencer.hip): the training step of a [sparse conv -> BatchNorm1d ->
ReLU] chain as ONE autograd node, and the eval-mode forward of both 3-D backbones as one list without an autograd node.

The reference's VoxelBackBone8x.forward (detector3d/pcdet/models/backbones_3d/spconv_backbone.py:128-180) is 12 such blocks; through the module
tree each block costs the host an autograd node, three output allocations and two or three ctypes calls per direction (2.2 ms of Python per
step for 4.0 ms of GPU time on the bench workload).  Here the forward of the whole chain is written as one list of operations -- every
argument is known before the first kernel runs: the rulebooks and plans are built ahead, the activations are slices of one allocation -- and
enqueued with one call; the backward (BatchNorm backward, weight gradient, data gradient per block, last to first) likewise.  Same kernels,
same arithmetic, same parameters and running statistics as the per-module path (SparseSequential), which stays the fallback for anything
this does not take (hooks, a conv bias or residual blocks in training mode, a layer without a plan for its data gradient).

Eval mode (eval_applicable / run_eval_chain; tools/test.py of the reference, the post_processing + recall path): the list is one
launch that makes every BatchNorm's (scale, shift) from its running statistics (SV_OP_BN_EVAL_COEF_BATCH) and one convolution per layer whose
epilogue applies conv bias, folded BatchNorm, the identity of a residual block (SparseBasicBlock, spconv_backbone.py:30-66) and the ReLU -- every
activation is written once, normalised.  It stands down (module tree) when gradients are enabled, a norm is in training mode or keeps no running
statistics, the input is empty, anything walked carries a hook, a residual block has a downsample module or a forward of its own, or SEEVCN_CHAIN=0 /
SEEVCN_EVAL_CHAIN=0.
A second form of the same list runs the layers behind the input layer on fp16 activations and fp16 weight fragments with fp32 arithmetic
(eval_half_applicable / run_eval_chain(dtype=torch.float16), csrc/sparse_conv_half.hip); a backbone takes it only when asked (EVAL_DTYPE / set_eval_dtype).

Both routes read ONE description of the network: flatten() -> BlockList of Entry, one per convolution (applicable() declines for training what only
the eval list carries: a residual identity, a conv bias).  Every row of a list is made by the constructor of its operation code (CONV_PLANNED ...
BN_EVAL_COEF_BATCH below): the only place that knows which word of the row a field of include/seevcn_hip.h is."""
from collections import namedtuple
from functools import partial
import os
import struct

import numpy as np
import torch

from .. import _lib
from . import functional as Fsp
from . import norm
from .core import SparseConvTensor

CHAIN_OFF = os.environ.get("SEEVCN_CHAIN", "1") == "0"          # 0: every block through its own modules (A/B runs, tests)
# 1 (default since round 5): a BatchNorm backward takes its two per-channel sums from the epilogue of the data-gradient launch above it
# (sv_sparse_conv_dgrad_planned_bn) instead of reducing them in a pass of its own.  Round 3 built it and measured 5.13-5.26 ms without, 5.26-5.56 ms with
# (the 11 saved reduce launches were paid back by the epilogues' 16 extra row reads per tile on a chain that was waiting for its weight gradients anyway);
# with the weight gradients on their own stream the data-gradient chain IS the critical path and the saved launches count: 3.70 -> 3.63 ms (same box, two
# alternations).  The sums are added in plan order instead of row order: gradients equal the separate pass to 1e-5 of each tensor's largest entry, and
# are reproducible run to run (one plan per table, fixed partial slots); 0 restores bit-identity with the per-module path.
BWD_SUMS_IN_CONV = os.environ.get("SEEVCN_BN_BWD_IN_CONV", "1") != "0"
# 0: every weight gradient is followed by its own slab-reduction launch (SV_OP_WGRAD) instead of ONE reduction launch for all layers at the end of the backward
# list (SV_OP_WGRAD_DEFERRED: bitwise the same gradients) -- A/B runs
DEFER_WGRAD_REDUCE = os.environ.get("SEEVCN_WGRAD_DEFER", "1") != "0"
# 1 (default since round 5): the weight gradients of the backward list on a stream of their own (sv_run_ops_two_streams), each behind the BatchNorm backward that
# makes its operand; the main chain (data gradient -> next BatchNorm backward -> ...) does not wait for them until the end of the list.  Their matrix-core work
# fills the bandwidth-bound BatchNorm launches and the prologues / tails of the data-gradient launches.  Round 4 measured the trained side alone 3.16 -> 3.06 ms
# but the pipelined step 4.07-4.19 -> 4.3-4.4 ms (a third stream on a GPU the one-stage input side kept busy) and left it off; with round 5's two-stage
# prefetch and shorter forward the same switch takes the step from 3.92 to 3.73 ms (same box, two alternations: profiles/r05_wstream_ab.txt).  0: one stream.
WGRAD_STREAM = os.environ.get("SEEVCN_WGRAD_STREAM", "1") != "0"
_wgrad_stream = {}
# 1 (default): the BatchNorm + ReLU behind a conv is NOT applied in a pass of its own -- the block keeps the raw conv output and the norm's (scale, shift), and the
# next block's convolution and weight gradient apply them as they gather the rows (sv_conv_next_input_norm): one read + one write of every activation
# tensor and one launch per block less; the values a consumer sees are bit for bit those of the separate pass.  Tensors that leave the chain (taps) are
# made when somebody reads them (LazyTap), the last block's in the list.  0: every block writes its normalised output (A/B runs, tests).
BN_FOLD = os.environ.get("SEEVCN_BN_FOLD", "1") != "0"
# 0: an eval-mode backbone forward walks the module tree (conv, BatchNorm coefficients and the elementwise pass as launches of their own) instead of
# running as one launch list with the BatchNorms folded into the convs' epilogues (run_eval_chain) -- A/B runs, tests.  Bitwise the same outputs.
EVAL_CHAIN_OFF = os.environ.get("SEEVCN_EVAL_CHAIN", "1") == "0"
OP_CONV_PLANNED, OP_CONV_PLAIN, OP_BN_FWD, OP_BN_BWD, OP_WGRAD, OP_DGRAD_PLANNED_BN, OP_WGRAD_DEFERRED, OP_BN_FINALIZE, OP_BN_APPLY = 1, 2, 3, 5, 6, 7, 8, 9, 10
OP_BN_STATS_LOCAL, OP_BN_FINALIZE_GLOBAL, OP_BN_BWD_SUMS_LOCAL, OP_BN_BWD_APPLY_GLOBAL, OP_BN_EVAL_COEF_BATCH = 11, 12, 13, 14, 15
OP_CONV_PLANNED_H16, OP_NARROW_H16 = 16, 17
WORDS = 32


def _bits(x):
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


def _row(code, i=(), n=(), f=(), p=()):
    r = [0] * WORDS
    r[0] = code
    r[1:1 + len(i)] = [int(v) for v in i]
    r[9:9 + len(n)] = [int(v) for v in n]
    r[13:13 + len(f)] = f
    r[17:17 + len(p)] = [0 if v is None else int(v) for v in p]
    return r


# One constructor per operation code: keyword arguments named like the fields of the executor's header comment (include/seevcn_hip.h), pointers as device
# addresses (None = null).  `plan` is the tuple of Rulebook.plan_addrs: (table_rows, perm, masks_p, tile_of, tiles_per_wave, table_k_reversed); mom_eps
# the bit patterns of (momentum, eps) (Entry.mom_eps).  in_coef / in_relu: the input transform (X is the raw conv output of the layer below).
def CONV_PLANNED(plan, *, X, n_src, wfrag, Y, n_rows, K, Kd, Nc, relu=0, bias=None, scale=None, shift=None, residual=None, bn_partial=None, in_coef=None,
                 in_relu=0):
    table_rows, perm, masks_p, tile_of, tiles_per_wave, table_k_reversed = plan
    return _row(OP_CONV_PLANNED, i=(tiles_per_wave, K, Kd, Nc, relu, bool(table_k_reversed), in_relu), n=(n_src, n_rows),
                p=(X, table_rows, perm, masks_p, tile_of, wfrag, Y, bias, scale, shift, residual, bn_partial, in_coef))


def CONV_PLAIN(*, X, n_src, nbr, Wt, Y, n_rows, K, Kd, Nc, relu=0, bias=None, scale=None, shift=None, residual=None):
    return _row(OP_CONV_PLAIN, i=(K, Kd, Nc, relu), n=(n_src, n_rows), p=(X, nbr, Wt, Y, bias, scale, shift, residual))


def DGRAD_PLANNED_BN(plan, *, dZ, n_src, wfrag, dY, n_rows, K, Kd, Nc, bn_x, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_partial, bn_relu):
    table_rows, perm, masks_p, tile_of, tiles_per_wave, table_k_reversed = plan
    return _row(OP_DGRAD_PLANNED_BN, i=(tiles_per_wave, K, Kd, Nc, bool(table_k_reversed), bn_relu), n=(n_src, n_rows),
                p=(dZ, table_rows, perm, masks_p, tile_of, wfrag, dY, bn_x, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_partial))


def WGRAD(*, X, n_src, nbr, dY, n_rows, dW, scratch, K, Cin, Cout, stride_k, stride_cin, stride_cout, plan=None, in_coef=None, in_relu=0, code=OP_WGRAD):
    return _row(code, i=(K, Cin, Cout, n_src, in_relu), n=(n_rows, stride_k, stride_cin, stride_cout), p=(X, nbr, dY, dW, scratch, plan, in_coef))


WGRAD_DEFERRED = partial(WGRAD, code=OP_WGRAD_DEFERRED)          # the same fields; `scratch` is the layer's OWN partial region


def BN_FWD(*, x, rows, channels, gamma, beta, running_mean, running_var, mom_eps, scratch, y, save_mean, save_invstd, num_batches_tracked, training, relu,
           n_partials=0):
    return _row(OP_BN_FWD, i=(channels, training, relu, n_partials), n=(rows,), f=mom_eps,
                p=(x, gamma, beta, running_mean, running_var, scratch, y, save_mean, save_invstd, num_batches_tracked))


def BN_FINALIZE(*, x, rows, channels, gamma, beta, running_mean, running_var, mom_eps, scratch, coef, save_mean, save_invstd, num_batches_tracked,
                n_partials=0):
    return _row(OP_BN_FINALIZE, i=(channels, n_partials), n=(rows,), f=mom_eps,
                p=(gamma, beta, running_mean, running_var, scratch, coef, save_mean, save_invstd, num_batches_tracked, x))


def BN_APPLY(*, x, rows, channels, coef, relu, y):
    return _row(OP_BN_APPLY, i=(channels, relu), n=(rows,), p=(x, coef, y))


def BN_STATS_LOCAL(*, x, rows, channels, scratch, sums, n_partials=0):
    return _row(OP_BN_STATS_LOCAL, i=(channels, n_partials), n=(rows,), p=(x, scratch, sums))


def BN_FINALIZE_GLOBAL(*, gathered, world, channels, gamma, beta, running_mean, running_var, mom_eps, coef, save_mean, save_invstd, num_batches_tracked,
                       total_rows):
    return _row(OP_BN_FINALIZE_GLOBAL, i=(channels, world), f=mom_eps,
                p=(gathered, gamma, beta, running_mean, running_var, coef, save_mean, save_invstd, num_batches_tracked, total_rows))


def BN_BWD(*, x, dy, rows, channels, gamma, beta, save_mean, save_invstd, relu, scratch, dx, dgamma, dbeta, n_partials=0):
    return _row(OP_BN_BWD, i=(channels, relu, n_partials), n=(rows,), p=(x, dy, gamma, beta, save_mean, save_invstd, scratch, dx, dgamma, dbeta))


def BN_BWD_SUMS_LOCAL(*, x, dy, rows, channels, gamma, beta, save_mean, save_invstd, relu, scratch, dgamma, dbeta, sums, n_partials=0):
    return _row(OP_BN_BWD_SUMS_LOCAL, i=(channels, relu, n_partials), n=(rows,),
                p=(x, dy, gamma, beta, save_mean, save_invstd, scratch, dgamma, dbeta, sums))


def BN_BWD_APPLY_GLOBAL(*, x, dy, rows, channels, gamma, beta, save_mean, save_invstd, relu, scratch, gathered, world, total_rows, dx):
    return _row(OP_BN_BWD_APPLY_GLOBAL, i=(channels, relu, world), n=(rows,),
                p=(x, dy, gamma, beta, save_mean, save_invstd, scratch, gathered, total_rows, dx))


def BN_EVAL_COEF_BATCH(*, jobs_host, n_jobs):
    return _row(OP_BN_EVAL_COEF_BATCH, i=(n_jobs,), p=(jobs_host,))                  # the job table is HOST memory, read before the list's call returns


def CONV_PLANNED_H16(plan, *, X16, n_src, wfrag16, Y, y_is_f32, n_rows, K, Kd, Nc, relu=0, bias=None, scale=None, shift=None, residual16=None):
    table_rows, perm, masks_p = plan[:3]                                             # the fp16 kernel walks perm itself: no tile_of, no tiles_per_wave
    return _row(OP_CONV_PLANNED_H16, i=(K, Kd, Nc, relu, bool(y_is_f32)), n=(n_src, n_rows),
                p=(X16, table_rows, perm, masks_p, wfrag16, Y, bias, scale, shift, residual16))


def NARROW_H16(*, x_f32, n_elems, y_f16):
    return _row(OP_NARROW_H16, n=(n_elems,), p=(x_f32, y_f16))


def _run(rows, what):
    """Run one launch list; `what` names the list for the measurement tools that stand in for this function."""
    arr = np.array(rows, dtype=np.int64)
    _lib.launch("sv_run_ops", arr.ctypes.data, len(rows))


def _run_two_streams(rows, dev):
    """The backward list with its weight gradients on a second stream (sv_run_ops_two_streams): the chain's data gradients and BatchNorm backwards do not
    wait for them; the current stream is ordered behind the side stream when the call returns."""
    side = _wgrad_stream.get(dev)
    if side is None:
        # SEEVCN_WGRAD_STREAM_PRIORITY (A/B): priority of the weight gradients' stream (torch: lower number = served first; default 0 = the main stream's)
        side = _wgrad_stream[dev] = torch.cuda.Stream(dev, priority=int(os.environ.get("SEEVCN_WGRAD_STREAM_PRIORITY", "0")))
    arr = np.array(rows, dtype=np.int64)
    _lib.check(_lib.load().sv_run_ops_two_streams(arr.ctypes.data, len(rows), _lib.stream(), side.cuda_stream), "sv_run_ops_two_streams (chain backward)")


class Cut:
    """A place where a launch list is cut: the rows in front run, the ranks exchange a synced norm's per-channel sums (norm.exchange), the rows behind run."""

    def __init__(self, local, gathered, group):
        self.local, self.gathered, self.group = local, gathered, group


def _run_cut(rows, run):
    """run(segment) for every run of rows between the Cuts of `rows`, the exchange of each Cut in between.  A list without a Cut is one call with all its rows."""
    seg = []
    for r in rows:
        if isinstance(r, Cut):
            run(seg)
            norm.exchange(r.local, r.gathered, r.group)
            seg = []
        else:
            seg.append(r)
    if seg:
        run(seg)


class Entry:
    """One convolution of a chain and what follows it: (conv, bn, relu, residual_from, tap); the modules keep their parameters and running statistics.
    residual_from: index of the entry whose output is added before the ReLU (a residual block's identity), -1 for the chain's input, None for none;
    tap: the output is returned by the chain."""
    __slots__ = ("conv", "bn", "relu", "residual_from", "tap", "K", "cin", "cout")

    def __init__(self, conv, bn, relu, residual_from, tap):
        self.conv, self.bn, self.relu, self.residual_from, self.tap = conv, bn, bool(relu), residual_from, tap
        self.K = conv.kernel_size[0] * conv.kernel_size[1] * conv.kernel_size[2]
        self.cin, self.cout = conv.in_channels, conv.out_channels

    def __iter__(self):
        return iter((self.conv, self.bn, self.relu, self.residual_from, self.tap))

    @property
    def mom_eps(self):
        # read when a training list is made, i.e. after applicable() -> fusable_with() has rejected momentum=None (cumulative average)
        return (_bits(self.bn.momentum), _bits(self.bn.eps))


class BlockList(list):
    """The entries of a chain + every module the flattening walked over (stage containers, nested SparseSequentials, residual blocks, convs, norms,
    ReLUs): the chain bypasses __call__ of ALL of them, so a hook on any of them must send the forward back to the module tree."""
    walked = ()


def _has_hooks(m):
    return bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, '_backward_pre_hooks', None))


_residual_blocks = []


def register_residual_block(cls):
    """cls: a residual block class (SparseBasicBlock) whose OWN forward is relu(bn2(conv2(relu(bn1(conv1(x))))) + x) when its downsample is None;
    flatten takes instances whose forward is that very function (a subclass with a forward of its own is declined)."""
    if cls not in _residual_blocks:
        _residual_blocks.append(cls)
    return cls


def _is_residual_block(m):
    from .conv import SparseConvolution
    if not any(isinstance(m, cls) and type(m).forward is cls.forward for cls in _residual_blocks):
        return False
    c1, c2 = getattr(m, "conv1", None), getattr(m, "conv2", None)
    return (isinstance(c1, SparseConvolution) and isinstance(c2, SparseConvolution) and c1.subm and c2.subm and c1.indice_key is not None
            and c1.indice_key == c2.indice_key and c1.kernel_size == c2.kernel_size and c1.in_channels == c2.out_channels
            and c1.out_channels == c2.in_channels and getattr(m, "downsample", 0) is None and type(getattr(m, "relu", None)) is torch.nn.ReLU
            and norm.route(getattr(m, "bn1", None)) is not None and norm.route(getattr(m, "bn2", None)) is not None)


def flatten(stages):
    """stages: the backbone's stages in execution order (SparseSequential each).  -> BlockList of Entry, one per convolution, or None when a stage is
    anything but (SparseConvolution [with or without bias], BatchNorm1d | SyncBatchNorm, ReLU) triples and registered residual blocks without a
    downsample.  The last entry of every stage is a tap."""
    from .conv import SparseConvolution
    from .modules import SparseSequential
    entries = BlockList()
    walked = []

    def walk(m, out):
        walked.append(m)
        for child in m._modules.values():
            if isinstance(child, SparseSequential):
                walk(child, out)
            else:
                walked.append(child)
                out.append(child)

    for stage in stages:
        if not isinstance(stage, SparseSequential):
            return None
        mods = []
        walk(stage, mods)
        j, n0 = 0, len(entries)
        while j < len(mods):
            m = mods[j]
            if isinstance(m, SparseConvolution):
                if m.inverse:
                    return None                                                     # no launch-list rows for a mirrored table: module tree
                if j + 2 >= len(mods) or norm.route(mods[j + 1]) is None or type(mods[j + 2]) is not torch.nn.ReLU:
                    return None
                entries.append(Entry(m, mods[j + 1], True, None, False))
                j += 3
            elif _is_residual_block(m):
                walked.extend(c for c in m._modules.values() if c is not None)      # a downsample set and cleared again stays registered as None
                identity = len(entries) - 1                                         # -1: the block reads the chain's input
                entries.append(Entry(m.conv1, m.bn1, True, None, False))
                entries.append(Entry(m.conv2, m.bn2, True, identity, False))
                j += 1
            else:
                return None
        if len(entries) == n0:
            return None
        entries[-1].tap = True
    entries.walked = tuple(walked)
    return entries


def applicable(blocks, x):
    """The chain takes these blocks on x now: training with gradients on, fp32 CUDA features, no residual identity, every block what fusable_with()
    accepts, no hooks, every rulebook in x's indice_dict (prebuild_rulebooks ran) with at least two output rows, and a planned data-gradient kernel
    for every block behind the first (the first one's is needed only when the input features want a gradient, which the backbone's never do)."""
    if CHAIN_OFF or blocks is None or not torch.is_grad_enabled() or x.features.requires_grad or x.indices.shape[0] < 2:
        return False
    if any(b.residual_from is not None for b in blocks):
        return False               # a residual block's identity: only the eval list adds it (a conv bias is declined by fusable_with below)
    if any(_has_hooks(m) for m in getattr(blocks, 'walked', ())):
        return False               # a forward / pre-forward / backward hook on a stage, a nested sequential, a conv, a norm or a ReLU: module path
    for k, b in enumerate(blocks):
        if not b.conv.fusable_with(b.bn, x) or b.conv.indice_key is None:
            return False
        rb = x.indice_dict.get(b.conv.indice_key)
        if rb is None or rb.n_out < 2 or rb.ksize != b.conv.kernel_size:
            return False
        if k > 0 and rb.plan_addrs("bwd", b.cout, b.cin) is None:
            return False
    return True


class _TapApply(torch.autograd.Function):
    """The normalised output of a chain block made on demand from its raw conv output: y = [relu](x * scale + shift) (sv_batchnorm_apply: the forward's
    own elementwise pass).  For autograd it is the identity: the chain's backward runs that block's BatchNorm backward itself, with whatever gradient
    arrives here as the gradient w.r.t. y."""

    @staticmethod
    def forward(ctx, raw, coef, relu):
        y = torch.empty_like(raw)
        _lib.launch("sv_batchnorm_apply", _lib.ptr(raw), raw.shape[0], raw.shape[1], _lib.ptr(coef), int(relu), _lib.ptr(y))
        return y

    @staticmethod
    def backward(ctx, g):
        return g, None, None


def fold_plan(blocks, rulebooks):
    """-> (fold_in, materialize): fold_in[k]: block k reads block k-1's RAW conv output through that block's BatchNorm coefficients (its conv runs on a
    plan and its weight gradient on an MFMA tile shape: the kernels that carry the transform); materialize[k]: block k writes its normalised output in
    the list (the last block, and a block whose successor cannot fold)."""
    L = len(blocks)
    fold_in = [False] * L
    if BN_FOLD:
        for k in range(1, L):
            b, rb = blocks[k], rulebooks[k]
            fold_in[k] = rb.plan_addrs("fwd", b.cin, b.cout) is not None and b.cin % 16 == 0 and b.cout % 16 == 0
    materialize = [k == L - 1 or not fold_in[k + 1] for k in range(L)]
    return fold_in, materialize


# where a block's pieces lie in the chain's allocations (offsets in floats; _addresses(): the same record as device addresses).  Forward arena per block:
# [conv output | block output (when it is written at all) | batch mean | batch invstd | scale | shift]; backward work buffer per block: [gradient of the
# conv output | gradient of the block's input (blocks >= 1) | dgamma | dbeta]
_Forward = namedtuple("_Forward", "conv y mean istd coef")
_Backward = namedtuple("_Backward", "dconv dx dgamma dbeta")


def _addresses(base, offs):
    return offs._make(base + 4 * v for v in offs)


def _conv_row(e, rb, keep, X, n_src, Y, bn_partial=None, in_coef=None, in_relu=0, **epilogue):
    """-> (row, backward fragments, planned) of entry e's forward convolution X (n_src rows) -> Y on rulebook rb: on the table's plan with the weights in
    fragment order when the MFMA kernel takes the layer (planned), else (backward fragments None) the plain kernel on a (K, C_out, C_in) copy of the weights that `keep`
    holds until the list has run: the 3/4/5-channel input layer only.  epilogue: relu, bias, scale, shift, residual.  Only the planned kernel writes
    bn_partial and reads its input through in_coef."""
    wk = e.conv.weight_kio_nograd()
    plan = rb.plan_addrs("fwd", e.cin, e.cout)
    if plan is not None:
        wfrag, frag_bwd = Fsp.fragment_cache.get(wk)
        return CONV_PLANNED(plan, X=X, n_src=n_src, wfrag=wfrag.data_ptr(), Y=Y, n_rows=rb.n_out, K=e.K, Kd=e.cin, Nc=e.cout, bn_partial=bn_partial,
                            in_coef=in_coef, in_relu=in_relu, **epilogue), frag_bwd, True
    assert in_coef is None
    wt = wk.detach().permute(0, 2, 1).contiguous()
    keep.append(wt)
    return CONV_PLAIN(X=X, n_src=n_src, nbr=rb.addr("nbr_out"), Wt=wt.data_ptr(), Y=Y, n_rows=rb.n_out, K=e.K, Kd=e.cin, Nc=e.cout, **epilogue), None, False


def _bn_forward_rows(e, a, rows, gamma, beta, n_partials, materialize, total_rows):
    """The rows of a block's BatchNorm in the training forward.  a: the block's arena addresses; n_partials: the conv in front left that many partial sums
    in the norm's scratch (norm.partial_address; 0: the statistics read a.conv); total_rows: where a SYNCED norm (norm.route) keeps the row count of all ranks -- its list is
    cut behind this rank's sums, the ranks exchange them, the next list starts with the combine over all ranks."""
    bn, dev = e.bn, gamma.device
    x = None if n_partials else a.conv
    scratch = norm._scratch(e.cout, dev).data_ptr()
    stats = dict(channels=e.cout, gamma=gamma.data_ptr(), beta=beta.data_ptr(), running_mean=bn.running_mean.data_ptr(), running_var=bn.running_var.data_ptr(),
                 mom_eps=e.mom_eps, save_mean=a.mean, save_invstd=a.istd, num_batches_tracked=bn.num_batches_tracked.data_ptr())
    if total_rows is not None:
        local, gathered, group = norm.sync_buffers(bn, e.cout, dev)
        out = [BN_STATS_LOCAL(x=x, rows=rows, channels=e.cout, scratch=scratch, sums=local.data_ptr(), n_partials=n_partials), Cut(local, gathered, group),
               BN_FINALIZE_GLOBAL(gathered=gathered.data_ptr(), world=gathered.shape[0], coef=a.coef, total_rows=total_rows, **stats)]
    elif BN_FOLD:
        out = [BN_FINALIZE(x=x, rows=rows, scratch=scratch, coef=a.coef, n_partials=n_partials, **stats)]
    else:                                                                             # statistics, normalisation and ReLU in one operation
        return [BN_FWD(x=a.conv, rows=rows, scratch=scratch, y=a.y, training=1, relu=e.relu, n_partials=n_partials, **stats)]
    if materialize:
        out.append(BN_APPLY(x=a.conv, rows=rows, channels=e.cout, coef=a.coef, relu=e.relu, y=a.y))
    return out


def _bn_backward_rows(e, a, w, rows, dy, gamma, beta, n_partials, total_rows):
    """The rows of a block's BatchNorm in the backward.  a / w: the block's addresses in the forward arena / the backward work buffer; n_partials: the
    data-gradient launch above left that many partial sums (0: the reduce pass over x, dy runs first); total_rows: as in the forward (SYNCED: this rank's
    two sums | exchange | the elementwise pass with everybody's)."""
    dev = gamma.device
    common = dict(x=a.conv, dy=dy, rows=rows, channels=e.cout, gamma=gamma.data_ptr(), beta=beta.data_ptr(), save_mean=a.mean, save_invstd=a.istd,
                  relu=e.relu, scratch=norm._scratch(e.cout, dev).data_ptr())
    if total_rows is None:
        return [BN_BWD(dx=w.dconv, dgamma=w.dgamma, dbeta=w.dbeta, n_partials=n_partials, **common)]
    local, gathered, group = norm.sync_buffers(e.bn, e.cout, dev, backward=True)
    return [BN_BWD_SUMS_LOCAL(dgamma=w.dgamma, dbeta=w.dbeta, sums=local.data_ptr(), n_partials=n_partials, **common), Cut(local, gathered, group),
            BN_BWD_APPLY_GLOBAL(gathered=gathered.data_ptr(), world=gathered.shape[0], total_rows=total_rows, dx=w.dconv, **common)]


class SparseChainFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, blocks, rulebooks, *params):
        lib = _lib.load()
        dev = features.device
        ctx.set_materialize_grads(False)                                              # a tap nobody differentiates arrives as None, not as zeros
        features = features.contiguous().float()
        fold_in, materialize = fold_plan(blocks, rulebooks)
        offs, total = [], 0                                                           # one allocation for every activation
        for k, (b, rb) in enumerate(zip(blocks, rulebooks)):
            n = rb.n_out * b.cout
            ny = n if materialize[k] else 0
            offs.append(_Forward(total, total + n, total + n + ny, total + n + ny + b.cout, total + n + ny + 2 * b.cout))
            total += n + ny + 4 * b.cout
        arena = torch.empty((total,), dtype=torch.float32, device=dev)
        base = arena.data_ptr()
        n_part = lib.sv_conv_planned_partials()
        rows, x_ptr, n_src, keep = [], features.data_ptr(), features.shape[0], []
        frags = []
        # every rank keeps the total row count of each synced block (norm.route) on the device for the backward
        synced = [norm.route(b.bn) == norm.SYNCED for b in blocks]
        totals = torch.empty((len(blocks),), dtype=torch.float64, device=dev) if any(synced) else None
        in_coef, in_relu = None, 0                                                    # the transform this block's conv applies on load
        for k, (b, rb) in enumerate(zip(blocks, rulebooks)):
            w, gamma, beta = params[3 * k:3 * k + 3]
            a = _addresses(base, offs[k])
            row, frag_bwd, planned = _conv_row(b, rb, keep, x_ptr, n_src, a.conv, bn_partial=norm.partial_address(b.cout, dev) if norm.STATS_IN_CONV else None,
                                               in_coef=in_coef, in_relu=in_relu)
            rows.append(row)
            frags.append(frag_bwd)
            n_partials = n_part if norm.STATS_IN_CONV and planned else 0              # only the planned kernel's epilogue makes the sums
            rows += _bn_forward_rows(b, a, rb.n_out, gamma, beta, n_partials, materialize[k], totals.data_ptr() + 8 * k if synced[k] else None)
            if k + 1 < len(blocks) and fold_in[k + 1]:
                x_ptr, in_coef, in_relu = a.conv, a.coef, int(b.relu)
            else:
                x_ptr, in_coef, in_relu = a.y, None, 0
            n_src = rb.n_out
        _run_cut(rows, lambda seg: _run(seg, "sv_run_ops (chain forward)"))
        ctx.blocks, ctx.rulebooks, ctx.offs, ctx.frags, ctx.fold_in, ctx.synced = blocks, rulebooks, offs, frags, fold_in, synced
        ctx.save_for_backward(features, arena, totals, *params)
        # a tap whose normalised output is written in the list is that tensor; the others hand out [raw conv output, coefficients] (see run_chain)
        outs, coefs = [], []
        for k, b in enumerate(blocks):
            if b.tap:
                o = offs[k]
                outs.append((arena[o.y:o.mean] if materialize[k] else arena[o.conv:o.y]).view(rulebooks[k].n_out, b.cout))
                if not materialize[k]:
                    coefs.append(arena[o.coef:o.coef + 2 * b.cout])
        ctx.mark_non_differentiable(*coefs)
        return tuple(outs) + tuple(coefs)

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.load()
        features, arena, totals, *params = ctx.saved_tensors
        blocks, rulebooks, offs, frags, fold_in, synced = ctx.blocks, ctx.rulebooks, ctx.offs, ctx.frags, ctx.fold_in, ctx.synced
        dev = arena.device
        L = len(blocks)
        ext, gi = [None] * L, 0                                                       # gradient that reaches a block's output from outside the chain
        for k, b in enumerate(blocks):                                                # (behind the taps' gradients come the Nones of the coefficient outputs)
            if b.tap:
                ext[k] = None if grads[gi] is None else grads[gi].contiguous().float()
                gi += 1
        if ext[L - 1] is None:
            ext[L - 1] = torch.zeros((rulebooks[-1].n_out, blocks[-1].cout), dtype=torch.float32, device=dev)
        # one allocation for the work buffers, one for the weight gradients (in the parameters' own layout)
        boffs, total, woffs, wtotal, wbytes, poffs, wplans = [], 0, [], 0, 0, [], []
        for k, (b, rb) in enumerate(zip(blocks, rulebooks)):
            n, nin = rb.n_out * b.cout, (rb.n_in * b.cin if k > 0 else 0)
            boffs.append(_Backward(total, total + n, total + n + nin, total + n + nin + b.cout))
            total += n + nin + 2 * b.cout
            woffs.append(wtotal)
            wtotal += b.K * b.cin * b.cout
            wp = rb.wgrad_plan(b.cin, b.cout)                        # equal-pieces plan of the table (built with the index; here only if it was not)
            wplans.append(None if wp is None else wp.data_ptr())
            if DEFER_WGRAD_REDUCE:                                   # every layer keeps its own partial slabs until the one reduction at the end of the list
                poffs.append(wbytes)
                wbytes += lib.sv_sparse_conv_wgrad_partial_bytes(rb.n_out, b.K, b.cin, b.cout) if wp is None else lib.sv_sparse_conv_wgrad_planned_bytes(b.K, b.cin, b.cout)
            else:
                poffs.append(0)
                wbytes = max(wbytes, lib.sv_sparse_conv_wgrad_scratch_bytes(rb.n_out, b.K, b.cin, b.cout) if wp is None
                             else lib.sv_sparse_conv_wgrad_planned_bytes(b.K, b.cin, b.cout))
        work = torch.empty((total,), dtype=torch.float32, device=dev)
        wgrads = torch.empty((wtotal,), dtype=torch.float32, device=dev)
        wscratch = _lib.workspace.scratch("wgrad_layers" if DEFER_WGRAD_REDUCE else "wgrad", wbytes, dev)
        base, abase, wbase = work.data_ptr(), arena.data_ptr(), wgrads.data_ptr()       # abase: of the SAVED arena (autograd may hand back another tensor)
        rows = []
        n_part, n_part_bwd = lib.sv_conv_planned_partials(), 0          # n_part_bwd: partials the data-gradient launch above left for this BatchNorm
        wgrad_row = WGRAD_DEFERRED if DEFER_WGRAD_REDUCE else WGRAD
        dy_ptr = ext[L - 1].data_ptr()
        for k in range(L - 1, -1, -1):
            b, rb = blocks[k], rulebooks[k]
            w, gamma, beta = params[3 * k:3 * k + 3]
            a, o = _addresses(abase, offs[k]), _addresses(base, boffs[k])
            lo = _addresses(abase, offs[k - 1]) if k > 0 else None                    # the block below, whose output is this layer's input
            rows += _bn_backward_rows(b, a, o, rb.n_out, dy_ptr, gamma, beta, n_part_bwd, totals.data_ptr() + 8 * k if synced[k] else None)
            n_part_bwd = 0
            # the layer's input: the features, the block below's normalised output, or (folded) its raw conv output + the coefficients of its BatchNorm
            x_in = features.data_ptr() if k == 0 else lo.conv if fold_in[k] else lo.y
            rows.append(wgrad_row(X=x_in, n_src=rb.n_in, nbr=rb.addr("nbr_out"), dY=o.dconv, n_rows=rb.n_out, dW=wbase + 4 * woffs[k],
                                  scratch=wscratch.data_ptr() + poffs[k], K=b.K, Cin=b.cin, Cout=b.cout, stride_k=b.cin, stride_cin=1, stride_cout=b.K * b.cin,
                                  plan=wplans[k], in_coef=lo.coef if fold_in[k] else None, in_relu=int(blocks[k - 1].relu) if fold_in[k] else 0))
            if k > 0:
                dgrad = dict(n_src=rb.n_out, wfrag=frags[k].data_ptr(), n_rows=rb.n_in, K=b.K, Kd=b.cout, Nc=b.cin)
                plan = rb.plan_addrs("bwd", b.cout, b.cin)
                res = ext[k - 1]
                if res is None and norm.STATS_IN_CONV and BWD_SUMS_IN_CONV:
                    # the gradient this launch writes is the whole gradient of block k-1's output: its epilogue also makes the two sums of that
                    # block's BatchNorm backward (the rows' x comes from the arena), and the BatchNorm op below starts at the combine
                    below = blocks[k - 1]
                    rows.append(DGRAD_PLANNED_BN(plan, dZ=o.dconv, dY=o.dx, bn_x=lo.conv, bn_mean=lo.mean, bn_invstd=lo.istd,
                                                 bn_gamma=params[3 * (k - 1) + 1].data_ptr(), bn_beta=params[3 * (k - 1) + 2].data_ptr(),
                                                 bn_partial=norm.partial_address(below.cout, dev), bn_relu=int(below.relu), **dgrad))
                    n_part_bwd = n_part
                else:
                    rows.append(CONV_PLANNED(plan, X=o.dconv, Y=o.dx, residual=None if res is None else res.data_ptr(), **dgrad))
                dy_ptr = o.dx
        # cut lists (synced norms): every segment is a call of its own, so a weight gradient joins -- and a deferred reduction runs -- at the end of its segment
        _run_cut(rows, (lambda seg: _run_two_streams(seg, dev)) if WGRAD_STREAM else (lambda seg: _run(seg, "sv_run_ops (chain backward)")))
        out = [None, None, None]
        for k, b in enumerate(blocks):
            o = boffs[k]
            out += [wgrads[woffs[k]:woffs[k] + b.K * b.cin * b.cout].view(params[3 * k].shape), work[o.dgamma:o.dbeta], work[o.dbeta:o.dbeta + b.cout]]
        return tuple(out)


class LazyTap(SparseConvTensor):
    """A tap whose normalised features are made when somebody reads them (BN_FOLD): PV-RCNN's set abstraction reads multi_scale_3d_features, SECOND /
    the benchmarked step read none of x_conv1..4 -- their elementwise passes never run.  (One class for all taps: a class made per call is a
    reference cycle that only the cyclic collector frees, and it kept the tap's tensors alive with it -- sporadic allocator growth in the step.)"""

    def __init__(self, raw, coef, relu, indices, spatial_shape, batch_size, grid=None, indice_dict=None):
        super().__init__(None, indices, spatial_shape, batch_size, grid, indice_dict)
        self._raw, self._coef, self._relu = raw, coef, relu

    @property
    def features(self):
        if self._features is None:
            self._features = _TapApply.apply(self._raw, self._coef, self._relu)
            self._raw = self._coef = None
        return self._features

    @features.setter
    def features(self, value):
        self._features = value


def run_chain(blocks, x):
    """x: SparseConvTensor at the chain's input with every rulebook prebuilt.  -> list of SparseConvTensor, one per tap, in order."""
    rulebooks = [x.indice_dict[b.conv.indice_key] for b in blocks]
    params = []
    for b in blocks:
        params += [b.conv.weight, b.bn.weight, b.bn.bias]
    outs = SparseChainFunction.apply(x.features, blocks, rulebooks, *params)
    taps = [(b, rb) for b, rb in zip(blocks, rulebooks) if b.tap]
    _, materialize = fold_plan(blocks, rulebooks)
    tap_mat = [materialize[k] for k, b in enumerate(blocks) if b.tap]
    coefs = list(outs[len(taps):])
    res = []
    for f, (b, rb), mat in zip(outs[:len(taps)], taps, tap_mat):
        if mat:
            res.append(SparseConvTensor(f, rb.out_indices, rb.out_shape, x.batch_size, x.grid, x.indice_dict))
        else:
            res.append(LazyTap(f, coefs.pop(0), b.relu, rb.out_indices, rb.out_shape, x.batch_size, x.grid, x.indice_dict))
    return res


# ---------------------------------------------------------------------------------------------------------------- eval mode
def eval_applicable(entries, x):
    """The eval list takes these entries on x now: SEEVCN_CHAIN and SEEVCN_EVAL_CHAIN not 0, gradients disabled, fp32 CUDA features with at least one row,
    no hooks on anything walked, every norm in eval mode with running statistics on a channel count the fused BatchNorm kernels take (what the module
    path would run, so both give the same bits), every rulebook in x's indice_dict with the conv's kernel size and the row counts of a chain."""
    if CHAIN_OFF or EVAL_CHAIN_OFF or entries is None or torch.is_grad_enabled():
        return False
    f = x.features
    if not (f.is_cuda and f.dtype == torch.float32 and f.dim() == 2 and f.shape[0] >= 1 and f.shape[1] == entries[0].cin):
        return False
    if any(_has_hooks(m) for m in getattr(entries, 'walked', ())):
        return False
    rows = [f.shape[0]]                                                              # rows[k + 1]: rows of entry k's output; rows[0]: of the input
    for e in entries:
        bn, w = e.bn, e.conv.weight
        if (norm.route(bn) is None or bn.training or not bn.track_running_stats or bn.running_mean is None or bn.running_var is None
                or bn.num_features != e.cout or not norm.channels_fusable(e.cout) or bn.momentum is None or not bn.running_mean.is_cuda):
            return False
        if not (w.is_cuda and w.dtype == torch.float32) or e.conv.indice_key is None:
            return False
        rb = x.indice_dict.get(e.conv.indice_key)
        if rb is None or rb.ksize != e.conv.kernel_size or rb.n_in != rows[-1] or rb.n_out < 1:
            return False
        if e.residual_from is not None and rows[e.residual_from + 1] != rb.n_out:
            return False
        rows.append(rb.n_out)
    return True


def eval_half_applicable(entries, x):
    """The half-precision form of the eval list takes these entries on x now: everything eval_applicable asks, at least two entries, and behind the
    first one (the fp32 input layer) every convolution on a planned table with a shape the fp16 kernel is built for (sv_conv_h16_applies), no identity
    read from the chain's fp32 input."""
    if not eval_applicable(entries, x) or len(entries) < 2:
        return False
    lib = _lib.load()
    for k, e in enumerate(entries):
        if e.residual_from is not None and e.residual_from < 0:
            return False
        if k == 0:
            continue
        rb = x.indice_dict[e.conv.indice_key]
        if not lib.sv_conv_h16_applies(int(e.K), int(e.cin), int(e.cout), int(rb.n_in)) or rb.plan_addrs("fwd", e.cin, e.cout) is None:
            return False
    return True


class HalfTap(SparseConvTensor):
    """A tap of the half-precision eval list: the rows stay fp16 until somebody reads `.features`, which widens them to fp32 once (exact) and keeps the
    result -- SECOND and CenterPoint read none of x_conv1..4, PV-RCNN pays one elementwise pass per scale it reads.  `features_half` is the stored tensor."""

    def __init__(self, half, indices, spatial_shape, batch_size, grid=None, indice_dict=None):
        super().__init__(None, indices, spatial_shape, batch_size, grid, indice_dict)
        self.features_half = half

    @property
    def features(self):
        if self._features is None:
            self._features = self.features_half.float()
        return self._features

    @features.setter
    def features(self, value):
        self._features = value


def _align16(nbytes):
    return (int(nbytes) + 15) & ~15


def _run_eval_chain_half(entries, x, keep_all=False):
    """run_eval_chain's half-precision form.  The list: [all BatchNorm coefficients, fp32] + [entry 0 on the fp32 conv row: raw point features (coordinates
    of up to 70 m) are never rounded to fp16] + [SV_OP_NARROW_H16: its fp16 copy] + one SV_OP_CONV_PLANNED_H16 per further entry, each reading and
    writing fp16 rows, the last one storing fp32.  Offsets are BYTES, every piece 16-byte aligned.  keep_all: every entry's output leaves with the result
    (-> list of (n_out, cout) tensors, one per entry: tests hold each layer to its own bound)."""
    dev = x.features.device
    features = x.features.contiguous()
    rulebooks = [x.indice_dict[e.conv.indice_key] for e in entries]
    L = len(entries)
    leaves = [keep_all or e.tap for e in entries]
    size = [rb.n_out * e.cout * (4 if k == L - 1 else 2) for k, (e, rb) in enumerate(zip(entries, rulebooks))]
    t_total, w_total, c_offs, y_offs = 0, 0, [], []
    for e in entries:
        c_offs.append(w_total)
        w_total += _align16(8 * e.cout)
    y0_f32 = w_total                                                                 # entry 0's fp32 output: dies with the call
    w_total += _align16(4 * rulebooks[0].n_out * entries[0].cout)
    for k in range(L):
        if leaves[k]:
            y_offs.append(t_total)
            t_total += _align16(size[k])
        else:
            y_offs.append(w_total)
            w_total += _align16(size[k])
    arena = torch.empty((t_total,), dtype=torch.uint8, device=dev)
    work = torch.empty((w_total,), dtype=torch.uint8, device=dev)
    assert arena.data_ptr() % 16 == 0 and work.data_ptr() % 16 == 0
    base = work.data_ptr()
    y_addr = [(arena.data_ptr() if leaves[k] else base) + y_offs[k] for k in range(L)]
    jobs = np.zeros((L, 8), dtype=np.int64)
    rows = [BN_EVAL_COEF_BATCH(jobs_host=jobs.ctypes.data, n_jobs=L)]
    keep = []
    x_ptr, n_src = features.data_ptr(), features.shape[0]
    for k, (e, rb) in enumerate(zip(entries, rulebooks)):
        bn, conv = e.bn, e.conv
        o_coef = base + c_offs[k]
        jobs[k, :7] = (0 if bn.weight is None else bn.weight.data_ptr(), 0 if bn.bias is None else bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                       bn.running_var.data_ptr(), o_coef, e.cout, _bits(bn.eps))
        bias = None if conv.bias is None else conv.bias.data_ptr()
        epilogue = dict(relu=int(e.relu), bias=bias, scale=o_coef, shift=o_coef + 4 * e.cout)
        if k == 0:
            assert e.residual_from is None
            rows.append(_conv_row(e, rb, keep, x_ptr, n_src, base + y0_f32, residual=None, **epilogue)[0])
            rows.append(NARROW_H16(x_f32=base + y0_f32, n_elems=rb.n_out * e.cout, y_f16=y_addr[0]))
        else:
            res = None if e.residual_from is None else y_addr[e.residual_from]
            rows.append(CONV_PLANNED_H16(rb.plan_addrs("fwd", e.cin, e.cout), X16=x_ptr, n_src=n_src, wfrag16=Fsp.fragment_cache.get_half(conv.weight_kio_nograd()).data_ptr(),
                                         Y=y_addr[k], y_is_f32=k == L - 1, n_rows=rb.n_out, K=e.K, Kd=e.cin, Nc=e.cout, residual16=res, **epilogue))
        x_ptr, n_src = y_addr[k], rb.n_out
    _run(rows, "sv_run_ops (eval chain, fp16)")

    def view(k):
        e, rb = entries[k], rulebooks[k]
        return arena[y_offs[k]:y_offs[k] + size[k]].view(torch.float32 if k == L - 1 else torch.float16).view(rb.n_out, e.cout)

    if keep_all:
        return [view(k) for k in range(L)]
    out = []
    for k, (e, rb) in enumerate(zip(entries, rulebooks)):
        if e.tap:
            meta = (rb.out_indices, rb.out_shape, x.batch_size, x.grid, x.indice_dict)
            out.append(SparseConvTensor(view(k), *meta) if k == L - 1 else HalfTap(view(k), *meta))
    return out


def run_eval_chain(entries, x, dtype=torch.float32):
    """dtype torch.float16: the half-precision form (_run_eval_chain_half; ask eval_half_applicable first) -- fp16 activations and weight fragments, fp32
    arithmetic, the last entry's output and every tap's `.features` fp32.  Default: the fp32 list, unchanged.
    x: SparseConvTensor at the chain's input with every rulebook prebuilt (and the weight fragments refreshed).  -> list of SparseConvTensor, one per
    tap, in order.  ONE sv_run_ops call: [all BatchNorm coefficients] + one convolution per entry; nothing is saved, parameters and buffers are only read.
    Only the taps' features outlive the call."""
    if dtype == torch.float16:
        return _run_eval_chain_half(entries, x)
    assert dtype == torch.float32, dtype
    dev = x.features.device
    features = x.features.contiguous()
    rulebooks = [x.indice_dict[e.conv.indice_key] for e in entries]
    L = len(entries)
    # two allocations (all offsets multiples of 4 floats: 16-byte aligned pieces): the taps' outputs, which leave with the result, and everything that dies
    # with this call -- every entry's (scale | shift) and the outputs nobody outside reads (freed to torch's allocator on the stream the list runs on)
    t_total, w_total, c_offs, y_offs = 0, 0, [], []
    for e in entries:
        c_offs.append(w_total)
        w_total += 2 * e.cout
    for e, rb in zip(entries, rulebooks):
        if e.tap:
            y_offs.append(t_total)
            t_total += rb.n_out * e.cout
        else:
            y_offs.append(w_total)
            w_total += rb.n_out * e.cout
    arena = torch.empty((t_total,), dtype=torch.float32, device=dev)
    work = torch.empty((w_total,), dtype=torch.float32, device=dev)
    y_addr = [(arena if e.tap else work).data_ptr() + 4 * y_offs[k] for k, e in enumerate(entries)]
    base = work.data_ptr()
    jobs = np.zeros((L, 8), dtype=np.int64)
    rows = [BN_EVAL_COEF_BATCH(jobs_host=jobs.ctypes.data, n_jobs=L)]
    keep = []
    x_ptr, n_src = features.data_ptr(), features.shape[0]
    for k, (e, rb) in enumerate(zip(entries, rulebooks)):
        bn, conv = e.bn, e.conv
        o_coef, o_y = base + 4 * c_offs[k], y_addr[k]
        jobs[k, :7] = (0 if bn.weight is None else bn.weight.data_ptr(), 0 if bn.bias is None else bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                       bn.running_var.data_ptr(), o_coef, e.cout, _bits(bn.eps))
        bias = None if conv.bias is None else conv.bias.data_ptr()
        res = None if e.residual_from is None else (features.data_ptr() if e.residual_from < 0 else y_addr[e.residual_from])
        rows.append(_conv_row(e, rb, keep, x_ptr, n_src, o_y, relu=int(e.relu), bias=bias, scale=o_coef, shift=o_coef + 4 * e.cout, residual=res)[0])
        x_ptr, n_src = o_y, rb.n_out
    _run(rows, "sv_run_ops (eval chain)")
    return [SparseConvTensor(arena[y_offs[k]:y_offs[k] + rb.n_out * e.cout].view(rb.n_out, e.cout), rb.out_indices, rb.out_shape, x.batch_size, x.grid,
                             x.indice_dict)
            for k, (e, rb) in enumerate(zip(entries, rulebooks)) if e.tap]
