"""Oracle: the TRAINING step of VoxelBackBone8x / VoxelResBackBone8x + HeightCompression as one differentiable chain on the CPU.  Test infrastructure only.

The sparse convolutions are oracle/spconv.py's numpy restatement (spconv itself is un-vendored: PARITY UNPINNED, see that header) wrapped in a
torch.autograd.Function; BatchNorm1d(eps 1e-3, momentum 0.01, batch statistics) and ReLU are torch's own CPU ops in the chosen dtype -- the
reference's layer composition, detector3d/pcdet/models/backbones_3d/spconv_backbone.py:8-27,77-117,128-180; the dense scatter follows
backbones_2d/map_to_bev/height_compression.py:21-26.  float64 gives the tight reference for the gradient-parity test
(tests/test_spconv.py), float32 is what bench.py's cpu_baseline times."""
import numpy as np
import torch

from . import spconv as osp


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, nbr):
        ctx.nbr = nbr
        ctx.save_for_backward(x, w)
        return torch.from_numpy(osp.conv_forward(x.numpy(), nbr, w.numpy())).to(x.dtype)

    @staticmethod
    def backward(ctx, go):
        x, w = ctx.saved_tensors
        gf, gw = osp.conv_backward(x.numpy(), ctx.nbr, w.numpy(), go.numpy())
        return torch.from_numpy(gf).to(x.dtype), torch.from_numpy(gw).to(w.dtype), None


def backbone8x_train_chain(sd, features, coords, batch_size, sparse_shape, dtype=torch.float64):
    """sd: VoxelBackBone8x state_dict (numpy, 2.x weight layout, the reference's key names).  Returns (dense (B, C*D, H, W) tensor with grad_fn,
    leaves): leaves = {'input': features leaf, '<conv key>': (K, C_in, C_out) weight leaf, '<bn key>.weight' / '.bias': leaves}."""
    leaves = {}

    def W(key):
        t = torch.from_numpy(osp.weight_to_kio(np.asarray(sd[key]))).to(dtype).requires_grad_(True)
        leaves[key] = t
        return t

    def bn_relu(x, prefix):
        g = torch.from_numpy(np.asarray(sd[prefix + ".weight"])).to(dtype).requires_grad_(True)
        b = torch.from_numpy(np.asarray(sd[prefix + ".bias"])).to(dtype).requires_grad_(True)
        leaves[prefix + ".weight"], leaves[prefix + ".bias"] = g, b
        return torch.relu(torch.nn.functional.batch_norm(x, None, None, g, b, True, 0.01, 1e-3))

    shape = tuple(int(s) for s in sparse_shape)
    x = torch.from_numpy(np.asarray(features)).to(dtype).requires_grad_(True)
    leaves["input"] = x
    nb = osp.rulebook_subm(coords, shape, 3)
    x = bn_relu(_Conv.apply(x, W("conv_input.0.weight"), nb), "conv_input.1")
    x = bn_relu(_Conv.apply(x, W("conv1.0.0.weight"), nb), "conv1.0.1")
    c = coords
    for name, pad in (("conv2", 1), ("conv3", 1), ("conv4", (0, 1, 1))):
        oc, nbo, _, oshape = osp.rulebook_sparse(c, shape, 3, 2, pad)
        x = bn_relu(_Conv.apply(x, W(f"{name}.0.0.weight"), nbo), f"{name}.0.1")
        c, shape = oc, oshape
        nb = osp.rulebook_subm(c, shape, 3)
        for i in (1, 2):
            x = bn_relu(_Conv.apply(x, W(f"{name}.{i}.0.weight"), nb), f"{name}.{i}.1")
    oc, nbo, _, oshape = osp.rulebook_sparse(c, shape, (3, 1, 1), (2, 1, 1), 0)
    x = bn_relu(_Conv.apply(x, W("conv_out.0.weight"), nbo), "conv_out.1")
    dense = torch.zeros(batch_size, *oshape, x.shape[1], dtype=dtype)
    idx = [torch.from_numpy(oc[:, i].astype(np.int64)) for i in range(4)]
    dense = dense.index_put((idx[0], idx[1], idx[2], idx[3]), x)                       # (B, D, H, W, C)
    dense = dense.permute(0, 4, 1, 2, 3).reshape(batch_size, x.shape[1] * oshape[0], oshape[1], oshape[2])
    return dense, leaves, (x, oc, oshape)


def sparse_conv(x, w, nbr):
    """The sparse convolution as a differentiable torch function: x (N_in, C_in), w (K, C_in, C_out), nbr (K, N_out) as in oracle/spconv.py."""
    return _Conv.apply(x, w, nbr)


class _Layers:
    """The layer kinds of both backbones as differentiable CPU steps that record what the tests need: parameter leaves, the batch statistics of
    every BatchNorm, the tensors on both sides of every BatchNorm (gradients retained) and the ReLU branches taken from hints.

    The ReLU's derivative jumps at zero: for a pre-activation within rounding distance of zero a float32 and a float64 evaluation may take
    different branches, both valid, and the gradients of everything it feeds then differ by O(1).  branch_hints {key: bool (rows, C)} are
    the branches the evaluation under test took (its ReLU output > 0); they are followed ONLY where |pre-activation| < hint_band, everywhere
    else the oracle's own sign decides.  `overridden` counts the positions where the hint changed the oracle's branch, `hinted` all positions
    of the hinted activations."""

    def __init__(self, sd, dtype, branch_hints=None, hint_band=0.0):
        self.sd, self.dtype, self.hints, self.band = sd, dtype, branch_hints, hint_band
        self.leaves, self.bn_stats, self.bn_in, self.bn_out, self.pre_act = {}, {}, {}, {}, {}
        self.overridden = self.hinted = 0

    def leaf(self, key, t):
        t = t.to(self.dtype).requires_grad_(True)
        self.leaves[key] = t
        return t

    def conv(self, x, key, nbr, bias_key=None):
        """_Conv with the (K, C_in, C_out) view of sd[key] as a leaf; + sd[bias_key] (a leaf too) when given."""
        y = _Conv.apply(x, self.leaf(key, torch.from_numpy(osp.weight_to_kio(np.asarray(self.sd[key])))), nbr)
        if bias_key is not None:
            y = y + self.leaf(bias_key, torch.from_numpy(np.asarray(self.sd[bias_key])))
        return y

    def bn(self, x, prefix):
        """BatchNorm1d in training mode (batch statistics, eps 1e-3, momentum 0.01: spconv_backbone.py:73, :187).  bn_stats[prefix] = (mean, biased
        variance, rows) of the batch; bn_in / bn_out[prefix] keep x and the result with their gradients retained."""
        g = self.leaf(prefix + ".weight", torch.from_numpy(np.asarray(self.sd[prefix + ".weight"])))
        b = self.leaf(prefix + ".bias", torch.from_numpy(np.asarray(self.sd[prefix + ".bias"])))
        if x.requires_grad:
            x.retain_grad()
        z = torch.nn.functional.batch_norm(x, None, None, g, b, True, 0.01, 1e-3)
        z.retain_grad()
        xd = x.detach()
        self.bn_stats[prefix] = (xd.mean(0).numpy(), xd.var(0, unbiased=False).numpy(), int(xd.shape[0]))
        self.bn_in[prefix], self.bn_out[prefix] = x, z
        return z

    def relu(self, z, key):
        self.pre_act[key] = z.detach()
        on = z.detach() > 0
        if self.hints is not None and key in self.hints:
            hint = torch.from_numpy(np.asarray(self.hints[key], bool))
            use = (z.detach().abs() < self.band) & (hint != on)
            self.overridden += int(use.sum())
            self.hinted += hint.numel()
            on = torch.where(use, hint, on)
        return torch.where(on, z, torch.zeros_like(z))

    def post_act(self, x, key, bn, nbr):
        """conv -> BatchNorm -> ReLU (post_act_block, spconv_backbone.py:8-27); the ReLU's hint key is the conv key."""
        return self.relu(self.bn(self.conv(x, key, nbr), bn), key)

    def basic(self, x, prefix, nbr):
        """SparseBasicBlock (spconv_backbone.py:30-66): conv1(+bias) -> bn1 -> ReLU -> conv2(+bias) -> bn2 -> (+identity) -> ReLU on ONE submanifold
        rulebook.  Hint keys: '<prefix>.bn1' for the ReLU behind bn1, '<prefix>' for the one behind the add."""
        y = self.conv(x, prefix + ".conv1.weight", nbr, prefix + ".conv1.bias")
        y = self.relu(self.bn(y, prefix + ".bn1"), prefix + ".bn1")
        y = self.conv(y, prefix + ".conv2.weight", nbr, prefix + ".conv2.bias")
        return self.relu(self.bn(y, prefix + ".bn2") + x, prefix)


def _dense_bev(x, oc, oshape, batch_size):
    """HeightCompression of a sparse tensor (height_compression.py:21-26): (B, C*D, H, W)."""
    dense = torch.zeros(batch_size, *oshape, x.shape[1], dtype=x.dtype)
    idx = [torch.from_numpy(oc[:, i].astype(np.int64)) for i in range(4)]
    dense = dense.index_put((idx[0], idx[1], idx[2], idx[3]), x)                       # (B, D, H, W, C)
    return dense.permute(0, 4, 1, 2, 3).reshape(batch_size, x.shape[1] * oshape[0], oshape[1], oshape[2])


def res_backbone8x_train_chain(sd, features, coords, batch_size, sparse_shape, dtype=torch.float64, branch_hints=None, hint_band=0.0):
    """The TRAINING step of VoxelResBackBone8x + HeightCompression (reference spconv_backbone.py:30-66, 183-293), composed as
    oracle/spconv.py voxel_res_backbone8x_forward composes the eval forward: conv_input; per level a strided conv-BN-ReLU (levels 2-4) and two
    basic blocks, both on the level's one submanifold rulebook; conv_out; dense scatter.  sd: state_dict (numpy, 2.x weight layout).
    Returns (dense (B, C*D, H, W) with grad_fn, leaves, info): leaves = {'input', every conv weight as (K, C_in, C_out), every conv bias, every
    BatchNorm weight / bias}; info = {'taps': {x_conv1..4, out: (features, coords, shape)}, 'bn_stats': {bn prefix: (mean, biased variance, rows)},
    'bn_in' / 'bn_out': {bn prefix: tensor, gradient retained}, 'pre_act': {hint key: pre-activation}, 'overridden', 'hinted'} (_Layers)."""
    L = _Layers(sd, dtype, branch_hints, hint_band)
    shape = tuple(int(s) for s in sparse_shape)
    c = np.asarray(coords)
    x = L.leaf("input", torch.from_numpy(np.asarray(features)))
    nb = osp.rulebook_subm(c, shape, 3)
    x = L.post_act(x, "conv_input.0.weight", "conv_input.1", nb)
    for i in (0, 1):
        x = L.basic(x, f"conv1.{i}", nb)
    taps = {"x_conv1": (x, c, shape)}
    for name, pad in (("conv2", 1), ("conv3", 1), ("conv4", (0, 1, 1))):
        c, nbo, _, shape = osp.rulebook_sparse(c, shape, 3, 2, pad)
        x = L.post_act(x, f"{name}.0.0.weight", f"{name}.0.1", nbo)
        nb = osp.rulebook_subm(c, shape, 3)
        for i in (1, 2):
            x = L.basic(x, f"{name}.{i}", nb)
        taps["x_" + name] = (x, c, shape)
    oc, nbo, _, oshape = osp.rulebook_sparse(c, shape, (3, 1, 1), (2, 1, 1), 0)
    x = L.post_act(x, "conv_out.0.weight", "conv_out.1", nbo)
    taps["out"] = (x, oc, oshape)
    info = {"taps": taps, "bn_stats": L.bn_stats, "bn_in": L.bn_in, "bn_out": L.bn_out, "pre_act": L.pre_act, "overridden": L.overridden, "hinted": L.hinted}
    return _dense_bev(x, oc, oshape, batch_size), L.leaves, info


def res_stage_train_chain(sd, layers, features, coords, shape, dtype=torch.float64, branch_hints=None, hint_band=0.0):
    """stage_train_chain for stages with residual blocks.  layers: stage_train_chain's 6-tuples, or ('basic', prefix) for a SparseBasicBlock on the
    submanifold rulebook of the current coordinates (consecutive blocks share it).  Returns (output with grad_fn, leaves incl. 'input', out_coords,
    out_shape, info) with info as in res_backbone8x_train_chain (without 'taps')."""
    L = _Layers(sd, dtype, branch_hints, hint_band)
    x = L.leaf("input", torch.from_numpy(np.asarray(features)))
    c, shape = np.asarray(coords), tuple(int(s) for s in shape)
    subm = None                                            # the 3x3x3 submanifold rulebook of the current coordinates
    for layer in layers:
        if layer[0] == "basic":
            if subm is None:
                subm = osp.rulebook_subm(c, shape, 3)
            x = L.basic(x, layer[1], subm)
            continue
        key, bn, kind, ksize, stride, pad = layer
        if kind == "subm":
            nbr = osp.rulebook_subm(c, shape, ksize)
        else:
            c, nbr, _, shape = osp.rulebook_sparse(c, shape, ksize, stride, pad)
            subm = None
        x = L.post_act(x, key, bn, nbr)
    info = {"bn_stats": L.bn_stats, "bn_in": L.bn_in, "bn_out": L.bn_out, "pre_act": L.pre_act, "overridden": L.overridden, "hinted": L.hinted}
    return x, L.leaves, c, shape, info


def stage_train_chain(sd, layers, features, coords, shape, dtype=torch.float64, branch_hints=None, hint_band=0.0):
    """One STAGE of the backbone (a run of conv -> BatchNorm(batch statistics) -> ReLU blocks, spconv_backbone.py:8-27) as a differentiable chain.
    layers: [(conv key, bn prefix, 'subm' | 'sparse', ksize, stride, padding)], sd as in backbone8x_train_chain.  Returns (output tensor with grad_fn,
    leaves incl. 'input', out_coords, out_shape, n_overridden) -- used by the 16-scene sampled-stage gradient test, where the inputs and the
    upstream gradient of the stage are the GPU step's own tensors.

    The ReLU's derivative jumps at zero: for a pre-activation within rounding distance of zero a float32 and a float64 evaluation may take
    different branches, both valid, and the gradients of everything it feeds then differ by O(1).  branch_hints {conv key: bool (rows, C)} are
    the branches the evaluation under test took (its ReLU output > 0); they are followed ONLY where |pre-activation| < hint_band, everywhere
    else the oracle's own sign decides.  n_overridden counts the positions where the hint changed the oracle's branch."""
    leaves = {}
    x = torch.from_numpy(np.asarray(features)).to(dtype).requires_grad_(True)
    leaves["input"] = x
    c, shape = np.asarray(coords), tuple(int(s) for s in shape)
    overridden = 0
    for key, bn, kind, ksize, stride, pad in layers:
        w = torch.from_numpy(osp.weight_to_kio(np.asarray(sd[key]))).to(dtype).requires_grad_(True)
        g = torch.from_numpy(np.asarray(sd[bn + ".weight"])).to(dtype).requires_grad_(True)
        b = torch.from_numpy(np.asarray(sd[bn + ".bias"])).to(dtype).requires_grad_(True)
        leaves[key], leaves[bn + ".weight"], leaves[bn + ".bias"] = w, g, b
        if kind == "subm":
            nbr = osp.rulebook_subm(c, shape, ksize)
        else:
            c, nbr, _, shape = osp.rulebook_sparse(c, shape, ksize, stride, pad)
        z = torch.nn.functional.batch_norm(_Conv.apply(x, w, nbr), None, None, g, b, True, 0.01, 1e-3)
        on = z.detach() > 0
        if branch_hints is not None and key in branch_hints:
            hint = torch.from_numpy(np.asarray(branch_hints[key], bool))
            use = (z.detach().abs() < hint_band) & (hint != on)
            overridden += int(use.sum())
            on = torch.where(use, hint, on)
        x = torch.where(on, z, torch.zeros_like(z))
    return x, leaves, c, shape, overridden
