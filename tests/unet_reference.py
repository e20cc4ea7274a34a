"""TEST INFRASTRUCTURE: float64 torch restatements on the CPU, over the oracle's rulebooks (oracle/spconv.py), of the inverse sparse convolution
and of UNetV2's forward (detector3d/pcdet/models/backbones_3d/spconv_unet.py).  Everything is differentiable, so autograd gives the gradients.

  sparse / submanifold conv   y[j] = sum_k x[nbr_out[k][j]] W[k]
  inverse conv                z[i] = sum_k sum_{j: nbr_out[k][j] = i} u[j] W[k]      over the PAIRED strided layer's nbr_out
  weights                     (C_out, kz, ky, kx, C_in) -> W[k] (C_in, C_out), k = (kz * ky_size + ky) * kx_size + kx
"""
import numpy as np
import torch

from oracle import spconv as osp

D = torch.float64


def w_kio(weight):
    w = weight.to(D)
    co, ci = w.shape[0], w.shape[-1]
    return w.reshape(co, -1, ci).permute(1, 2, 0)


def conv(x, nbr_out, weight, bias=None):
    """x (N_in, C_in) -> (N_out, C_out) over an output-major table nbr_out (K, N_out) (numpy int32, -1 = no pair)."""
    w = w_kio(weight)
    out = torch.zeros((nbr_out.shape[1], w.shape[2]), dtype=D)
    for k in range(nbr_out.shape[0]):
        j = np.flatnonzero(nbr_out[k] >= 0)
        if len(j):
            out = out.index_add(0, torch.from_numpy(j), x[torch.from_numpy(nbr_out[k, j].astype(np.int64))] @ w[k])
    return out if bias is None else out + bias.to(D)


def inverse_conv(u, nbr_out, n_in, weight, bias=None):
    """u (N_out, C_in) on the paired strided layer's OUTPUT sites -> z (n_in, C_out) on its input sites."""
    w = w_kio(weight)
    out = torch.zeros((n_in, w.shape[2]), dtype=D)
    for k in range(nbr_out.shape[0]):
        j = np.flatnonzero(nbr_out[k] >= 0)
        if len(j):
            out = out.index_add(0, torch.from_numpy(nbr_out[k, j].astype(np.int64)), u[torch.from_numpy(j)] @ w[k])
    return out if bias is None else out + bias.to(D)


def bn(x, sd, prefix, training, eps=1e-3):
    g, b = sd[prefix + ".weight"].to(D), sd[prefix + ".bias"].to(D)
    if training:
        m, v = x.mean(0), x.var(0, unbiased=False)
    else:
        m, v = sd[prefix + ".running_mean"].to(D), sd[prefix + ".running_var"].to(D)
    return (x - m) / torch.sqrt(v + eps) * g + b


class UNetV2Reference:
    """UNetV2.forward (spconv_unet.py:165-212) on the state_dict `sd` of the module (tensors that require grad stay in the graph)."""

    def __init__(self, sd, coords, sparse_shape, training):
        self.sd, self.training = sd, training
        c0 = np.asarray(coords, np.int32)
        self.coords = [c0]
        self.subm, self.down = {}, {}
        shape = tuple(sparse_shape)
        self.shapes = [shape]
        for lv, pad in ((2, 1), (3, 1), (4, (0, 1, 1))):
            oc, nbr_out, _, oshape = osp.rulebook_sparse(self.coords[-1], self.shapes[-1], 3, 2, pad)
            self.down[lv] = nbr_out
            self.coords.append(oc)
            self.shapes.append(tuple(oshape))
        for lv in range(4):
            self.subm[lv + 1] = osp.rulebook_subm(self.coords[lv], self.shapes[lv], 3)
        oc, nbr_out, _, oshape = osp.rulebook_sparse(self.coords[3], self.shapes[3], (3, 1, 1), (2, 1, 1), 0)
        self.out_coords, self.out_nbr, self.out_shape = oc, nbr_out, tuple(oshape)

    def _cbr(self, x, nbr, prefix, inverse_n=None):
        """SparseSequential(conv, BatchNorm1d, ReLU) named prefix.0 / prefix.1"""
        w = self.sd[prefix + ".0.weight"]
        y = conv(x, nbr, w) if inverse_n is None else inverse_conv(x, nbr, inverse_n, w)
        return torch.relu(bn(y, self.sd, prefix + ".1", self.training))

    def _basic_block(self, x, nbr, prefix):
        sd = self.sd
        y = conv(x, nbr, sd[prefix + ".conv1.weight"], sd.get(prefix + ".conv1.bias"))
        y = torch.relu(bn(y, sd, prefix + ".bn1", self.training))
        y = conv(y, nbr, sd[prefix + ".conv2.weight"], sd.get(prefix + ".conv2.bias"))
        y = bn(y, sd, prefix + ".bn2", self.training)
        return torch.relu(y + x)

    @staticmethod
    def _channel_reduction(x, out_channels):
        n, c = x.shape
        assert c % out_channels == 0
        return x.view(n, out_channels, -1).sum(2)

    def _ur_block(self, x_lateral, x_bottom, lv, inverse_nbr, inverse_n):
        x_trans = self._basic_block(x_lateral, self.subm[lv], f"conv_up_t{lv}")
        x = torch.cat([x_bottom, x_trans], 1)
        x_m = self._cbr(x, self.subm[lv], f"conv_up_m{lv}")
        x = x_m + self._channel_reduction(x, x_m.shape[1])
        if inverse_nbr is None:
            return self._cbr(x, self.subm[lv], "conv5.0")
        return self._cbr(x, inverse_nbr, f"inv_conv{lv}", inverse_n=inverse_n)

    def forward(self, features):
        x = self._cbr(features.to(D), self.subm[1], "conv_input")
        x1 = self._cbr(x, self.subm[1], "conv1.0")
        x2 = self._cbr(x1, self.down[2], "conv2.0")
        x2 = self._cbr(self._cbr(x2, self.subm[2], "conv2.1"), self.subm[2], "conv2.2")
        x3 = self._cbr(x2, self.down[3], "conv3.0")
        x3 = self._cbr(self._cbr(x3, self.subm[3], "conv3.1"), self.subm[3], "conv3.2")
        x4 = self._cbr(x3, self.down[4], "conv4.0")
        x4 = self._cbr(self._cbr(x4, self.subm[4], "conv4.1"), self.subm[4], "conv4.2")
        out = None
        if "conv_out.0.weight" in self.sd:
            out = torch.relu(bn(conv(x4, self.out_nbr, self.sd["conv_out.0.weight"]), self.sd, "conv_out.1", self.training))
        up4 = self._ur_block(x4, x4, 4, self.down[4], len(self.coords[2]))
        up3 = self._ur_block(x3, up4, 3, self.down[3], len(self.coords[1]))
        up2 = self._ur_block(x2, up3, 2, self.down[2], len(self.coords[0]))
        up1 = self._ur_block(x1, up2, 1, None, None)
        return {"point_features": up1, "encoded": out, "encoded_coords": self.out_coords, "encoded_shape": self.out_shape,
                "voxel_coords": self.coords[0]}
