"""FusedAdam: Adam / AdamW with gradient-norm clipping as at most three launches over a chunk table on the device (csrc/optim.hip).

One step of the reference (detector3d/tools/train_utils/train_utils.py:52-54 with the OptimWrapper of train_utils/optimization/fastai_optim.py) is
clip_grad_norm_, one p.data.mul_(1 - wd*lr) per parameter tensor and torch.optim.Adam's passes: hundreds of small launches behind host loops.
Here the norm is one launch with a fixed summation order (equal gradients give equal bits), the update is one launch, and nothing is read back.
The arithmetic order is stated in include/seevcn_hip.h and restated in tests/optim_reference.py.
"""
import ctypes

import numpy as np
import torch

from . import _lib

NO_DECAY, L2, DECOUPLED = 0, 1, 2

_CHUNK_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("tensor", "<i4"), ("group", "<i4"), ("pad", "<i4")])


def _round_up(n, k):
    return (n + k - 1) // k * k


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam's interface (param_groups with lr / betas / eps / weight_decay, Adam's state_dict layout) over the fused kernels.

    decoupled_weight_decay: False adds wd * p to the gradient (torch Adam), True multiplies p by 1 - lr * wd first (AdamW, fastai's true_wd).
    max_grad_norm: clip the global L2 norm of all gradients as torch.nn.utils.clip_grad_norm_ does; None or <= 0: no clipping and no norm launch.
    consume_grads: the update stores zeros over each gradient it has read, so the next zero_grad() has nothing to do and gradients never move.
    last_total_norm: after a clipped step the device tensor clip_grad_norm_ would have returned (never read back here).
    exp_avg / exp_avg_sq live in two flat buffers; state[p] holds views of them and of the device step counter.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, max_grad_norm=None,
                 consume_grads=False, amsgrad=False, maximize=False, names=None):
        if amsgrad:
            raise ValueError("FusedAdam: amsgrad=True is not built (the fused step keeps no max of exp_avg_sq)")
        if maximize:
            raise ValueError("FusedAdam: maximize=True is not built")
        if not 0.0 <= lr:
            raise ValueError(f"FusedAdam: invalid lr {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: invalid betas {betas}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.consume_grads = bool(consume_grads)
        self.last_total_norm = None
        self.table_uploads = 0
        self._names = names or {}
        self._lib = _lib.load()
        self._chunk = self._lib.sv_optim_chunk_elems()
        assert self._lib.sv_optim_chunk_bytes() == _CHUNK_DTYPE.itemsize
        if len(self.param_groups) > self._lib.sv_optim_max_groups():
            raise ValueError(f"FusedAdam: {len(self.param_groups)} parameter groups, at most {self._lib.sv_optim_max_groups()} are built")
        self._params, self._group_of = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                self._params.append(p)
                self._group_of.append(gi)
        for i in range(len(self._params)):
            self._check_param(i)
        self._key = None
        self._exp_avg = None
        self._consumed = False
        self._nchunks = self._npresent = 0
        self._table = self._present = self._partials = None

    # ---- refusals -------------------------------------------------------------------------------------------------------------------
    def _name(self, i):
        p = self._params[i]
        given = self._names.get(id(p)) if isinstance(self._names, dict) else None
        where = f"parameter {i} (group {self._group_of[i]}, shape {tuple(p.shape)})"
        return f"{given!r}, {where}" if given else where

    def _check_param(self, i):
        p = self._params[i]
        if not p.is_cuda:
            raise _lib.SeevcnHipError(f"FusedAdam: {self._name(i)} is a CPU tensor; seevcn_amd ops run on the GPU only, there is no CPU fallback")
        if p.dtype != torch.float32:
            raise TypeError(f"FusedAdam: {self._name(i)} is {p.dtype}; only fp32 parameters are built")
        if not p.is_contiguous():
            raise ValueError(f"FusedAdam: {self._name(i)} is not contiguous")
        if p.device != self._params[0].device:
            raise ValueError(f"FusedAdam: {self._name(i)} is on {p.device}, the first parameter on {self._params[0].device}")

    def _check_grad(self, i, g):
        if g.layout != torch.strided:
            raise ValueError(f"FusedAdam: the gradient of {self._name(i)} is sparse ({g.layout}); only dense gradients are built")
        if not g.is_cuda:
            raise _lib.SeevcnHipError(f"FusedAdam: the gradient of {self._name(i)} is a CPU tensor")
        if g.dtype != torch.float32:
            raise TypeError(f"FusedAdam: the gradient of {self._name(i)} is {g.dtype}; only fp32 gradients are built")
        if not g.is_contiguous():
            raise ValueError(f"FusedAdam: the gradient of {self._name(i)} is not contiguous")
        if g.shape != self._params[i].shape:
            raise ValueError(f"FusedAdam: the gradient of {self._name(i)} has shape {tuple(g.shape)}")

    # ---- state ----------------------------------------------------------------------------------------------------------------------
    def _ensure_buffers(self):
        """The two flat moment buffers (each tensor's slice starts on a 16-byte boundary), the device step counters and the views in state[p]."""
        if self._exp_avg is not None:
            return
        dev = self._params[0].device
        offs, total = [], 0
        for p in self._params:
            offs.append(total)
            total += _round_up(p.numel(), 4)
        self._offsets = offs
        n = len(self._params)
        self._exp_avg = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        self._t = torch.zeros(n, dtype=torch.int32, device=dev)
        self._tensor_scal = torch.zeros(2 * n, dtype=torch.float32, device=dev)
        self._norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
        for i, p in enumerate(self._params):
            o, k = offs[i], p.numel()
            self.state[p] = {"step": self._t[i], "exp_avg": self._exp_avg[o:o + k].view(p.shape), "exp_avg_sq": self._exp_avg_sq[o:o + k].view(p.shape)}

    def _rebuild(self, key):
        """The chunk table of the parameters that have a gradient, and its upload: once per change of the (parameter, gradient) addresses."""
        C = self._chunk
        rows, present = [], []
        m0, v0 = self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr()
        for i, (pa, ga) in enumerate(key):
            if ga is None:
                continue
            self._check_param(i)
            self._check_grad(i, self._params[i].grad)
            present.append((i, self._group_of[i]))
            n = self._params[i].numel()
            if n == 0:
                continue
            start = np.arange(0, n, C, dtype=np.int64)
            r = np.zeros(len(start), dtype=_CHUNK_DTYPE)
            b = (start * 4).astype(np.uint64)
            r["p"], r["g"] = np.uint64(pa) + b, np.uint64(ga) + b
            r["m"], r["v"] = np.uint64(m0 + 4 * self._offsets[i]) + b, np.uint64(v0 + 4 * self._offsets[i]) + b
            r["n"] = np.minimum(C, n - start)
            r["tensor"], r["group"] = i, self._group_of[i]
            rows.append(r)
        table = np.concatenate(rows) if rows else np.zeros(0, dtype=_CHUNK_DTYPE)
        pres = np.asarray(present, dtype=np.int32).reshape(-1, 2)
        self._nchunks, self._npresent = len(table), len(pres)
        blob = np.concatenate([table.view(np.uint8).reshape(-1), pres.view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])
        dev = self._params[0].device
        self._blob = torch.from_numpy(blob).pin_memory().to(dev, non_blocking=True)
        self.table_uploads += 1
        self._table = self._blob.data_ptr()
        self._present = self._table + table.nbytes
        if self._partials is None or self._partials.numel() < self._nchunks:
            self._partials = torch.empty(max(self._nchunks, 1), dtype=torch.float64, device=dev)
        self._key = key

    def _group_scalars(self, decay_override):
        vals = []
        for gi, g in enumerate(self.param_groups):
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError(f"FusedAdam: group {gi} asks for amsgrad / maximize, which are not built")
            wd, dec = g["weight_decay"], g.get("decoupled_weight_decay", self.defaults["decoupled_weight_decay"])
            if decay_override is not None:
                wd, dec = decay_override[gi]
            mode = NO_DECAY if wd == 0 else (DECOUPLED if dec else L2)
            b1, b2 = g["betas"]
            vals += [float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(wd), float(mode)]
        return (ctypes.c_double * len(vals))(*vals)

    # ---- the step -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, decay_override=None):
        """One fused step.  decay_override: per group (weight_decay, decoupled) used instead of the group's own keys (OptimWrapper's true_wd)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._ensure_buffers()
        try:
            key = tuple([(p.data_ptr(), None if p.grad is None else p.grad.data_ptr()) for p in self._params])
        except RuntimeError:
            for i, p in enumerate(self._params):
                if p.grad is not None:
                    self._check_grad(i, p.grad)
            raise
        if key != self._key:
            self._rebuild(key)
        groups = self._group_scalars(decay_override)
        max_norm = self.max_grad_norm
        clipped = max_norm is not None and max_norm > 0 and self._nchunks > 0
        if clipped:
            _lib.launch("sv_optim_grad_sqnorm", self._table, self._nchunks, self._partials.data_ptr())
        _lib.launch("sv_optim_adam_step", self._table, self._nchunks, self._present, self._npresent, groups, len(self.param_groups),
                    self._partials.data_ptr() if clipped else None, float(max_norm) if clipped else 0.0,
                    int(self.consume_grads), self._t.data_ptr(), self._tensor_scal.data_ptr(), self._norm_out.data_ptr())
        self.last_total_norm = self._norm_out[0] if clipped else None
        self._consumed = self.consume_grads
        return loss

    def zero_grad(self, set_to_none=True):
        """With consume_grads the step has already stored zeros over the gradients: the zero_grad() that follows it does nothing (and keeps the
        gradients where they are).  A zero_grad() that does not directly follow a step zeroes in place."""
        if self.consume_grads:
            if not self._consumed:
                grads = [p.grad for p in self._params if p.grad is not None]
                if grads:
                    torch._foreach_zero_(grads)
            self._consumed = False
            return
        super().zero_grad(set_to_none=set_to_none)

    # ---- checkpoints in torch.optim.Adam's layout -----------------------------------------------------------------------------------
    def state_dict(self):
        """{'state': {index: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]} as torch.optim.Adam writes it: parameters that have
        never stepped have no entry, 'step' is a float32 scalar.  Reads the step counters back (the only host read of this class)."""
        groups, start = [], 0
        for g in self.param_groups:
            packed = {k: v for k, v in g.items() if k != "params"}
            packed["params"] = list(range(start, start + len(g["params"])))
            start += len(g["params"])
            groups.append(packed)
        state = {}
        if self._exp_avg is not None:
            for i, t in enumerate(self._t.tolist()):
                if t > 0:
                    s = self.state[self._params[i]]
                    state[i] = {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": s["exp_avg"].clone(), "exp_avg_sq": s["exp_avg_sq"].clone()}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups):
            raise ValueError(f"FusedAdam.load_state_dict: {len(groups)} parameter groups in the checkpoint, {len(self.param_groups)} here")
        order = []
        for gi, (g, sg) in enumerate(zip(self.param_groups, groups)):
            if len(sg["params"]) != len(g["params"]):
                raise ValueError(f"FusedAdam.load_state_dict: group {gi} has {len(sg['params'])} parameters in the checkpoint, {len(g['params'])} here")
            order += list(sg["params"])
        for g, sg in zip(self.param_groups, groups):
            for k, v in sg.items():
                if k != "params":
                    g[k] = tuple(v) if k == "betas" else v
        self._group_scalars(None)
        self._ensure_buffers()
        self._exp_avg.zero_()
        self._exp_avg_sq.zero_()
        steps = [0] * len(self._params)
        for saved_id, s in state_dict["state"].items():
            i = order.index(saved_id)
            mine = self.state[self._params[i]]
            for k in ("exp_avg", "exp_avg_sq"):
                if tuple(s[k].shape) != tuple(mine[k].shape):
                    raise ValueError(f"FusedAdam.load_state_dict: {k} of {self._name(i)} has shape {tuple(s[k].shape)} in the checkpoint")
                mine[k].copy_(torch.as_tensor(s[k]).to(torch.float32))
            steps[i] = int(float(s["step"]))
        self._t.copy_(torch.tensor(steps, dtype=torch.int32))
