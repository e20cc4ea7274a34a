"""OptimWrapper: the surface of detector3d/tools/train_utils/optimization/fastai_optim.py (fastai's hyper-parameter wrapper over layer-group pairs)
written over seevcn_amd.optim.FusedAdam.

Layer groups are split in two, non-BatchNorm children first, so param_groups[0::2] are the weights and param_groups[1::2] the BatchNorm parameters
of each layer group: the reference's even / odd order, which its checkpoints carry.  With true_wd the reference multiplies every parameter tensor by
1 - wd * lr in a Python loop before Adam's step (:138-151); here the same factor goes into the fused launch as the group's decoupled decay.
"""
from collections.abc import Iterable

from torch import nn

from ....optim import FusedAdam

bn_types = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)


def split_bn_bias(layer_groups):
    """Each layer group as two nn.Sequential: its non-BatchNorm children, then its BatchNorm children."""
    out = []
    for group in layer_groups:
        kids = list(group.children())
        out.append(nn.Sequential(*[c for c in kids if not isinstance(c, bn_types)]))
        out.append(nn.Sequential(*[c for c in kids if isinstance(c, bn_types)]))
    return out


def listify(p=None, q=None):
    """p as a list as long as q (an int, or something with a length); a single value is repeated."""
    if p is None:
        p = []
    elif isinstance(p, str) or not isinstance(p, Iterable):
        p = [p]
    p = list(p)
    if isinstance(q, int) and not isinstance(q, bool):
        n = q
    else:
        n = len(p) if q is None else len(q)
    if len(p) == 1:
        p = p * n
    assert len(p) == n, f"List len mismatch ({len(p)} vs {n})"
    return p


def trainable_params(m):
    return [p for p in m.parameters() if p.requires_grad]


class OptimWrapper:
    """Hyper-parameters of the wrapped optimizer as properties over the layer-group pairs: lr, mom (beta1 or momentum), beta (beta2 or alpha), wd."""

    def __init__(self, opt, wd, true_wd=False, bn_wd=True):
        self.opt, self.true_wd, self.bn_wd = opt, true_wd, bn_wd
        self.opt_keys = [k for k in self.opt.param_groups[0] if k != "params"]
        self.read_defaults()
        self.wd = wd

    @classmethod
    def create(cls, opt_func, lr, layer_groups, **kwargs):
        groups = split_bn_bias(layer_groups)
        opt = cls(opt_func([{"params": trainable_params(g), "lr": 0} for g in groups]), **kwargs)
        opt.lr, opt.opt_func = listify(lr, layer_groups), opt_func
        return opt

    def new(self, layer_groups):
        """A wrapper with the same hyper-parameters over other layer groups."""
        opt_func = getattr(self, "opt_func", self.opt.__class__)
        return self.create(opt_func, self.lr, layer_groups, wd=self.wd, true_wd=self.true_wd, bn_wd=self.bn_wd)

    def __repr__(self):
        return f"OptimWrapper over {self.opt!r}.\nTrue weight decay: {self.true_wd}"

    def step(self):
        """With true_wd: decoupled decay by wd * lr on the even groups, and on the odd (BatchNorm) groups when bn_wd, inside the fused launch; the
        optimizer's own weight_decay keys read 0 afterwards, as in the reference."""
        if not self.true_wd:
            self.opt.step()
            return
        decay = []
        for wd in self._wd:
            decay += [(wd, True), (wd if self.bn_wd else 0.0, True)]
        self.set_val("weight_decay", listify(0, self._wd))
        if isinstance(self.opt, FusedAdam):
            self.opt.step(decay_override=decay)
        else:
            raise NotImplementedError(f"OptimWrapper: true_wd is built over FusedAdam only, not {type(self.opt).__name__}")

    def zero_grad(self):
        self.opt.zero_grad()

    def __getattr__(self, k):
        if k == "opt":
            raise AttributeError(k)
        return getattr(self.opt, k, None)

    def clear(self):
        """Forget the optimizer's moments and step counts."""
        sd = self.state_dict()
        sd["state"] = {}
        self.load_state_dict(sd)

    @property
    def lr(self):
        return self._lr[-1]

    @lr.setter
    def lr(self, val):
        self._lr = self.set_val("lr", listify(val, self._lr))

    @property
    def mom(self):
        return self._mom[-1]

    @mom.setter
    def mom(self, val):
        val = listify(val, self._mom)
        if "momentum" in self.opt_keys:
            self.set_val("momentum", val)
        elif "betas" in self.opt_keys:
            self.set_val("betas", (val, self._beta))
        self._mom = val

    @property
    def beta(self):
        return None if self._beta is None else self._beta[-1]

    @beta.setter
    def beta(self, val):
        if val is None:
            return
        val = listify(val, self._beta)
        if "betas" in self.opt_keys:
            self.set_val("betas", (self._mom, val))
        elif "alpha" in self.opt_keys:
            self.set_val("alpha", val)
        self._beta = val

    @property
    def wd(self):
        return self._wd[-1]

    @wd.setter
    def wd(self, val):
        val = listify(val, self._wd)
        if not self.true_wd:
            self.set_val("weight_decay", val, bn_groups=self.bn_wd)
        self._wd = val

    def read_defaults(self):
        self._beta = None
        if "lr" in self.opt_keys:
            self._lr = self.read_val("lr")
        if "momentum" in self.opt_keys:
            self._mom = self.read_val("momentum")
        if "alpha" in self.opt_keys:
            self._beta = self.read_val("alpha")
        if "betas" in self.opt_keys:
            self._mom, self._beta = self.read_val("betas")
        if "weight_decay" in self.opt_keys:
            self._wd = self.read_val("weight_decay")

    def set_val(self, key, val, bn_groups=True):
        """val[i] into layer group i: its even param group, and its odd one when bn_groups.  A tuple of lists is zipped into per-group tuples."""
        if isinstance(val, tuple):
            val = list(zip(*val))
        groups = self.opt.param_groups
        for v, even, odd in zip(val, groups[0::2], groups[1::2]):
            even[key] = v
            if bn_groups:
                odd[key] = v
        return val

    def read_val(self, key):
        val = [g[key] for g in self.opt.param_groups[0::2]]
        if isinstance(val[0], tuple):
            val = [v[0] for v in val], [v[1] for v in val]
        return val


class FastAIMixedOptim(OptimWrapper):
    """The reference's fp16 model / fp32 master wrapper (fastai_optim.py:238-264) is not built: parameters here are fp32."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("FastAIMixedOptim is not built: FusedAdam steps fp32 parameters only (no fp16 model copy, no loss scale)")

    @classmethod
    def create(cls, *args, **kwargs):
        raise NotImplementedError("FastAIMixedOptim is not built: FusedAdam steps fp32 parameters only (no fp16 model copy, no loss scale)")
