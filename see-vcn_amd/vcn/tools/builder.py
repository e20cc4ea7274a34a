"""build_opti_sche for a VCN config (see/surface_completion/models/vcn/tools/builder.py:49-76): AdamW / Adam over seevcn_amd.optim.FusedAdam,
SGD and the schedulers from torch."""
import torch

from ...optim import FusedAdam


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def build_lambda_sche(opti, config):
    """LambdaLR with lr_decay ** (epoch / decay_step), floored at lowest_decay (utils/misc.py:42-48 of the reference)."""
    step = _get(config, "decay_step")
    if step is None:
        raise NotImplementedError("scheduler LambdaLR needs kwargs.decay_step")
    decay, lowest = _get(config, "lr_decay"), _get(config, "lowest_decay")
    return torch.optim.lr_scheduler.LambdaLR(opti, lambda e: max(decay ** (e / step), lowest))


def build_opti_sche(base_model, config, steps_per_epoch, epochs):
    opti = _get(config, "optimizer")
    kind, kwargs = _get(opti, "type"), dict(_get(opti, "kwargs") or {})
    names = {id(p): n for n, p in base_model.named_parameters()}
    if kind == "AdamW":
        kwargs.setdefault("weight_decay", 1e-2)                                   # torch.optim.AdamW's default
        optimizer = FusedAdam(base_model.parameters(), decoupled_weight_decay=True, names=names, **kwargs)
    elif kind == "Adam":
        optimizer = FusedAdam(base_model.parameters(), names=names, **kwargs)
    elif kind == "SGD":
        optimizer = torch.optim.SGD(base_model.parameters(), nesterov=True, **kwargs)
    else:
        raise NotImplementedError(f"optimizer.type {kind!r} (AdamW, Adam and SGD are built)")

    sche = _get(config, "scheduler")
    kind, kwargs = _get(sche, "type"), dict(_get(sche, "kwargs") or {})
    if kind == "LambdaLR":
        scheduler = build_lambda_sche(optimizer, kwargs)
    elif kind == "StepLR":
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, **kwargs)
    elif kind == "OneCycle":
        scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, steps_per_epoch=steps_per_epoch, epochs=epochs, **kwargs)
    else:
        raise NotImplementedError(f"scheduler.type {kind!r} (LambdaLR, StepLR and OneCycle are built)")

    if _get(config, "bnmscheduler") is not None:
        raise NotImplementedError("config key 'bnmscheduler': the BatchNorm-momentum scheduler of utils/misc.py is not built")
    return optimizer, scheduler
