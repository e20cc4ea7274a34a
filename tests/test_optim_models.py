"""GPU: one train step of the small SECOND config through build_optimizer / build_scheduler and one of VCN_VC through build_opti_sche, against the
same model stepped by the reference's route stated in plain torch (clip_grad_norm_, one mul_ per parameter, torch.optim.Adam / AdamW) from equal
gradients."""
import os
import sys

import numpy as np
import pytest
import torch

import optim_reference as OR
from oracle.tolerances import assert_close_per_channel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clones(params):
    out = []
    for p in params:
        q = torch.nn.Parameter(p.detach().clone())
        q.grad = p.grad.detach().clone()
        out.append(q)
    return out


def compare(params, ref, names):
    for p, r, n in zip(params, ref, names):
        assert_close_per_channel(p.detach().cpu().numpy(), r.detach().cpu().numpy(), rtol=1e-3, atol_frac=1e-4, name=n)


def test_second_step_equals_reference_route(cuda, hip_lib):
    sys.path.insert(0, ROOT)
    import bench_configs as BC
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet import model_cfgs as C
    from seevcn_amd.tools.train_utils import optimization as O
    cfg = OR.CASES["onecycle7"]["cfg"]
    pts, gt = synth.make_scene_batch(2, seed=2000, n_az=128)
    net = BC._detector(C.second_model_cfg(dynamic_vfe=True), 3, C.SyntheticDatasetInfo(), cuda, 5)
    opt = O.build_optimizer(net, cfg)
    sched, _ = O.build_scheduler(opt, 50, 2, -1, cfg)
    groups = [g["params"] for g in opt.opt.param_groups]
    names = {id(p): n for n, p in net.named_parameters()}
    assert {id(p) for g in groups for p in g} == {id(p) for p in net.parameters() if p.requires_grad}
    bn = {id(p) for m in net.modules() if isinstance(m, O.fastai_optim.bn_types) for p in m.parameters()}
    assert bn and {id(p) for p in groups[1]} == bn                  # BatchNorm parameters are the odd group, and nothing else is
    sched.step(0)
    opt.zero_grad()
    ret, _, _ = net({"batch_size": 2, "points": torch.from_numpy(pts).to(cuda), "gt_boxes": torch.from_numpy(gt).to(cuda)})
    ret["loss"].backward()
    assert all(p.grad is not None for g in groups for p in g)
    ref = [clones(g) for g in groups]
    lr, mom = opt.lr, opt.mom
    assert (lr, mom) == OR.one_cycle(0, 100, cfg.LR, cfg.MOMS, cfg.DIV_FACTOR, cfg.PCT_START)
    want_norm = torch.nn.utils.clip_grad_norm_([q for g in ref for q in g], cfg.GRAD_NORM_CLIP)
    with torch.no_grad():
        for g in ref:
            for q in g:
                q.mul_(1 - cfg.WEIGHT_DECAY * lr)
    torch.optim.Adam([{"params": g} for g in ref], lr=lr, betas=(mom, 0.99), weight_decay=0).step()
    opt.step()
    n = sum(p.numel() for g in groups for p in g)
    assert abs(float(opt.opt.last_total_norm) - float(want_norm)) <= ((n + 2) / 2 + 2) * OR.U * float(want_norm)
    compare([p for g in groups for p in g], [q for g in ref for q in g], [names[id(p)] for g in groups for p in g])


def vcn_step(cuda, fused):
    """Seeded VCN_VC, one forward + backward + step; returns (parameters, the plain-torch copies stepped by torch.optim.AdamW or None)."""
    import seevcn_amd.synth as synth
    import seevcn_amd.vcn as V
    from oracle import vcn_train as T
    from seevcn_amd.seeding import seeded_state_dict
    from seevcn_amd.vcn.tools import builder
    cfg = OR.CASES["adamw0"]["cfg"]
    clouds, boxes = synth.make_object_batch(8, seed=1000)
    m = V.MODELS.build({"NAME": "VCN_VC"})
    m.load_state_dict(seeded_state_dict(m, seed=0))
    m = m.to(cuda).train()
    opt, sched = builder.build_opti_sche(m, cfg, 10, 2)
    out = m({"input": torch.from_numpy(clouds).to(cuda), "gt_boxes": torch.from_numpy(boxes).to(cuda)})
    up = torch.randn(out["coarse"].shape, generator=torch.Generator().manual_seed(1))
    T.parity_loss(out, up.to(cuda)).backward()
    params = [p for p in m.parameters() if p.grad is not None]
    ref = None
    if not fused:
        ref = clones(params)
        torch.optim.AdamW(ref, **cfg.optimizer.kwargs).step()
    opt.step()
    sched.step()
    return [n for n, p in m.named_parameters() if p.grad is not None], params, ref


def test_vcn_step_equals_reference_route(cuda, hip_lib):
    names, params, ref = vcn_step(cuda, fused=False)
    assert len(params) >= 10
    compare(params, ref, names)


def test_vcn_step_with_ordered_gradients_repeats_bit_for_bit(cuda, hip_lib):
    import seevcn_amd
    with seevcn_amd.set_ordered_gradients(True):
        _, a, _ = vcn_step(cuda, fused=True)
        _, b, _ = vcn_step(cuda, fused=True)
    for x, y in zip(a, b):
        assert np.array_equal(x.detach().cpu().numpy(), y.detach().cpu().numpy())
