"""Focal sparse conv at voxel_rcnn_car.yaml sizes (KITTI range, 5 cm x 5 cm x 10 cm voxels, 41 x 1600 x 1408 grid): a few synthetic scenes through a
seeded VoxelBackBone8xFocal in eval mode, the inputs of its three focal layers captured, and per layer
  * the expansion path (sv_focal_select / _expand / _place behind spconv.focal.focal_expand) against a plain-torch GPU statement of the reference's
    algorithm written here -- a per-scene loop of sort, boolean indexing, repeat, cat, unique_consecutive, index_add_ and scatter_, as split_voxels /
    check_repeat / combine_out do it, but on the true linear cell key so that the two can be compared; they are asserted to agree before anything
    is timed;
  * conv_imp (C -> 27) on its two routes: the VALU gather-GEMM as it is, and the planned MFMA kernel with the weight zero-padded to 32 output rows.
Time: device events around windows of calls behind a warm-up, median with range.  Launches: torch.profiler over one call.  Host reads: the
synchronising calls torch reports in one call (torch.cuda.set_sync_debug_mode).  Needs a GPU.

    python tools/focal_conv_micro.py [--out profiles/focal_conv.txt] [--scenes 4] [--windows 9] [--calls 5]
"""
import argparse
import os
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANGE, VOXEL, GRID = [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1], [1408, 1600, 40]


def torch_statement(feats, indices, s, batch, shape, topk, threshold, mask_multi, skip_mask_kernel):
    """(out_features, out_indices): the reference's sequence in plain torch on the device, cells keyed by ((z * Y) + y) * X + x per scene."""
    dev = feats.device
    Z, Y, X = shape
    offs = torch.tensor([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], device=dev)

    def dedup(f, c, add=None):
        key = (c[:, 1].long() * Y + c[:, 2].long()) * X + c[:, 3].long()
        key, order = key.sort()
        f, c = f[order], c[order]
        uniq, inverse, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
        fn = torch.zeros((uniq.shape[0], f.shape[1]), device=dev).index_add_(0, inverse, f)
        perm = torch.arange(inverse.shape[0], device=dev)
        first = inverse.new_empty(uniq.shape[0]).scatter_(0, inverse, perm)
        if add is not None:
            add = torch.zeros((uniq.shape[0],), device=dev).index_add_(0, inverse, add[order]) / counts
        return fn, c[first], add

    out_f, out_c = [], []
    for b in range(batch):
        sel = indices[:, 0] == b
        c_b, f_b, s_b = indices[sel], feats[sel], s[sel]
        mv, mk = s_b[:, -1], s_b[:, :-1]
        if mask_multi:
            f_b = f_b * mv.unsqueeze(-1)
        if topk:
            order = mv.sort(descending=True)[1]
            k = int(mv.shape[0] * threshold)
            i_fore, i_back = order[:k], order[k:]
        else:
            i_fore, i_back = mv > threshold, mv <= threshold
        f_fore, c_fore, mk_fore = f_b[i_fore], c_b[i_fore], mk[i_fore]
        keep = mk_fore >= threshold
        cand = (c_fore[:, 1:].unsqueeze(1).repeat(1, 26, 1) + offs.unsqueeze(0).repeat(c_fore.shape[0], 1, 1))[keep]
        w_cand = mk_fore[keep]
        inside = (cand > 0).all(1) & (cand[:, 0] < Z) & (cand[:, 1] < Y) & (cand[:, 2] < X)
        cand, w_cand = cand[inside], w_cand[inside]
        cand = torch.cat([torch.full((cand.shape[0], 1), b, device=dev, dtype=cand.dtype), cand], dim=1)
        f_all = torch.cat([f_fore, torch.zeros((cand.shape[0], f_b.shape[1]), device=dev)], dim=0)
        c_all = torch.cat([c_fore, cand.to(c_fore.dtype)], dim=0)
        w_all = torch.cat([torch.ones(f_fore.shape[0], device=dev), w_cand], dim=0)
        f_all, c_all, w_all = dedup(f_all, c_all, w_all)
        if not skip_mask_kernel:
            f_all = f_all * w_all.unsqueeze(-1)
        f_all, c_all, _ = dedup(torch.cat([f_all, f_b[i_back]], dim=0), torch.cat([c_all, c_b[i_back]], dim=0))
        out_f.append(f_all), out_c.append(c_all)
    return torch.cat(out_f, dim=0), torch.cat(out_c, dim=0)


def timed(fn, windows, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def launches_of_one_call(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        return len(ev) if ev else None
    except Exception as e:
        print("profiler:", repr(e), file=sys.stderr)
        return None


def host_reads_of_one_call(fn):
    """Synchronising calls torch reports during one call (a .item(), a boolean index, a nonzero ...), or None where the debug mode is not there."""
    try:
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        hits = [str(w.message).splitlines()[0] for w in seen if "called a synchronizing" in str(w.message)]      # not the mode's own "prototype feature" notice
        for h in sorted(set(hits)):
            print(f"  sync x{hits.count(h)}: {h}", file=sys.stderr)
        return len(hits)
    except Exception as e:
        print("sync debug mode:", repr(e), file=sys.stderr)
        return None


def fmt(ms):
    return f"median {ms[0]:8.3f} ms (min {ms[1]:.3f}, max {ms[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    import seevcn_amd.spconv as spconv
    import seevcn_amd.spconv.functional as Fsp
    import seevcn_amd.synth as synth
    from seevcn_amd.pcdet.models import backbones_3d
    from seevcn_amd.pcdet.models.backbones_3d.focal_sparse_conv import FocalSparseConv
    from seevcn_amd.pcdet.ops import voxel_ops
    from seevcn_amd.seeding import seeded_state_dict
    from seevcn_amd.spconv import focal
    dev = torch.device("cuda:0")
    pts, _ = synth.make_scene_batch(a.scenes, seed=2000)
    feats, coords, _ = voxel_ops.voxelize_dynamic(torch.from_numpy(pts).to(dev).contiguous(), RANGE, VOXEL, GRID, a.scenes)
    net = backbones_3d.__all__["VoxelBackBone8xFocal"](dict(USE_IMG=False), feats.shape[1], GRID)
    net.load_state_dict(seeded_state_dict(net, seed=4))
    net = net.to(dev).eval()
    captured = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: captured.append((mod, args[0]))) for m in net.modules() if isinstance(m, FocalSparseConv)]
    with torch.no_grad():
        net({"batch_size": a.scenes, "voxel_features": feats, "voxel_coords": coords})
    for h in hooks:
        h.remove()
    lines = [f"focal sparse conv, {a.scenes} synthetic scenes, {feats.shape[0]} input voxels, grid {[GRID[2] + 1, GRID[1], GRID[0]]}; top-k, threshold 0.5 "
             f"(the yaml's defaults); {a.windows} windows of {a.calls} calls each"]
    with torch.no_grad():
        for mod, x in captured:
            x = spconv.SparseConvTensor(x.features.contiguous(), x.indices, x.spatial_shape, x.batch_size)        # a dictionary of its own
            n, C = x.features.shape
            rb = mod.conv_imp.get_rulebook(x)
            w = mod.conv_imp.weight_kio().detach()
            w32 = F.pad(w, (0, 5)).contiguous()
            valu = lambda: Fsp.SparseConvFunction.apply(x.features, w, rb)
            pad32 = lambda: Fsp.SparseConvFunction.apply(x.features, w32, rb)[:, :27]
            planned = rb.plan("fwd", C, 32) is not None
            assert rb.plan("fwd", C, 27) is None, "the 27-channel layer is expected on the VALU gather-GEMM"
            d = float((valu() - pad32()).abs().max())
            s = valu().sigmoid()
            kw = dict(topk=mod.topk, threshold=mod.threshold, mask_multi=mod.mask_multi, skip_mask_kernel=mod.skip_mask_kernel)
            ours = lambda: focal.focal_expand(x, s, rb.nbr_out, **kw)[0]
            plain = lambda: torch_statement(x.features, x.indices, s, x.batch_size, x.spatial_shape, **kw)
            got, (want_f, want_c) = ours(), plain()
            assert torch.equal(got.indices, want_c.int()), "the two statements list different cells"
            err = float((got.features - want_f).abs().max())
            assert err <= 1e-5 * float(want_f.abs().max()), err
            lines.append(f"{mod.conv.indice_key}: C = {C}, grid {x.spatial_shape}, {n} -> {got.indices.shape[0]} voxels (x{got.indices.shape[0] / n:.2f}); "
                         f"max |ours - torch| = {err:.2e}")
            for name, fn in (("expansion, HIP entries", ours), ("expansion, plain-torch statement", plain)):
                lines.append(f"    {name:<36s} {fmt(timed(fn, a.windows, a.calls))}   launches {launches_of_one_call(fn)}   host reads {host_reads_of_one_call(fn)}")
            lines.append(f"    {'conv_imp, VALU gather-GEMM (27)':<36s} {fmt(timed(valu, a.windows, a.calls))}   launches {launches_of_one_call(valu)}")
            lines.append(f"    {'conv_imp, padded to 32 ' + ('(planned MFMA)' if planned else '(NOT planned)'):<36s} {fmt(timed(pad32, a.windows, a.calls))}   "
                         f"launches {launches_of_one_call(pad32)}   max |valu - padded| = {d:.2e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
