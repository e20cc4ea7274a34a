"""GPU: the VCN validation-metric kernels (csrc/vc_metrics.hip) and their host layer against tests/vc_metrics_reference.py."""
import numpy as np
import pytest
import torch

import vc_metrics_reference as R

pytestmark = pytest.mark.gpu


def _on(case, dev):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pred = {"coarse": t(case["coarse"])}
    if case["reg_rot"] is not None:
        pred["reg_rot"], pred["reg_centre"] = t(case["reg_rot"]), t(case["reg_centre"])
    gt = {"complete": t(case["complete"]), "gt_boxes": t(case["gt_boxes"]), "num_pts": case["num_pts"]}
    return pred, gt


def _table(case, dev):
    from seevcn_amd.vcn.utils import metrics as M
    pred, gt = _on(case, dev)
    tab = M.objects_table(pred["coarse"], gt["complete"], gt["gt_boxes"], pred.get("reg_rot"), pred.get("reg_centre")).cpu()
    return tab.numpy().astype(np.float64), tab.view(torch.int32).numpy()


def test_layout_constants(cuda, hip_lib):
    from seevcn_amd.vcn.utils import metrics as M
    assert hip_lib.sv_vc_metrics_tile() == R.TILE
    assert hip_lib.sv_vc_metrics_columns() == M.COLUMNS


@pytest.mark.parametrize("index", range(len(R.cases())), ids=[c["name"] for c in R.cases()])
def test_object_table_against_restatement(cuda, hip_lib, index):
    """Integers exact, sums within the bounds derived from the stated order, the per-point minimum through sv_chamfer_forward's dist."""
    from seevcn_amd.vcn.extensions.chamfer_dist import chamfer
    from seevcn_amd.vcn.utils import metrics as M
    case = R.cases()[index]
    t, _, _ = R.expected(index)
    f, i = _table(case, cuda)
    B, n, m = len(case["coarse"]), case["coarse"].shape[1], case["complete"].shape[1]
    assert np.array_equal(i[:, M.COL_NZ1], t["nz1"]) and np.array_equal(i[:, M.COL_NZ2], t["nz2"])
    assert np.array_equal(i[:, M.COL_NUM_OOB], t["num_oob"]) and np.array_equal(i[:, M.COL_NUM_PC], t["num_pc"])
    assert (i[:, 22] == n).all() and (i[:, 23] == m).all()
    assert np.array_equal(f[:, M.COL_OOB].astype(np.float32), t["ratio"])
    fails = []
    for col, key in enumerate(("d1", "s1", "d2", "s2", "zd1", "zs1", "zd2", "zs2")):
        err, tol = np.abs(f[:, col] - t[key]), t["tol_" + key]
        print("%-4s worst error %.3g, bound there %.3g" % (key, err.max(), tol[err.argmax()]))
        if (err > tol).any():
            fails.append("%s: object %d got %r want %r bound %r" % (key, err.argmax(), f[err.argmax(), col], t[key][err.argmax()], tol[err.argmax()]))
    dist1, dist2, _, _ = chamfer.forward(*[torch.from_numpy(case[k]).to(cuda) for k in ("coarse", "complete")])
    for col, dist, key in ((0, dist1, "d1"), (2, dist2, "d2")):
        want = dist.cpu().numpy().astype(np.float64).sum(1)
        if (np.abs(f[:, col] - want) > t["tol_" + key]).any():
            fails.append("%s: differs from the float64 sum of sv_chamfer_forward's dist" % key)
        assert np.array_equal(dist.cpu().numpy(), np.stack(t["dist" + key[1]]).astype(np.float32)), "sv_chamfer_forward vs the stated fp32 distance"
    err = np.abs(f[:, M.COL_BOX:M.COL_BOX + 6] - t["box"][:, :6])
    print("box  worst error / bound %.3g" % (err / np.maximum(t["tol_box"], 1e-300)).max())
    if (err > t["tol_box"]).any():
        fails.append("predicted box beyond its bound: %r" % (err / np.maximum(t["tol_box"], 1e-300)).max())
    for b in range(B):
        own = np.concatenate([f[b, M.COL_BOX:M.COL_BOX + 6], [case["gt_boxes"][b, 6]]])
        lo, hi = R.iou_interval(own, case["gt_boxes"][b])
        if not lo <= f[b, M.COL_IOU] <= hi:
            fails.append("IoU of object %d: %r outside [%r, %r]" % (b, f[b, M.COL_IOU], lo, hi))
        if abs(f[b, M.COL_IOU] - t["iou"][b]) > t["tol_iou"][b]:
            fails.append("IoU of object %d: %r, float64 %r, bound %r" % (b, f[b, M.COL_IOU], t["iou"][b], t["tol_iou"][b]))
    if case["reg_rot"] is None:
        assert (f[:, M.COL_ROT] == -1).all() and (f[:, M.COL_TRANS] == -1).all()
    else:
        for col, key in ((M.COL_ROT, "rot"), (M.COL_TRANS, "trans")):
            err = np.abs(f[:, col] - t[key])
            print("%-5s worst error / bound %.3g" % (key, (err / t["tol_" + key]).max()))
            if (err > t["tol_" + key]).any():
                fails.append("%s beyond its bound: object %d got %r want %r" % (key, err.argmax(), f[err.argmax(), col], t[key][err.argmax()]))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("index", range(len(R.cases())), ids=[c["name"] for c in R.cases()])
def test_thirty_values_get_counters_and_repeatability(cuda, hip_lib, index):
    from seevcn_amd.vcn.utils import metrics as M
    case = R.cases()[index]
    _, want, tols = R.expected(index)
    pred, gt = _on(case, cuda)
    M.reset_counters()
    got = M.Metrics.get(pred, gt)
    assert M.COUNTERS == {"library_calls": 2, "host_reads": 1}, (len(case["coarse"]), dict(M.COUNTERS))
    assert isinstance(got, list) and len(got) == 30 and all(type(v) is float for v in got)
    dev = M.Metrics.get_device(pred, gt)
    assert dev.is_cuda and dev.shape == (30,) and dev.dtype == torch.float32
    assert torch.equal(torch.tensor(got, dtype=torch.float32), dev.cpu())
    assert torch.equal(dev, M.Metrics.get_device(pred, gt)), "two runs differ"
    got = np.array(got)
    assert np.array_equal(got == -1, want == -1), (case["name"], got, want)
    err = np.abs(got - want)
    for k, name in enumerate(R.NAMES):
        print("%-22s got %-14.8g want %-14.8g error %.3g bound %.3g" % (name, got[k], want[k], err[k], tols[k]))
    bad = err > tols
    assert not bad.any(), [(R.NAMES[k], got[k], want[k], tols[k]) for k in np.flatnonzero(bad)]
    whole = M.Metrics.get(pred, gt, eval_by_num_pts=False)
    assert whole == [got[5 * k] for k in range(6)]


def test_get_oob_error_equals_the_ratios(cuda, hip_lib):
    from seevcn_amd.vcn.utils.losses import get_oob_error
    from seevcn_amd.vcn.utils.transform import rotm_to_heading
    for index in (2, 5, 6):
        case = R.cases()[index]
        t, _, _ = R.expected(index)
        got = get_oob_error(torch.from_numpy(case["coarse"]).to(cuda), torch.from_numpy(case["gt_boxes"]).to(cuda))
        assert got.dtype == torch.float32 and got.shape == (len(case["coarse"]),)
        assert np.array_equal(got.cpu().numpy(), t["ratio"])
    case = R.cases()[6]
    h = rotm_to_heading(torch.from_numpy(case["reg_rot"]).to(cuda)).cpu().numpy().astype(np.float64)
    want = np.array([np.arctan2(r[0, 1], r[0, 0]) for r in case["reg_rot"].astype(np.float64)])
    assert np.abs(h - want).max() <= (R.TRIG_ULPS + 4) * R.EPS32 * np.pi


def test_num_pts_forms(cuda, hip_lib):
    from seevcn_amd.vcn.utils.metrics import Metrics
    case = R.cases()[2]
    pred, gt = _on(case, cuda)
    base = Metrics.get(pred, gt)
    for form in (list(int(v) for v in case["num_pts"]), np.asarray(case["num_pts"], np.int32), torch.tensor(case["num_pts"]), torch.tensor(case["num_pts"]).to(cuda)):
        assert Metrics.get(pred, dict(gt, num_pts=form)) == base


def test_validate_vc_equals_the_host_fold(cuda, hip_lib):
    """validate_vc on a tiny eval-mode VCN_VC over three batches of two taxonomies: per-batch Metrics.get folded through AverageMeter, one read."""
    import seevcn_amd.vcn as V
    from seevcn_amd.seeding import seeded_state_dict
    from seevcn_amd.vcn.tools import runner
    from seevcn_amd.vcn.utils import metrics as M
    from seevcn_amd.vcn.utils.AverageMeter import AverageMeter
    from seevcn_amd.vcn.utils.bbox_utils import get_bbox_from_keypoints
    net = V.MODELS.build({"NAME": "VCN_VC"})
    net.load_state_dict(seeded_state_dict(net, seed=0))
    net = net.to(cuda).train()
    rng = np.random.default_rng(11)
    batches = []
    for tax, num_pts in (("02958343", [12, 250]), ("03790512", [40, 90]), ("02958343", [5, 5])):
        boxes = np.stack([R._rand_box(rng, rng.uniform(-3, 3)) for _ in range(2)])
        inp = np.stack([R._cloud_around(rng, b, 96, "inside") for b in boxes])
        complete = np.stack([R._cloud_around(rng, b, 300, "inside") for b in boxes])
        label = {"gt_boxes": torch.from_numpy(boxes), "num_pts": num_pts}
        batches.append(([tax, tax], ["m0", "m1"], (torch.from_numpy(inp), torch.from_numpy(complete), label)))
    M.reset_counters()
    result = runner.validate_vc(net, batches, epoch=3)
    assert M.COUNTERS == {"library_calls": 6, "host_reads": 1}
    assert not net.training
    assert isinstance(result, M.Metrics) and result.metric_name == "CDL1"
    category = {}
    for (tax, _, (inp, complete, label)) in batches:
        in_dict = {"input": inp.to(cuda), "gt_boxes": label["gt_boxes"].to(cuda), "num_pts": label["num_pts"], "complete": complete.to(cuda), "training": False}
        ret = net(in_dict)
        ret["pred_box"] = get_bbox_from_keypoints(ret["coarse"], in_dict["gt_boxes"])
        category.setdefault(tax[0], AverageMeter(M.Metrics.names())).update(M.Metrics.get(ret, in_dict))
    overall = AverageMeter(M.Metrics.names())
    for v in category.values():
        overall.update(v.avg())
    assert result.state_dict() == dict(zip(M.Metrics.names(), overall.avg()))
    assert result.state_dict()["CDL1"] > 0 and result.state_dict()["CDL1_L3"] > 0 and result.state_dict()["CDL1_L2"] > 0
    # test_vc: the widened box moves IOU_3D alone, the rotation names become medians of the positive per-batch values
    for b in batches:
        b[2][2]["dataset"] = ["waymo", "waymo"]
    tested = runner.test_vc(net, batches).state_dict()
    plain = runner.test_vc(net, [(a, b, (c[0], c[1], {k: v for k, v in c[2].items() if k != "dataset"})) for a, b, c in batches]).state_dict()
    for name in M.Metrics.names():
        if name.startswith("IOU_3D"):
            assert tested[name] != plain[name] or plain[name] in (-1, 0), name
        else:
            assert tested[name] == plain[name] or (np.isnan(tested[name]) and np.isnan(plain[name])), name
