"""Generate tests/golden/kitti_eval.npz by running the REFERENCE's own kitti_object_eval_python/eval.py on the seeded annotations of
kitti_eval_inputs.py (both detection sets, class lists ['Car', 'Pedestrian', 'Cyclist'] and ['Car']).

numba is absent, so eval.py and rotate_iou.py are loaded by path under a stub `numba` installed HERE: _refimport.install_stubs()'s `jit` returns
its inner lambda for the bare `@numba.jit` on get_thresholds, so this stub returns the function itself when called with a single callable; it adds
numba.float32 and a cuda.local.array that returns np.zeros.  rotate_iou_gpu_eval (a CUDA launch) is replaced by a per-pair loop over the
reference's own device functions (devRotateIoUEval) on float32 arrays; pairs whose circumscribed circles are apart are 0 without the call (every
test of the algorithm fails for them), and results are cached by content because every eval_class recomputes them.  pcdet.datasets is not imported.

This pins the matching, the thresholds, the AP arithmetic and the result string to the reference.  The overlap values are the reference's
statements on float32 arrays with Python-float intermediates where numba would type differently, so they agree with an fp32 kernel to fp32
rounding only (tests/kitti_eval_reference.py, header).

Run only where the reference checkout is present (SEEVCN_REFERENCE):  python tests/golden/make_kitti_eval_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kitti_eval_inputs as I  # noqa: E402

REF = os.environ.get("SEEVCN_REFERENCE", "/root/reference")
PKG = os.path.join(REF, "detector3d", "pcdet", "datasets", "kitti", "kitti_object_eval_python")


def _jit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda f: f


numba = types.ModuleType("numba")
numba.jit = numba.njit = _jit
numba.float32 = np.float32
cuda = types.ModuleType("numba.cuda")
cuda.jit = _jit
cuda.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype=dtype))
numba.cuda = cuda
sys.modules["numba"], sys.modules["numba.cuda"] = numba, cuda

pkg = types.ModuleType("ref_kitti_eval")
pkg.__path__ = [PKG]
sys.modules["ref_kitti_eval"] = pkg


def _load(name):
    spec = importlib.util.spec_from_file_location("ref_kitti_eval." + name, os.path.join(PKG, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


rot = _load("rotate_iou")
_cache = {}


def rotate_iou_cpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    boxes, query_boxes = boxes.astype(np.float32), query_boxes.astype(np.float32)
    key = (boxes.tobytes(), query_boxes.tobytes(), criterion)
    if key not in _cache:
        iou = np.zeros((boxes.shape[0], query_boxes.shape[0]), dtype=np.float32)
        half = lambda b: 0.5 * np.hypot(b[:, 2].astype(np.float64), b[:, 3].astype(np.float64))
        dist = np.hypot(boxes[:, None, 0].astype(np.float64) - query_boxes[None, :, 0], boxes[:, None, 1].astype(np.float64) - query_boxes[None, :, 1])
        for n, k in zip(*np.nonzero(dist <= 1.01 * (half(boxes)[:, None] + half(query_boxes)[None, :]) + 1e-3)):
            iou[n, k] = rot.devRotateIoUEval(query_boxes[k], boxes[n], criterion)          # the argument roles of rotate_iou_kernel_eval
        _cache[key] = iou
    return _cache[key].copy()


rot.rotate_iou_gpu_eval = rotate_iou_cpu_eval
ev = _load("eval")
assert ev.rotate_iou_gpu_eval is rotate_iou_cpu_eval

recorded = []
_eval_class = ev.eval_class


def eval_class_recorded(*args, **kwargs):
    ret = _eval_class(*args, **kwargs)
    recorded.append(ret)
    return ret


ev.eval_class = eval_class_recorded          # do_eval looks the name up in its module

gt_annos, dt_annos, dt_noalpha = I.make_inputs()
margin, bound = I.check_conditions(gt_annos, dt_annos)
print("fixture: smallest margin to a min_overlap %.3e, largest pair bound %.3e" % (margin, bound))

out = {}
out.update(I.pack(gt_annos, "gt"))
out.update(I.pack(dt_annos, "dt"))
for metric in (0, 1, 2):          # the reference's per-frame blocks (detections as rows, as eval_class asks for them)
    blocks = ev.calculate_iou_partly(dt_annos, gt_annos, metric, 100)[0]
    out["overlaps_%d" % metric] = np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1) for b in blocks])
for set_name, dets in (("alpha", dt_annos), ("noalpha", dt_noalpha)):
    for cls_name, classes in (("cpc", ["Car", "Pedestrian", "Cyclist"]), ("car", ["Car"])):
        del recorded[:]
        detail = {}
        result, ret_dict = ev.get_official_eval_result(gt_annos, dets, classes, PR_detail_dict=detail)
        tag = "%s_%s" % (set_name, cls_name)
        out[tag + "_result"] = np.array(result)
        out[tag + "_ret_keys"] = np.array(list(ret_dict.keys()))
        out[tag + "_ret_values"] = np.array([float(v) for v in ret_dict.values()], dtype=np.float64)
        assert len(recorded) == 3
        for metric, ret in enumerate(recorded):
            for k in ("recall", "precision", "orientation"):
                out["%s_m%d_%s" % (tag, metric, k)] = ret[k]
        for k, v in detail.items():
            assert np.array_equal(v, recorded[{"bbox": 0, "aos": 0, "bev": 1, "3d": 2}[k]]["orientation" if k == "aos" else "precision"])
        print(tag)
        print(result)
path = os.path.join(HERE, "kitti_eval.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
