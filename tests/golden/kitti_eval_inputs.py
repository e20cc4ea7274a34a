"""Seeded annotations for the KITTI evaluation tests (tests/golden/kitti_eval.npz): about two dozen frames in camera coordinates with the classes
Car, Pedestrian, Cyclist, Van, Person_sitting, Truck and DontCare, every occlusion and truncation level, box heights on both sides of 25 and 40 px,
detections = jittered ground truths + false positives (some on DontCare regions, some of low height), a frame with nothing, one with ground truth
only, one with detections only, and one with 150 detections and 70 ground truths (both axes cross the wave width).  A second detection set is the
first with alpha = -10 (no AOS).

Two conditions hold by construction (the generator redraws a detection until they do; check_conditions() verifies them from scratch):
  * every (detection, ground truth) overlap of a frame, under each metric, and every detection / DontCare overlap of metric 0, is at least
    max(FIXTURE_MARGIN, 4 x the pair's fp32 bound) away from every min_overlap in use (0.7, 0.5, 0.25), so no match hangs on fp32 rounding;
  * the scores of a frame are distinct, so scores that compete for one ground truth never tie.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kitti_eval_reference as K  # noqa: E402

SEED = 20240607
NUM_FRAMES = 24
MIN_OVERLAPS_IN_USE = (0.7, 0.5, 0.25)
CLASSES = ["Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Truck"]
DIMS = {"Car": (3.9, 1.55, 1.6), "Pedestrian": (0.8, 1.75, 0.6), "Cyclist": (1.75, 1.7, 0.6), "Van": (5.0, 2.2, 1.9),        # l, h, w
        "Person_sitting": (0.8, 1.25, 0.6), "Truck": (10.0, 3.2, 2.6)}
CLASS_P = [0.4, 0.2, 0.15, 0.1, 0.07, 0.08]
FOCAL, CU, CV = 720.0, 620.0, 190.0
KEYS = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")


def _project(loc, dims):
    """A plausible image box for a 3-D box: pixel height ~ FOCAL * h / z, so the distance decides the side of the 25 / 40 px limits."""
    x, y, z = loc
    l, h, w = dims
    hp, wp = FOCAL * h / z, FOCAL * 0.7 * max(l, w) / z
    u, v = CU + FOCAL * x / z, CV + FOCAL * (y - h / 2) / z * 0.3
    return np.round(np.array([u - wp / 2, v - hp / 2, u + wp / 2, v + hp / 2]) * 4) / 4            # quarter pixels: exact in fp32


def _gt_object(rng):
    name = CLASSES[rng.choice(len(CLASSES), p=CLASS_P)]
    dims = np.round(np.array(DIMS[name]) * (1 + 0.08 * rng.randn(3)), 2)
    z = float(rng.choice([rng.uniform(5, 25), rng.uniform(25, 45), rng.uniform(45, 75)]))
    loc = np.round(np.array([rng.uniform(-0.45, 0.45) * z, rng.uniform(1.4, 1.9), z]), 2)
    ry = round(float(rng.uniform(-np.pi, np.pi)), 2)
    return dict(name=name, truncated=float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.6], p=[0.5, 0.15, 0.15, 0.1, 0.1])),
                occluded=int(rng.choice([0, 1, 2, 3], p=[0.5, 0.2, 0.2, 0.1])), alpha=round(float(ry - np.arctan2(loc[0], loc[2])), 2),
                bbox=_project(loc, dims), dimensions=dims, location=loc, rotation_y=ry)


def _dontcare(rng):
    u, v = rng.uniform(50, 1150), rng.uniform(150, 220)
    w, h = rng.uniform(40, 160), rng.uniform(25, 70)
    return dict(name="DontCare", truncated=-1.0, occluded=-1, alpha=-10.0, bbox=np.round(np.array([u, v, u + w, v + h]) * 4) / 4,
                dimensions=np.array([-1.0, -1.0, -1.0]), location=np.array([-1000.0, -1000.0, -1000.0]), rotation_y=-10.0)


def _jittered(rng, g):
    name = g["name"] if rng.rand() > 0.1 else CLASSES[rng.choice(len(CLASSES))]
    dims = np.round(g["dimensions"] * (1 + 0.05 * rng.randn(3)), 2)
    loc = np.round(g["location"] + rng.randn(3) * [0.15, 0.05, 0.15], 2)
    ry = round(float(g["rotation_y"] + 0.08 * rng.randn()), 2)
    bbox = np.round((g["bbox"] + rng.randn(4) * 2.5) * 4) / 4
    return dict(name=name, truncated=0.0, occluded=0, alpha=round(float(g["alpha"] + 0.2 * rng.randn()), 2), bbox=bbox, dimensions=dims, location=loc,
                rotation_y=ry)


def _false_positive(rng, dontcares):
    d = _gt_object(rng)
    d.update(truncated=0.0, occluded=0)
    kind = rng.rand()
    if kind < 0.35 and dontcares:                         # sits on a DontCare region
        dc = dontcares[rng.randint(len(dontcares))]["bbox"]
        w, h = (dc[2] - dc[0]) * rng.uniform(0.4, 0.8), max(42.0, (dc[3] - dc[1]) * rng.uniform(0.5, 0.9))
        u, v = rng.uniform(dc[0], dc[2] - w), dc[1] + rng.uniform(-4, 4)
        d["bbox"] = np.round(np.array([u, v, u + w, v + h]) * 4) / 4
    elif kind < 0.55:                                      # low height
        b = d["bbox"]
        d["bbox"] = np.round(np.array([b[0], b[1], b[2], b[1] + rng.uniform(12, 24)]) * 4) / 4
    return d


def _pair_ok(d, others, dontcares):
    """The margin condition for detection d against the ground truths `others` and the DontCare boxes of its frame."""
    def clear(value, bound):
        return all(abs(value - mo) >= max(K.FIXTURE_MARGIN, 4 * bound) for mo in MIN_OVERLAPS_IN_USE)
    for g in others:
        v = K.image_box_overlap(d["bbox"][None], g["bbox"][None])[0, 0]
        if v > 0 and not clear(v, K.image_overlap_bound(d["bbox"], g["bbox"])):
            return False
        db, gb = K.metric_boxes(_as_anno([d]), 2)[0], K.metric_boxes(_as_anno([g]), 2)[0]
        v = K.bev_box_overlap(db[None, [0, 2, 3, 5, 6]], gb[None, [0, 2, 3, 5, 6]])[0, 0]
        if v > 0 and not clear(v, K.rotated_overlap_bound(gb[[0, 2, 3, 5, 6]], db[[0, 2, 3, 5, 6]])):
            return False
        v = K.d3_box_overlap(db[None], gb[None])[0, 0]
        if v > 0 and not clear(v, K.d3_overlap_bound(db, gb)):
            return False
    for c in dontcares:
        v = K.image_box_overlap(d["bbox"][None], c["bbox"][None], 0)[0, 0]
        if v > 0 and not clear(v, K.image_overlap_bound(d["bbox"], c["bbox"])):
            return False
    return True


def _as_anno(objs, with_score=False):
    keys = KEYS if with_score else KEYS[:-1]
    if not objs:
        return {k: (np.zeros((0, 4)) if k == "bbox" else np.zeros((0, 3)) if k in ("dimensions", "location") else
                    np.zeros(0, dtype="<U14") if k == "name" else np.zeros(0)) for k in keys}
    out = {}
    for k in keys:
        vals = [o[k] for o in objs]
        out[k] = np.array(vals) if k == "name" else np.array(vals, dtype=np.float64)
    return out


def make_inputs():
    """-> gt_annos, dt_annos, dt_annos_no_alpha (lists of NUM_FRAMES annotation dicts of numpy arrays)."""
    rng = np.random.RandomState(SEED)
    gt_annos, dt_annos = [], []
    for f in range(NUM_FRAMES):
        if f == 0:
            n_gt, n_dc, n_match, n_fp = 0, 0, 0, 0
        elif f == 1:
            n_gt, n_dc, n_match, n_fp = 6, 1, 0, 0
        elif f == 2:
            n_gt, n_dc, n_match, n_fp = 0, 0, 0, 5
        elif f == 3:
            n_gt, n_dc, n_match, n_fp = 66, 4, 60, 90
        else:
            n_gt, n_dc = rng.randint(4, 13), rng.randint(0, 4)
            n_match, n_fp = n_gt, rng.randint(2, 8)
        real = [_gt_object(rng) for _ in range(n_gt)]
        dontcares = [_dontcare(rng) for _ in range(n_dc)]
        gts = real + dontcares
        order = rng.permutation(len(gts))
        gts = [gts[i] for i in order]
        dets = []
        sources = [real[i] for i in rng.permutation(len(real))[:n_match] if rng.rand() < 0.85 or f == 3]
        scores = (rng.permutation(2000)[:len(sources) + n_fp] + 1) / 2001.0              # distinct within the frame
        for i in range(len(sources) + n_fp):
            for attempt in range(200):
                d = _jittered(rng, sources[i]) if i < len(sources) else _false_positive(rng, dontcares)
                if _pair_ok(d, gts, dontcares):
                    break
            else:
                raise RuntimeError("could not place a detection clear of every min_overlap: change the seed or the jitter")
            d["score"] = float(scores[i])
            dets.append(d)
        dets = [dets[i] for i in rng.permutation(len(dets))]
        gt_annos.append(_as_anno(gts))
        dt_annos.append(_as_anno(dets, with_score=True))
    no_alpha = [dict(a, alpha=np.full_like(a["alpha"], -10.0)) for a in dt_annos]
    return gt_annos, dt_annos, no_alpha


def check_conditions(gt_annos, dt_annos):
    """Both conditions of the module header, from the annotations alone.  Returns (smallest margin seen, largest pair bound seen)."""
    worst_margin, worst_bound = np.inf, 0.0
    for g, d in zip(gt_annos, dt_annos):
        assert len(np.unique(d["score"])) == len(d["score"]), "scores of a frame tie"
        n_d, n_g = len(d["name"]), len(g["name"])
        if n_d == 0:
            continue
        dc = np.asarray(g["bbox"]).reshape(-1, 4)[np.asarray(g["name"]) == "DontCare"] if n_g else np.zeros((0, 4))
        tables = []
        if n_g:
            d3, g3 = K.metric_boxes(d, 2), K.metric_boxes(g, 2)
            d1, g1 = d3[:, [0, 2, 3, 5, 6]], g3[:, [0, 2, 3, 5, 6]]
            tables.append((K.image_box_overlap(d["bbox"], g["bbox"]), lambda i, j: K.image_overlap_bound(d["bbox"][i], g["bbox"][j])))
            tables.append((K.bev_box_overlap(d1, g1), lambda i, j: K.rotated_overlap_bound(g1[j], d1[i])))
            tables.append((K.d3_box_overlap(d3, g3), lambda i, j: K.d3_overlap_bound(d3[i], g3[j])))
        if len(dc):
            tables.append((K.image_box_overlap(d["bbox"], dc, 0), lambda i, j: K.image_overlap_bound(d["bbox"][i], dc[j])))
        for ov, bound in tables:
            for i, j in zip(*np.nonzero(ov > 0)):
                b = bound(i, j)
                m = min(abs(ov[i, j] - mo) for mo in MIN_OVERLAPS_IN_USE)
                assert m >= max(K.FIXTURE_MARGIN, 4 * b), (ov[i, j], m, b)
                worst_margin, worst_bound = min(worst_margin, m), max(worst_bound, b)
    return worst_margin, worst_bound


def pack(annos, prefix):
    """Annotation list -> flat arrays for an .npz (per-frame counts + concatenations)."""
    out = {prefix + "_count": np.array([len(a["name"]) for a in annos], dtype=np.int64)}
    for k in KEYS:
        if k in annos[0]:
            parts = [np.asarray(a[k]) for a in annos]
            out[prefix + "_" + k] = np.concatenate([p.astype("<U14") for p in parts]) if k == "name" else np.concatenate(parts, 0)
    return out


def unpack(z, prefix):
    counts = z[prefix + "_count"]
    offs = np.concatenate([[0], np.cumsum(counts)])
    keys = [k for k in KEYS if prefix + "_" + k in z]
    return [{k: z[prefix + "_" + k][offs[f]:offs[f + 1]] for k in keys} for f in range(len(counts))]
