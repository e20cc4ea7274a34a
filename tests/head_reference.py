"""References for the dense-head kernels of csrc/head.hip (anchor decode, axis-aligned target assignment, centre targets, focal and smooth-L1
losses), the edge-case inputs that test_head_edges.py runs them on, and the measured constants of their float bounds.  Imports nothing from
seevcn_amd.

Two kinds of reference:
  * DISCRETE results (label, matched box, direction bin, period count, integer radius, cell, slot, mask) follow the fp32 SPEC: the reference's
    formulas in float32, in the operation order of its torch code, every operation correctly rounded (numpy float32; the library is built with
    correctly rounded divide / square root and without contraction, so it owes these bits).  float64 is asked to agree only on the dyadic
    families, where every intermediate is exact in both formats.
  * FLOAT results are held to float64 within K * eps32 * scale.  `scale` is written down per output below; K is 4 x K_REF, and K_REF is the
    worst error / (eps32 * scale) of the reference's own fp32 arithmetic on the CPU on the same inputs (test_head_reference.py asserts that every
    K_REF below is what was measured: the worst lies in [0.5 K_REF, K_REF]).  The factor 4 is for the device's expf / logf / log1pf / sinf / cosf /
    atan2f / powf, specified to a few ulp where the CPU's are within one."""
import functools

import numpy as np
import torch

import multihead_reference as MR
from oracle import heads as oh

F = np.float32
EPS32 = float(np.finfo(F).eps)
PI32 = F(np.pi)

# measured on the CPU (numpy float32 / torch-CPU float32 against float64), worst error / (eps32 * scale) per family, rounded up by less than a tenth
# (torch's vectorised exp / log1p differ in the last bit between CPU generations).  Measured: encode 0.692, decode 1.907, centre boxes 1.541,
# focal 0.347 / 0.418, smooth-L1 0.406 / 0.321.  A self-test that misses the UPPER edge of [0.5 K_REF, K_REF] on a new host with unchanged code
# means: measure again there, not a regression.  See the functions named
K_REF = {
    "encode": 0.75,           # encode_scale:        oracle encode (plain, sin/cos, extras) on every positive of the assignment cases
    "decode": 2.00,           # decode_f64:          decode_spec on decode_cases()
    "center_boxes": 1.60,     # center_box_scale:    oracle.heads.center_assign_single_head on center_cases()
    "focal": 0.38,            # focal_f64:           torch-CPU float32 chain on focal_cases()
    "focal_grad": 0.45,
    "smooth_l1": 0.44,        # smooth_l1_f64:       torch-CPU float32 chain on smooth_l1_cases()
    "smooth_l1_grad": 0.35,
}
K_KERNEL = {k: 4.0 * v for k, v in K_REF.items()}
UNDECIDED_CAP = 0.01          # random (non-dyadic) assignment family: share of anchors the float64 margin may leave undecided


def up(x, n=1):
    """the fp32 value n ulps above x (below for n < 0)"""
    x = F(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf))
    return x


# ============================================================================================ target assignment
def anchor_sets(A, per_loc, offs, set_major):
    """the set of every anchor, as k_assign finds it: the prefix `offs` over the slot of a location, or over the anchor index (set_major)"""
    key = np.arange(A) if set_major else np.arange(A) % per_loc
    return np.searchsorted(np.asarray(offs)[1:-1], key, side="right")


def _bev(b, dtype):
    """nearest_bev with the heading decision of the fp32 oracle (the spec of the switch) and the corners in `dtype`"""
    rot = np.abs(oh.limit_period(b[:, 6].astype(F), 0.5, np.pi))
    keep = (rot < PI32 / F(4))[:, None]
    d = b.astype(dtype)
    dims = np.where(keep, d[:, [3, 4]], d[:, [4, 3]])
    return np.concatenate([d[:, 0:2] - dims / 2, d[:, 0:2] + dims / 2], axis=1)


def _iou(a, b, dtype):
    xl = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    yl = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = xl * yl
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return (inter / np.clip(aa[:, None] + ab[None, :] - inter, dtype(F(1e-6)), None)).astype(dtype)


def assign_spec(anchors, sets, set_class, mthr, uthr, gt, dtype=F):
    """AxisAlignedTargetAssigner (axis_aligned_target_assigner.py:36-210, deterministic branch) with the IoU evaluated in `dtype`; thresholds are
    fp32 values (torch compares an fp32 tensor with a Python scalar in fp32).  anchors (A, 7 + E), sets (A,) the set of each anchor,
    gt (B, G, 8 + E) -> labels (B, A) int32, arg (B, A) the matched ground-truth row or -1, weights (B, A) fp32"""
    B, A = gt.shape[0], len(anchors)
    labels, arg_out = np.zeros((B, A), np.int32), np.full((B, A), -1, np.int64)
    ab = _bev(anchors, dtype)
    for b in range(B):
        cls_of = gt[b, :, -1].astype(int)
        gb = _bev(gt[b, :, :7], dtype) if gt.shape[1] else np.zeros((0, 4), dtype)
        for s, cls in enumerate(set_class):
            idx = np.nonzero(sets == s)[0]
            rows = np.nonzero(cls_of == cls)[0]
            if len(rows) == 0 or len(idx) == 0:
                continue
            ov = _iou(ab[idx], gb[rows], dtype)
            arg = ov.argmax(1)                                                   # first maximum
            mx = ov[np.arange(len(idx)), arg]
            gmax = ov.max(0)
            gmax[gmax == 0] = -1
            force = (ov == gmax[None]).any(1)
            lab = np.full(len(idx), -1, np.int32)
            lab[mx >= dtype(F(mthr[s]))] = cls
            lab[mx < dtype(F(uthr[s]))] = 0
            lab[force] = cls
            labels[b, idx] = lab
            arg_out[b, idx] = np.where(lab > 0, rows[arg], -1)
    return labels, arg_out, (labels > 0).astype(F)


def encode_targets(anchors, gt, arg, sincos, dtype=F):
    """the regression targets of the matched boxes `arg` (zeros elsewhere): ResidualCoder.encode_torch in fp32 (the oracle's) or in float64"""
    B, A = arg.shape
    E = anchors.shape[1] - 7
    out = np.zeros((B, A, 7 + sincos + E), dtype)
    for b in range(B):
        pos = np.nonzero(arg[b] >= 0)[0]
        if len(pos) == 0:
            continue
        g, a = gt[b, arg[b, pos], :-1].astype(dtype), anchors[pos].astype(dtype)
        if dtype is F:
            out[b, pos] = MR.encode(g, a, sincos)
            continue
        ad, gd = np.clip(a[:, 3:6], float(F(1e-5)), None), np.clip(g[:, 3:6], float(F(1e-5)), None)
        diag = np.sqrt(ad[:, 0] ** 2 + ad[:, 1] ** 2)
        ang = [np.cos(g[:, 6]) - np.cos(a[:, 6]), np.sin(g[:, 6]) - np.sin(a[:, 6])] if sincos else [g[:, 6] - a[:, 6]]
        out[b, pos] = np.concatenate([np.stack([(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / ad[:, 2],
                                                np.log(gd[:, 0] / ad[:, 0]), np.log(gd[:, 1] / ad[:, 1]), np.log(gd[:, 2] / ad[:, 2])] + ang, 1),
                                      g[:, 7:] - a[:, 7:]], axis=1)
    return out


def encode_scale(t64, anchors, gt, arg, sincos):
    """float64 magnitude of the target plus its inputs' rounding.  Centres and heading: |t| (a difference, one or two quotients).  Log sizes:
    |t| + 1, the quotient inside the logarithm is rounded to eps/2 of itself, which the logarithm turns into an absolute eps/2.  sin/cos code:
    |cos g| + |cos a| (|sin g| + |sin a|), each term rounded before the difference.  Extras: |t|."""
    s = np.abs(t64).copy()
    s[..., 3:6] += (arg >= 0)[..., None]
    if sincos:
        for b in range(arg.shape[0]):
            pos = np.nonzero(arg[b] >= 0)[0]
            rg, ra = gt[b, arg[b, pos], 6].astype(np.float64), anchors[pos, 6].astype(np.float64)
            s[b, pos, 6] = np.abs(np.cos(rg)) + np.abs(np.cos(ra))
            s[b, pos, 7] = np.abs(np.sin(rg)) + np.abs(np.sin(ra))
    return s


class AssignCase:
    """one call of sv_assign_targets_axis_aligned(_coded): anchors (A, 7 + E) in call order, per_loc / offs / set_major as the entry takes them"""

    def __init__(self, name, anchors, per_loc, offs, set_class, mthr, uthr, gt, sincos=0, set_major=0, coded=False, dyadic=True, f64_agrees=True,
                 expect=None):
        self.name, self.anchors, self.per_loc, self.offs = name, np.ascontiguousarray(anchors, F), int(per_loc), np.asarray(offs, np.int32)
        self.set_class, self.mthr, self.uthr = np.asarray(set_class, np.int32), np.asarray(mthr, F), np.asarray(uthr, F)
        self.gt, self.sincos, self.set_major, self.coded = np.ascontiguousarray(gt, F), sincos, set_major, bool(coded or sincos or set_major)
        self.dyadic, self.f64_agrees, self.expect = dyadic, f64_agrees, expect or {}
        self.E = self.anchors.shape[1] - 7
        self.coded = self.coded or self.E > 0
        self.sets = anchor_sets(len(self.anchors), self.per_loc, self.offs, set_major)

    @functools.cached_property
    def spec(self):
        """labels, arg, weights of the fp32 spec, fp32 targets, float64 targets and their scale"""
        lab, arg, w = assign_spec(self.anchors, self.sets, self.set_class, self.mthr, self.uthr, self.gt, F)
        t32 = encode_targets(self.anchors, self.gt, arg, self.sincos, F)
        t64 = encode_targets(self.anchors, self.gt, arg, self.sincos, np.float64)
        return dict(labels=lab, arg=arg, weights=w, t32=t32, t64=t64, scale=encode_scale(t64, self.anchors, self.gt, arg, self.sincos))

    @functools.cached_property
    def spec64(self):
        return assign_spec(self.anchors, self.sets, self.set_class, self.mthr, self.uthr, self.gt, np.float64)

    def check(self, labels, targets, weights, k):
        """(failure messages, worst target error / (eps32 * scale)) of one result against the spec"""
        s, fails = self.spec, []
        if not np.array_equal(labels, s["labels"]):
            bad = np.argwhere(labels != s["labels"])
            b, a = bad[0]
            fails.append("%s: %d labels differ from the fp32 spec, first (scene %d, anchor %d): got %d, want %d" %
                         (self.name, len(bad), b, a, labels[b, a], s["labels"][b, a]))
        if not np.array_equal(weights, s["weights"]):
            fails.append("%s: reg_weights differ from the fp32 spec" % self.name)
        err = np.abs(targets.astype(np.float64) - s["t64"])
        ratio = np.where(s["scale"] > 0, err / (EPS32 * np.maximum(s["scale"], 1e-300)), np.where(err > 0, np.inf, 0.0))
        worst = float(ratio.max()) if ratio.size else 0.0
        if not worst <= k:
            b, a, c = np.unravel_index(ratio.argmax(), ratio.shape)
            fails.append("%s: target[%d, %d, %d] = %r, float64 %r: error / (eps32 scale) = %.3g > %.3g" %
                         (self.name, b, a, c, targets[b, a, c], s["t64"][b, a, c], worst, k))
        for (b, a), (lab, row) in self.expect.items():                       # hand-derived expectations of the dyadic members
            if s["labels"][b, a] != lab or (row is not None and s["arg"][b, a] != row):
                fails.append("%s: the spec itself misses the hand-derived label / box at (%d, %d)" % (self.name, b, a))
        return fails, worst


def _box(x, y, dx, dy, rot=0.0, z=0.0, dz=2.0):
    return [x, y, z, dx, dy, dz, rot]


# Thresholds of the hand-built dyadic scene, one anchor set (= class) per pair.  0.6 / 0.45 and 0.35 are the configs' own; fp32 rules there:
# IoU 3/5 rounds to float32(0.6) = 0.60000002..., which float64 puts ABOVE 3/5 (float64 would call the anchor unmatched), and float32(0.45),
# float32(0.35) likewise sit on the rounded 9/20 and 7/20.
DYADIC_THRESHOLDS = [(F(0.5), F(0.25)), (up(0.5), up(0.25)), (up(0.5, -1), up(0.25, -1)), (F(0.6), F(0.45)), (F(0.5), F(0.35)), (F(0.5), F(0.25))]


def dyadic_scene(coded=False, E=0, sincos=0, G=None):
    """The hand-built members of the dyadic family in one call: centres and sizes multiples of 1/8 within +-64, so corners, intersections, areas
    and unions are exact in fp32 and float64 and the IoU is the correctly rounded quotient in both.  Every member sits alone in its own 16 m cell
    (IoU 0 with every other member).  A member's ground-truth box has an `owner` anchor equal to it (IoU 1) unless the member is about the
    forced match, so that a probe anchor below `matched` is not the box's best anchor.  Set s (class s + 1) has DYADIC_THRESHOLDS[s]; class 7 has
    no set.  Plain layout: slot s of a location is set s (sets padded to one length with far-away 1 x 1 anchors); coded: set-major runs of unequal
    length."""
    S = len(DYADIC_THRESHOLDS)
    per_set = [[] for _ in range(S)]
    gts, expect_by_key, cell = [], [], [0]

    def origin():
        c = cell[0]
        cell[0] += 1
        return -56.0 + 16.0 * (c % 8), -56.0 + 16.0 * (c // 8)

    def anchor(s, box, lab, row=None):
        per_set[s].append(box)
        expect_by_key.append((s, len(per_set[s]) - 1, lab, row))

    def truth(box, cls):
        gts.append(box + [cls])
        return len(gts) - 1

    for s in range(3):                                                          # IoU exactly 1/2 and 1/4 against 0.5 / 0.25 and both moved one ulp
        x, y = origin()
        g = truth(_box(x, y, 4, 4), s + 1)
        anchor(s, _box(x, y, 4, 4), s + 1, g)                                   # owner
        anchor(s, _box(x, y + 1, 4, 2), (s + 1) if s != 1 else -1, g if s != 1 else None)      # 8 / 16 = matched: positive; one ulp below the raised one
        x, y = origin()
        g = truth(_box(x, y, 8, 4), s + 1)
        anchor(s, _box(x, y, 8, 4), s + 1, g)
        anchor(s, _box(x - 2, y + 1, 4, 2), 0 if s == 1 else -1)                # 8 / 32 = unmatched: not below it, so -1; below the raised one: 0
    x, y = origin()                                                             # 3/5 against 0.6, 9/20 against 0.45 (set 3), 7/20 against 0.35 (set 4)
    g = truth(_box(x, y, 5, 2), 4)
    anchor(3, _box(x, y, 5, 2), 4, g)
    anchor(3, _box(x + 1, y, 3, 2), 4, g)
    x, y = origin()
    g = truth(_box(x, y, 10, 2), 4)
    anchor(3, _box(x, y, 10, 2), 4, g)
    anchor(3, _box(x + 0.5, y + 0.5, 9, 1), -1)
    x, y = origin()
    g = truth(_box(x, y, 10, 2), 5)
    anchor(4, _box(x, y, 10, 2), 5, g)
    anchor(4, _box(x - 1.5, y - 0.5, 7, 1), -1)
    # ties: two and three boxes of one class with IoU 6 / 10 to one anchor; the first row wins and the target is that box's (z differs)
    x, y = origin()
    g0 = truth(_box(x + 1, y, 4, 2, z=1.0), 1)
    truth(_box(x - 1, y, 4, 2, z=-1.0), 1)
    anchor(0, _box(x, y, 4, 2), 1, g0)
    x, y = origin()
    g0 = truth(_box(x - 1, y, 4, 2, z=-2.0), 6)
    truth(_box(x + 1, y, 4, 2, z=2.0), 6)
    truth(_box(x, y + 0.5, 4, 2, z=3.0), 6)
    anchor(5, _box(x, y, 4, 2), 6, g0)
    # forced match: a 1 x 1 box inside two 4 x 4 anchors (IoU 1/16 < unmatched, both tied at the box's maximum: both positive); a third anchor
    # that overlaps it by less stays background
    x, y = origin()
    g = truth(_box(x, y, 1, 1), 1)
    anchor(0, _box(x + 1, y, 4, 4), 1, g)
    anchor(0, _box(x - 1, y + 1, 4, 4), 1, g)
    anchor(0, _box(x + 2.25, y, 4, 4), 0)                                      # covers a quarter of the box: 0.25 / 16.75
    # a box that touches anchors along an edge only: IoU 0 everywhere, gt_max 0 -> -1, nothing forced; and a zero-area box on an anchor
    x, y = origin()
    truth(_box(x, y, 2, 2), 1)
    anchor(0, _box(x + 2, y, 2, 2), 0)
    anchor(0, _box(x, y - 3, 2, 4), 0)
    x, y = origin()
    truth(_box(x, y, 0, 3), 1)
    anchor(0, _box(x, y, 4, 4), 0)
    # a class without a set on top of an anchor; a class-0 row in the middle of the list; duplicated boxes
    x, y = origin()
    truth(_box(x, y, 4, 2), 7)
    anchor(0, _box(x, y, 4, 2), 0)
    x, y = origin()
    truth(_box(x, y, 4, 2), 0)
    anchor(1, _box(x, y, 4, 2), 0)
    x, y = origin()
    g = truth(_box(x, y, 4, 2, z=0.5), 2)
    truth(_box(x, y, 4, 2, z=0.5), 2)
    anchor(1, _box(x, y, 4, 2), 2, g)
    anchor(1, _box(x + 1, y, 4, 2), 2, g)                                      # 6 / 10 >= matched + 1 ulp
    # nearest_bev headings: a 4 x 2 box at heading h under a 4 x 2 anchor at heading 0: IoU 1 while the switch keeps the sizes, 1/3 (between the
    # thresholds: -1) once it swaps them; the owner anchor carries the box's own heading.  Spec of the switch: oracle.heads.nearest_bev (fp32)
    q = F(np.pi / 4)
    for h in [0.0, q, up(q), up(q, -1), F(np.pi / 2), PI32, -PI32, F(3 * np.pi / 4), F(7.5 * np.pi), F(1e4), -q, up(-q, -1), F(np.pi) - q, F(5 * np.pi / 4)]:
        x, y = origin()
        g = truth(_box(x, y, 4, 2, rot=float(h)), 1)
        anchor(0, _box(x, y, 4, 2, rot=float(h)), 1, g)                         # owner: the box's own heading, so the same switch and IoU 1
        swapped = not bool(np.abs(oh.limit_period(F(h), 0.5, np.pi)) < PI32 / F(4))
        anchor(0, _box(x, y, 4, 2), -1 if swapped else 1, None if swapped else g)
        anchor(0, _box(x, y, 2, 4, rot=float(np.pi / 2)), -1 if swapped else 1, None if swapped else g)   # the anchors' own switch: pi/2 swaps 2 x 4 to 4 x 2
    assert cell[0] <= 64
    n_real = len(gts)
    G = G or n_real + 3                                                         # trailing padding rows
    assert G >= n_real
    gt = np.zeros((2, G, 8 + E), F)                                             # scene 0 full, scene 1 empty
    g7 = np.array(gts, F)
    gt[0, :n_real, :7], gt[0, :n_real, -1] = g7[:, :7], g7[:, 7]
    if E:
        gt[0, :n_real, 7:7 + E] = (np.arange(n_real * E).reshape(n_real, E) % 7 - 3) * 0.25
    set_class = np.arange(1, S + 1)
    mthr, uthr = [t[0] for t in DYADIC_THRESHOLDS], [t[1] for t in DYADIC_THRESHOLDS]
    pad = _box(60.0, 60.0, 1, 1)
    if coded:
        runs = [np.array(p, F).reshape(-1, 7) for p in per_set]
        anchors = np.concatenate(runs)
        offs = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
        at = {(s, i): offs[s] + i for s in range(S) for i in range(len(per_set[s]))}
        per_loc, set_major = 1, 1
    else:
        n = max(len(p) for p in per_set)
        anchors = np.array([[p[i] if i < len(p) else pad for p in per_set] for i in range(n)], F).reshape(-1, 7)
        offs = np.arange(S + 1)
        at = {(s, i): i * S + s for s in range(S) for i in range(len(per_set[s]))}
        per_loc, set_major = S, 0
    if E:
        anchors = np.concatenate([anchors, ((np.arange(len(anchors) * E).reshape(-1, E) % 5) - 2) * F(0.5)], axis=1)
    expect = {(0, at[(s, i)]): (lab, row) for s, i, lab, row in expect_by_key}
    # float64 disagrees by construction on the three members whose IoU rounds onto a non-dyadic threshold (3/5, 9/20, 7/20): fp32 rules
    return AssignCase("dyadic scene%s" % (" coded E=%d sincos=%d" % (E, sincos) if coded else ""), anchors, per_loc, offs, set_class, mthr, uthr, gt,
                      sincos=sincos, set_major=set_major, coded=coded, f64_agrees=False, expect=expect)


def dyadic_f64_exceptions(case):
    """anchors of the dyadic scene on which float64 is not asked to agree: the probes at IoU 3/5, 9/20 and 7/20 (sets 3 and 4)"""
    return np.isin(case.sets, [3, 4])[None, :] & np.ones((case.gt.shape[0], 1), bool)


def dyadic_random(name, A, B, G, seed, coded=False, E=0, sincos=0):
    """Random member of the dyadic family at a given shape: anchors 4 x 2 / 2 x 4 / 1 x 1 and boxes with sizes in halves up to 6, centres multiples of
    1/8 in a 12 m window (so that boxes and anchors meet often).  Areas are multiples of 1/64 below 64: two different IoU values differ by more
    than 2^-24 and cannot round to one fp32 number, so ties, maxima and threshold decisions are the same in fp32 and float64 (thresholds 1/2 and
    1/4, 5/8 and 3/8)."""
    rng = np.random.default_rng(seed)
    S = 2 if not coded else 3
    sizes = np.array([[4, 2], [2, 4], [1, 1], [2, 2]], F)
    anchors = np.zeros((A, 7 + E), F)
    anchors[:, 0:2] = rng.integers(-48, 49, (A, 2)) / 8.0
    anchors[:, 3:5] = sizes[rng.integers(0, 4, A)]
    anchors[:, 2], anchors[:, 5] = rng.integers(-8, 9, A) / 8.0, 1.5
    anchors[:, 6] = rng.choice([0.0, float(F(np.pi / 2))], A)
    gt = np.zeros((B, G, 8 + E), F)
    if G:
        gt[..., 0:2] = rng.integers(-48, 49, (B, G, 2)) / 8.0
        gt[..., 3:5] = rng.integers(1, 13, (B, G, 2)) / 2.0
        gt[..., 2], gt[..., 5] = rng.integers(-8, 9, (B, G)) / 8.0, rng.integers(1, 5, (B, G)) / 2.0
        gt[..., 6] = rng.choice([0.0, 0.5, float(F(np.pi / 2)), -2.0], (B, G))
        gt[..., -1] = rng.integers(0, S + 2, (B, G))                           # class 0 rows and a class without a set among them
        gt[:, G // 2:, :] = np.where(rng.random((B, 1, 1)) < 0.3, 0, gt[:, G // 2:, :])      # some scenes end in padding
        if G > 3:
            gt[:, 1] = gt[:, 0]                                                 # duplicated box
    if E:
        anchors[:, 7:] = rng.integers(-4, 5, (A, E)) / 4.0
        gt[..., 7:7 + E] = rng.integers(-8, 9, (B, G, E)) / 4.0
    if coded:                                                                   # set-major runs of unequal length
        cuts = sorted({0, A} | {min(A, max(0, int(A * f))) for f in (0.2, 0.7)})
        while len(cuts) < S + 1:
            cuts.append(A)
        offs, per_loc, set_major = np.array(sorted(cuts)[:S] + [A]), 1, 1
    else:
        per_loc = S + 1 if A >= S + 1 else 1                                    # set 1 owns two slots of a location
        offs, set_major = (np.array([0, 1, 3]) if per_loc > 1 else np.array([0, 1, 1])), 0
    set_class = np.arange(1, S + 1)
    mthr, uthr = ([0.5, 0.625, 0.5][:S], [0.25, 0.375, 0.25][:S])
    return AssignCase(name, anchors, per_loc, offs, set_class, mthr, uthr, gt, sincos=sincos, set_major=set_major, coded=coded)


@functools.lru_cache(maxsize=None)
def assign_cases():
    """every dyadic call: the hand-built scene in both layouts and the shapes A x B x G of the plain and the coded entry"""
    cases = [dyadic_scene(), dyadic_scene(coded=True, E=2, sincos=1), dyadic_scene(coded=True, E=0, sincos=0)]
    seed = 100
    for A in (1, 255, 257):
        for B in (1, 3):
            for G in (0, 1, 127, 128):
                if (A, B, G) in ((1, 3, 127), (255, 1, 127), (1, 1, 128), (255, 3, 1)):
                    continue                                                    # each A, B and G is met several times without these
                seed += 1
                cases.append(dyadic_random("plain A=%d B=%d G=%d" % (A, B, G), A, B, G, seed))
    cases.append(dyadic_random("plain A=131329 B=1 G=10", 131072 + 257, 1, 10, 200))       # one block cap of 512 x 256 anchors and a remainder
    for i, (A, B, G, E, sc) in enumerate([(257, 1, 255, 0, 1), (255, 3, 256, 2, 0), (257, 3, 256, 2, 1), (1, 1, 255, 2, 1), (600, 1, 0, 2, 1)]):
        cases.append(dyadic_random("coded A=%d B=%d G=%d E=%d sincos=%d" % (A, B, G, E, sc), A, B, G, 300 + i, coded=True, E=E, sincos=sc))
    return cases


def random_assign_case(A=3000, G=40, seed=7):
    """the non-dyadic family: KITTI-like anchors and boxes at arbitrary fp32 positions, sizes and headings"""
    rng = np.random.default_rng(seed)
    sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], F)
    per_loc, offs = 6, np.array([0, 2, 4, 6])
    loc = rng.uniform(-20, 20, (A // per_loc, 2)).astype(F)
    anchors = np.zeros((A // per_loc, per_loc, 7), F)
    anchors[:, :, 0:2] = loc[:, None]
    anchors[:, :, 3:6] = sizes[np.arange(per_loc) // 2][None]
    anchors[:, :, 2] = -1.0
    anchors[:, :, 6] = np.where(np.arange(per_loc) % 2 == 1, F(np.pi / 2), F(0))[None]
    anchors = anchors.reshape(-1, 7)
    gt = np.zeros((2, G, 8), F)
    cls = rng.integers(1, 4, (2, G))
    pick = rng.integers(0, len(loc), (2, G))
    gt[..., 0:2] = loc[pick] + rng.normal(0, 0.4, (2, G, 2))                   # near anchors, so that every kind of label occurs
    gt[..., 2] = rng.normal(-1, 0.3, (2, G))
    gt[..., 3:6] = sizes[cls - 1] * rng.uniform(0.8, 1.25, (2, G, 3))
    gt[..., 6] = rng.uniform(-np.pi, np.pi, (2, G))
    gt[..., 7] = cls
    gt[1, G - 5:] = 0
    return AssignCase("random", anchors, per_loc, offs, [1, 2, 3], [0.6, 0.5, 0.5], [0.45, 0.35, 0.35], gt, dyadic=False, f64_agrees=False)


def decided_by_margin(case, rel=8.0):
    """(B, A) bool: anchors whose float64 IoU maximum lies farther than rel * eps32 * IoU from both thresholds and from the second-best IoU of the
    anchor, and which no ground-truth box's own maximum comes within that margin of -- there the float64 label is the label"""
    B, A = case.gt.shape[0], len(case.anchors)
    ok = np.ones((B, A), bool)
    ab = _bev(case.anchors, np.float64)
    for b in range(B):
        cls_of = case.gt[b, :, -1].astype(int)
        gb = _bev(case.gt[b, :, :7], np.float64)
        for s, cls in enumerate(case.set_class):
            idx, rows = np.nonzero(case.sets == s)[0], np.nonzero(cls_of == cls)[0]
            if len(rows) == 0 or len(idx) == 0:
                continue
            ov = _iou(ab[idx], gb[rows], np.float64)
            srt = np.sort(ov, axis=1)
            mx = srt[:, -1]
            second = srt[:, -2] if ov.shape[1] > 1 else np.full(len(idx), -1.0)
            m = rel * EPS32 * mx
            good = (np.abs(mx - float(case.mthr[s])) > m) & (np.abs(mx - float(case.uthr[s])) > m) & ((mx - second > m) | (mx == 0))
            gmax = ov.max(0)                                                    # forced match: an anchor near a box's maximum without being it
            near = (np.abs(ov - gmax[None]) <= rel * EPS32 * gmax[None]) & (ov < gmax[None])
            ok[b, idx] = good & ~near.any(1)
    return ok


# ============================================================================================ decode
def decode_spec(anchors, enc, dir_logits, num_bins, dir_offset, dir_limit_offset, sincos=0):
    """generate_predicted_boxes (anchor_head_template.py:225-272) in fp32 with the period float32(2 pi / num_bins), as the reference has it.
    Returns the boxes (B, A, 7 + E), the period count k of limit_period and the direction label (None without logits)."""
    boxes = MR.decode(enc, anchors[None], sincos)
    k = lab = None
    if dir_logits is not None:
        lab = np.argmax(dir_logits, axis=-1)                                    # first maximum
        period = F(2 * np.pi / num_bins)
        val = boxes[..., 6] - F(dir_offset)
        k = np.floor(val / period + F(dir_limit_offset))
        boxes[..., 6] = (val - k * period) + F(dir_offset) + period * lab.astype(F)
    return boxes, k, lab


def decode_f64(anchors, enc, k, lab, num_bins, dir_offset, sincos=0):
    """float64 decode on the branch (k, lab) the fp32 spec chose, and the scale of every output: the sum of the absolute values of the terms it is
    built from.  Heading with the sin/cos code: atan2(y, x) moves by at most (|dy| + |dx|) / hypot(y, x) and y, x carry eps of |t7| + |sin ra| and
    |t6| + |cos ra|, so scale = |rg| + (|t7| + |sin ra| + |t6| + |cos ra|) / hypot; at y = x = 0 both sides give atan2(0, 0) = 0."""
    a, t = anchors[None].astype(np.float64), enc.astype(np.float64)
    E = anchors.shape[1] - 7
    diag = np.sqrt(a[..., 3] ** 2 + a[..., 4] ** 2)
    out = np.zeros(enc.shape[:2] + (7 + E,))
    sc = np.zeros_like(out)
    for c, (m, base) in enumerate([(diag, a[..., 0]), (diag, a[..., 1]), (a[..., 5], a[..., 2])]):
        out[..., c], sc[..., c] = t[..., c] * m + base, np.abs(t[..., c] * m) + np.abs(base)
    for c in (3, 4, 5):
        out[..., c] = np.exp(t[..., c]) * a[..., c]
        sc[..., c] = np.abs(out[..., c])
    if sincos:
        y, x = t[..., 7] + np.sin(a[..., 6]), t[..., 6] + np.cos(a[..., 6])
        rg = np.arctan2(y, x)
        h = np.hypot(y, x)
        srg = np.abs(rg) + np.where(h > 0, (np.abs(t[..., 7]) + np.abs(np.sin(a[..., 6])) + np.abs(t[..., 6]) + np.abs(np.cos(a[..., 6]))) / np.maximum(h, 1e-300), 0)
    else:
        rg = t[..., 6] + a[..., 6]
        srg = np.abs(t[..., 6]) + np.abs(a[..., 6])
    if k is not None:
        period = float(F(2 * np.pi / num_bins))                                 # the period is a constant of the computation, not a rounded result
        off = float(F(dir_offset))
        rg = (rg - off) - k * period + off + period * lab
        srg = srg + 2 * abs(off) + np.abs(k * period) + np.abs(period * lab)
    out[..., 6], sc[..., 6] = rg, srg
    out[..., 7:] = t[..., 7 + sincos:] + a[..., 7:]
    sc[..., 7:] = np.abs(t[..., 7 + sincos:]) + np.abs(a[..., 7:])
    return out, sc


class DecodeCase:
    def __init__(self, name, anchors, enc, dir_logits, num_bins, dir_offset, dir_limit_offset, sincos=0, coded=False):
        self.name, self.anchors, self.enc = name, np.ascontiguousarray(anchors, F), np.ascontiguousarray(enc, F)
        self.dir_logits = None if dir_logits is None else np.ascontiguousarray(dir_logits, F)
        self.num_bins, self.dir_offset, self.dir_limit_offset, self.sincos = num_bins, dir_offset, dir_limit_offset, sincos
        self.E = self.anchors.shape[1] - 7
        self.coded = bool(coded or sincos or self.E)

    @functools.cached_property
    def spec(self):
        boxes, k, lab = decode_spec(self.anchors, self.enc, self.dir_logits, self.num_bins, self.dir_offset, self.dir_limit_offset, self.sincos)
        out64, scale = decode_f64(self.anchors, self.enc, k, lab, self.num_bins, self.dir_offset, self.sincos)
        return dict(boxes=boxes, k=k, lab=lab, out64=out64, scale=scale)

    def ratio(self, got):
        s = self.spec
        err = np.abs(got.astype(np.float64) - s["out64"])
        return np.where(s["scale"] > 0, err / (EPS32 * np.maximum(s["scale"], 1e-300)), np.where(err > 0, np.inf, 0.0))

    def check(self, got, kbound):
        """failure messages and the worst ratio.  A heading whose error is a multiple of the period (a wrong period count or a wrong bin) is named"""
        r = self.ratio(got)
        worst = float(r.max()) if r.size else 0.0
        fails = []
        if not worst <= kbound:
            b, a, c = np.unravel_index(r.argmax(), r.shape)
            n = int((r[..., 6] > kbound).sum())
            fails.append("%s: out[%d, %d, %d] = %r, float64 on the spec's branch %r: error / (eps32 scale) = %.3g > %.3g (%d headings out in all)" %
                         (self.name, b, a, c, got[b, a, c], self.spec["out64"][b, a, c], worst, kbound, n))
        return fails, worst


def _rand_anchors(rng, A, E=0):
    a = np.zeros((A, 7 + E), F)
    a[:, 0:2] = rng.uniform(-70, 70, (A, 2))
    a[:, 2] = rng.uniform(-3, 1, A)
    a[:, 3:6] = rng.uniform(0.4, 5, (A, 3))
    a[:, 6] = rng.choice([0.0, float(F(np.pi / 2))], A)
    if E:
        a[:, 7:] = rng.normal(0, 2, (A, E))
    return a


def boundary_decode_case(num_bins, dir_limit_offset, dir_offset=0.78539, n_per=40):
    """headings for which (rg - dir_offset) / period + dir_limit_offset sits on an integer and up to 3 fp32 ulps either side: rg = t6 + ra with
    ra = 0, so t6 is the heading; for every integer m in -3 .. 3 the fp32 number nearest to dir_offset + (m - dir_limit_offset) * period and its 3
    neighbours on each side.  Logits make every bin the maximum in turn."""
    rng = np.random.default_rng(num_bins * 10 + int(dir_limit_offset * 2))
    period = 2 * np.pi / num_bins
    heads = []
    for m in range(-3, 4):
        c = F(dir_offset + (m - dir_limit_offset) * period)
        heads += [up(c, j) for j in range(-3, 4)]
        c2 = F(F(m - dir_limit_offset) * F(period)) + F(dir_offset)             # the fp32 product: val / period is then the integer itself
        heads += [up(c2, j) for j in range(-3, 4)]
    heads = np.array(heads, F)
    A = len(heads)
    anchors = _rand_anchors(rng, A)
    anchors[:, 6] = 0
    enc = (rng.normal(0, 0.3, (1, A, 7))).astype(F)
    enc[0, :, 6] = heads
    logits = rng.normal(0, 1, (1, A, num_bins)).astype(F)
    logits[0, np.arange(A), np.arange(A) % num_bins] = 3.0
    return DecodeCase("boundary bins=%d limit=%g" % (num_bins, dir_limit_offset), anchors, enc, logits, num_bins, dir_offset, dir_limit_offset)


@functools.lru_cache(maxsize=None)
def decode_cases():
    cases = []
    for nb in (1, 2, 3, 4, 9):
        for lim in (0.0, 0.5):
            cases.append(boundary_decode_case(nb, lim))
    rng = np.random.default_rng(11)
    for i, (B, A) in enumerate([(1, 1), (1, 255), (1, 257), (3, 85)]):         # B * A in {1, 255, 257, 255}
        nb = (2, 3, 4, 9)[i]
        anchors = _rand_anchors(rng, A)
        enc = rng.normal(0, 0.5, (B, A, 7)).astype(F)
        enc[..., 6] = rng.uniform(-7, 7, (B, A))
        logits = rng.normal(0, 1, (B, A, nb)).astype(F)
        logits[:, ::3, :] = 0.25                                                # tied logits: the first maximum wins
        if nb > 2:
            logits[:, 1::3, 1] = logits[:, 1::3, 2] = 5.0                       # tie between bins 1 and 2
        cases.append(DecodeCase("plain B=%d A=%d bins=%d" % (B, A, nb), anchors, enc, logits, nb, 0.78539, 0.0))
    anchors = _rand_anchors(rng, 257)
    cases.append(DecodeCase("plain without dir_logits", anchors, rng.normal(0, 0.5, (1, 257, 7)).astype(F), None, 0, 0.0, 0.0))
    # coded: sin/cos heading in every quadrant, on the axes and with both arguments zero (anchor heading 0: sin 0, cos 1 exactly); extras;
    # zero-size anchors (diag = 0); |t[3..5]| up to 10
    for E, sincos in ((0, 1), (2, 1), (2, 0), (0, 0)):
        A = 257
        anchors = _rand_anchors(rng, A, E)
        enc = rng.normal(0, 0.5, (2, A, 7 + sincos + E)).astype(F)
        enc[..., 3:6] = rng.uniform(-10, 10, (2, A, 3))
        anchors[5:9, 3:5] = 0                                                   # diag = 0
        anchors[9, 3:6] = 0
        if sincos:
            anchors[:16, 6] = 0
            quad = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1], [1, 0], [0, 1], [-1, 0], [0, -1], [0, 0]], F)      # (x, y) wanted
            enc[:, :9, 6], enc[:, :9, 7] = quad[:, 0] - 1, quad[:, 1]           # x = t6 + cos 0, y = t7 + sin 0
            enc[1, :9, 6:8] *= F(0.5)
            enc[1, :9, 6] -= F(0.5)
            enc[1, 6, 6] = -3.0                                                 # x = -2, y = +0: pi
        cases.append(DecodeCase("coded E=%d sincos=%d" % (E, sincos), anchors, enc, None, 0, 0.0, 0.0, sincos=sincos, coded=True))
    anchors = _rand_anchors(rng, 200, 2)
    enc = rng.normal(0, 0.5, (1, 200, 9)).astype(F)
    cases.append(DecodeCase("coded E=2 bins=2", anchors, enc, rng.normal(0, 1, (1, 200, 2)).astype(F), 2, 0.78539, 0.0, coded=True))
    return cases


def stride_decode_case():
    """one call of 524288 + 300 elements: past the grid cap of 2048 blocks x 256 threads"""
    rng = np.random.default_rng(12)
    A = 524288 + 300
    anchors = _rand_anchors(rng, 1024)
    anchors = np.tile(anchors, (A // 1024 + 1, 1))[:A]
    anchors[:, 0] += np.arange(A, dtype=F) * F(1e-4)
    enc = rng.normal(0, 0.5, (1, A, 7)).astype(F)
    enc[..., 6] = rng.uniform(-7, 7, (1, A))
    return DecodeCase("plain stride loop A=%d" % A, anchors, enc, rng.normal(0, 1, (1, A, 2)).astype(F), 2, 0.78539, 0.0)


# ============================================================================================ centre targets
def radius_chain(h, w, min_overlap):
    """gaussian_radius (centernet_utils.py:9-35) as the reference's torch code evaluates it on fp32 tensors: Python-scalar constants are rounded to
    fp32 before the operation they enter (1 - min_overlap, 1 + min_overlap, 4 * min_overlap, ... are computed in double first), every operation in
    fp32.  Here in numpy so that the square root is the correctly rounded one the library is built with: torch's vectorised CPU sqrt is not (see
    radius_chain_torch and test_head_reference.py)."""
    h, w, mo = np.asarray(h, F), np.asarray(w, F), float(min_overlap)
    b1 = h + w
    c1 = w * h * F(1 - mo) / F(1 + mo)
    r1 = (b1 + np.sqrt(b1 * b1 - F(4) * c1)) / F(2)
    b2 = F(2) * (h + w)
    c2 = F(1 - mo) * w * h
    r2 = (b2 + np.sqrt(b2 * b2 - F(16) * c2)) / F(2)
    b3 = F(-2 * mo) * (h + w)
    c3 = F(mo - 1) * w * h
    r3 = (b3 + np.sqrt(b3 * b3 - F(4 * (4 * mo)) * c3)) / F(2)
    return np.minimum(np.minimum(r1, r2), r3)


def radius_chain_torch(h, w, min_overlap, exact_sqrt=False):
    """the reference's lines themselves on torch-CPU fp32 tensors; exact_sqrt replaces .sqrt() by the correctly rounded square root"""
    height, width = torch.as_tensor(np.asarray(h, F)), torch.as_tensor(np.asarray(w, F))
    sqrt = (lambda x: x.double().sqrt().float()) if exact_sqrt else (lambda x: x.sqrt())
    a1 = 1
    b1 = (height + width)
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + sqrt(b1 ** 2 - 4 * a1 * c1)) / 2
    a2 = 4
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + sqrt(b2 ** 2 - 4 * a2 * c2)) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    return torch.min(torch.min(r1, r2), r3).numpy()


def _radius64(h, w, mo):
    b1, c1 = h + w, w * h * (1 - mo) / (1 + mo)
    r1 = (b1 + np.sqrt(b1 * b1 - 4 * c1)) / 2
    b2, c2 = 2 * (h + w), (1 - mo) * w * h
    r2 = (b2 + np.sqrt(b2 * b2 - 16 * c2)) / 2
    a3, b3, c3 = 4 * mo, -2 * mo * (h + w), (mo - 1) * w * h
    r3 = (b3 + np.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


@functools.lru_cache(maxsize=None)
def radius_family():
    """(h, w, min_overlap) fp32 arrays: for every integer R = 2 .. 12, overlap 0.1 / 0.5 / 0.7 and two widths, the height at which the float64 radius
    is R (bisection; the radius grows with the height) and its fp32 neighbours at -3 .. 3 ulps.  462 sizes."""
    hs, ws, mos = [], [], []
    for mo in (0.1, 0.5, 0.7):
        for R in range(2, 13):
            for w in (float(F(2.5 * R + 1.1)), float(F(4 * R + 0.37))):            # the radius stays below 2 (1 - overlap) w however tall the box
                lo, hi = 1e-3, 1e5
                assert _radius64(lo, w, mo) < R < _radius64(hi, w, mo)
                for _ in range(200):
                    mid = 0.5 * (lo + hi)
                    lo, hi = (mid, hi) if _radius64(mid, w, mo) < R else (lo, mid)
                for j in range(-3, 4):
                    hs.append(up(F(hi), j)), ws.append(F(w)), mos.append(mo)
    return np.array(hs, F), np.array(ws, F), np.array(mos)


def radius_spec_family():
    h, w, mo = radius_family()
    return np.concatenate([radius_chain(h[mo == m], w[mo == m], m) for m in (0.1, 0.5, 0.7)])


def center_oracle(gt, class_names, each_head, fm_size, stride, pc_range, voxel, num_max_objs, overlap, min_radius, radius_delta=0):
    """oracle.heads.center_assign_targets with the integer radius of radius_chain (the spec); radius_delta moves every box's integer radius (the
    self-test of the radius family: a radius one off must show in the heat map of every member)"""
    saved = oh.gaussian_radius
    oh.gaussian_radius = lambda h, w, mo: F(int(radius_chain(h, w, overlap)) + radius_delta)
    try:
        return oh.center_assign_targets(gt, class_names, each_head, fm_size, stride, pc_range, voxel, num_max_objs=num_max_objs,
                                        gaussian_overlap=overlap, min_radius=min_radius)
    finally:
        oh.gaussian_radius = saved


class CenterCase:
    """one CenterHead.assign_targets call on a W x H map (W != H, voxel_x != voxel_y)"""

    def __init__(self, name, gt, class_names, each_head, W=24, H=40, voxel=(0.25, 0.5, 0.2), pc_range=(-12.0, -40.0, -5.0, 12.0, 40.0, 3.0), stride=4,
                 num_max_objs=500, overlap=0.1, min_radius=2):
        self.name, self.gt, self.class_names, self.each_head = name, np.ascontiguousarray(gt, F), list(class_names), [list(h) for h in each_head]
        self.W, self.H, self.voxel, self.pc_range, self.stride = W, H, voxel, pc_range, stride
        self.num_max_objs, self.overlap, self.min_radius = num_max_objs, overlap, min_radius

    def swapped(self):
        """x and y exchanged: map, voxel, range and the boxes' centres and sizes"""
        g = self.gt.copy()
        g[..., [0, 1, 3, 4]] = self.gt[..., [1, 0, 4, 3]]
        r = self.pc_range
        return CenterCase(self.name + " (x/y swapped)", g, self.class_names, self.each_head, self.H, self.W, (self.voxel[1], self.voxel[0], self.voxel[2]),
                          (r[1], r[0], r[2], r[4], r[3], r[5]), self.stride, self.num_max_objs, self.overlap, self.min_radius)

    @functools.cached_property
    def spec(self):
        return center_oracle(self.gt, self.class_names, self.each_head, (self.W, self.H), self.stride, self.pc_range, self.voxel, self.num_max_objs,
                             self.overlap, self.min_radius)

    def spec_heat(self, radius_delta):
        """the oracle's heat maps with every integer radius moved by radius_delta"""
        return center_oracle(self.gt, self.class_names, self.each_head, (self.W, self.H), self.stride, self.pc_range, self.voxel, self.num_max_objs,
                             self.overlap, self.min_radius, radius_delta)["heatmaps"]

    @functools.cached_property
    def boxes64(self):
        """float64 regression targets of the slots the spec fills, and their scale (center_box_scale)"""
        out = []
        for h, names in enumerate(self.each_head):
            t64 = np.zeros(self.spec["target_boxes"][h].shape)
            sc = np.zeros_like(t64)
            ids = [self.class_names.index(n) + 1 for n in names]
            for b in range(self.gt.shape[0]):
                rows = [r for r in self.gt[b] if int(r[-1]) in ids][:self.num_max_objs]
                for k, r in enumerate(rows):
                    if not self.spec["masks"][h][b, k]:
                        continue
                    ind = int(self.spec["inds"][h][b, k])
                    t64[b, k], sc[b, k] = center_box_scale(r.astype(np.float64), self, (ind % self.W, ind // self.W))
            out.append((t64, sc))
        return out

    def check(self, got, kbound):
        """got: dict of per-head lists as CenterHead.assign_targets returns them (numpy).  -> (failures, worst box ratio, worst heat-map ulps)"""
        s, fails, worst, worst_ulp = self.spec, [], 0.0, 0.0
        for h in range(len(self.each_head)):
            if not np.array_equal(got["masks"][h], s["masks"][h]):
                fails.append("%s head %d: masks differ (%d slots)" % (self.name, h, int((got["masks"][h] != s["masks"][h]).sum())))
            if not np.array_equal(got["inds"][h], s["inds"][h]):
                bad = np.argwhere(got["inds"][h] != s["inds"][h])
                fails.append("%s head %d: inds differ in %d slots, first %s: got %d, want %d" %
                             (self.name, h, len(bad), tuple(bad[0]), got["inds"][h][tuple(bad[0])], s["inds"][h][tuple(bad[0])]))
            hm, ref = got["heatmaps"][h], s["heatmaps"][h]                      # the oracle's map: the float64 Gaussian rounded to fp32, cut at eps
            if not np.array_equal(hm == 0, ref == 0):
                fails.append("%s head %d: heat-map support differs in %d cells" % (self.name, h, int(((hm == 0) != (ref == 0)).sum())))
            ulp = np.abs(hm.astype(np.float64) - ref) / np.spacing(np.maximum(ref, np.finfo(F).tiny).astype(F))
            worst_ulp = max(worst_ulp, float(ulp.max()) if ulp.size else 0.0)
            t64, sc = self.boxes64[h]
            err = np.abs(got["target_boxes"][h].astype(np.float64) - t64)
            r = np.where(sc > 0, err / (EPS32 * np.maximum(sc, 1e-300)), np.where(err > 0, np.inf, 0.0))
            if r.size and not r.max() <= kbound:
                b, k, c = np.unravel_index(r.argmax(), r.shape)
                fails.append("%s head %d: target_boxes[%d, %d, %d] = %r, float64 %r: error / (eps32 scale) = %.3g > %.3g" %
                             (self.name, h, b, k, c, got["target_boxes"][h][b, k, c], t64[b, k, c], r.max(), kbound))
            worst = max(worst, float(r.max()) if r.size else 0.0)
        if worst_ulp > 1.0:
            fails.append("%s: heat map %.3g ulps from the float64 Gaussian" % (self.name, worst_ulp))
        return fails, worst, worst_ulp


def center_box_scale(r, case, cell):
    """float64 target row [cx - ix, cy - iy, z, log sizes, cos, sin, extras] and its scale: the offsets carry the rounding of the cell coordinate
    (scale = the coordinate itself, before the clamp); z and the extras are copies (scale 0: exact); logarithm, cosine and sine of an exact
    input: |t|."""
    W, H = case.W, case.H
    t, sc = np.zeros(len(r)), np.zeros(len(r))
    for c, (lo, vox, size) in enumerate([(case.pc_range[0], case.voxel[0], W), (case.pc_range[1], case.voxel[1], H)]):
        raw = (r[c] - float(F(lo))) / float(F(vox)) / float(F(case.stride))
        cc = min(max(raw, 0.0), size - 0.5)
        t[c], sc[c] = cc - cell[c], abs(raw)                                    # the cell is the fp32 spec's
    t[2] = r[2]
    t[3:6] = np.log(r[3:6])
    t[6], t[7] = np.cos(r[6]), np.sin(r[6])
    sc[3:8] = np.abs(t[3:8])
    t[8:] = r[7:-1]
    return t, sc


CENTER_NAMES = ["c1", "c2", "c3", "c4", "c5", "c6"]
CENTER_HEADS = [["c1", "c4"], ["c2", "c5"], ["c3", "c6"]]                        # classes interleaved over three heads


def _center_boxes(rng, B, G, dim, ncls=6):
    gt = np.zeros((B, G, dim), F)
    gt[..., 0] = rng.uniform(-13.5, 13.5, (B, G))                               # some centres outside the range on every side: clamped and drawn
    gt[..., 1] = rng.uniform(-43, 43, (B, G))
    gt[..., 2] = rng.uniform(-2, 1, (B, G))
    gt[..., 3:6] = rng.uniform(0.3, 9, (B, G, 3))
    gt[..., 6] = rng.uniform(-3.2, 3.2, (B, G))
    if dim > 8:
        gt[..., 7:-1] = rng.normal(0, 2, (B, G, dim - 8))
    gt[..., -1] = (np.arange(G)[None] + rng.integers(0, 2, (B, G))) % ncls + 1  # interleaved classes
    return gt


@functools.lru_cache(maxsize=None)
def center_cases():
    cases = []
    rng = np.random.default_rng(21)
    # ranking across lanes, waves and 256-box chunks
    for i, G in enumerate((63, 64, 65, 255, 256, 257, 600)):
        dim = 10 if i % 2 else 8
        gt = _center_boxes(rng, 2, G, dim)
        gt[0, G // 2, 3] = 0                                                    # dx = 0 in the middle: the slot stays masked off, later slots keep their rank
        gt[1, G // 3, -1] = 0                                                   # a padding row inside the list
        gt[1, (2 * G) // 3:, :] = 0 if G > 100 else gt[1, (2 * G) // 3:, :]
        cases.append(CenterCase("ranking G=%d dim=%d nmax=500" % (G, dim), gt, CENTER_NAMES, CENTER_HEADS, num_max_objs=500))
        if G in (65, 257, 600):
            cases.append(CenterCase("ranking G=%d dim=%d nmax=5" % (G, dim), gt, CENTER_NAMES, CENTER_HEADS, num_max_objs=5))
    gt = _center_boxes(rng, 2, 300, 8, ncls=1)
    gt[1, 100:] = 0
    cases.append(CenterCase("one head one class G=300 nmax=5", gt, ["c1"], [["c1"]], num_max_objs=5))
    cases.append(CenterCase("one head one class G=300", gt, ["c1"], [["c1"]], overlap=0.5, min_radius=0))
    cases.append(CenterCase("no boxes", np.zeros((2, 0, 8), F), CENTER_NAMES, CENTER_HEADS))
    # centres: on integer cell coordinates, at 0, at W - 0.5 / H - 0.5, outside on all four sides; windows clipped at every border and corner;
    # two boxes on one cell with different radii (maximum); one cell, two classes of one head (two channels)
    W, H, vx, vy, st = 24, 40, 0.25, 0.5, 4
    x_of = lambda cx: -12.0 + cx * vx * st
    y_of = lambda cy: -40.0 + cy * vy * st
    rows = []
    for cx, cy in [(0, 0), (W - 0.5, H - 0.5), (0, H - 0.5), (W - 0.5, 0), (5, 7), (23, 39), (23.5, 39.5), (-3, 10), (30, 10), (10, -2), (10, 50), (-1, -1), (40, 60),
                   (12, 0), (12, H - 0.5), (0, 20), (W - 0.5, 20), (1, 1), (W - 2, H - 2), (11.999, 19.999)]:
        rows.append([x_of(cx), y_of(cy), 0.5, 6.0, 12.0, 1.5, 0.3, 1])
    rows.append([x_of(8), y_of(30), 0.0, 2.0, 4.0, 1.0, 0.0, 1])                # same cell, radii differ
    rows.append([x_of(8.4), y_of(30.2), 0.0, 12.0, 24.0, 1.0, 1.0, 1])
    rows.append([x_of(16), y_of(12), 0.0, 5.0, 9.0, 1.0, 0.0, 1])               # same cell, classes c1 and c4 of head 0
    rows.append([x_of(16.5), y_of(12.5), 0.0, 8.0, 14.0, 1.0, 2.0, 4])
    rows.append([x_of(3), y_of(3), 0.0, 3.0, 0.0, 1.0, 0.0, 1])                 # dy = 0: skipped
    rows.append([x_of(3), y_of(3), 0.0, 1e-3, 1e-3, 1.0, 0.0, 2])               # tiny: min_radius
    gt = np.array(rows, F)[None]
    cases.append(CenterCase("centres and windows", gt, CENTER_NAMES, CENTER_HEADS))
    cases.append(CenterCase("centres and windows overlap 0.7 min_radius 0", gt, CENTER_NAMES, CENTER_HEADS, overlap=0.7, min_radius=0))
    # the radius family as boxes: sizes on the map = (h, w) of the family (voxel * stride = 1 in x, 2 in y: both exact scalings).  Every box is a
    # class of its own, so its Gaussian has a heat-map channel to itself and no larger one covers it under the per-cell maximum; centres lie in
    # cells 1 .. 23 x 1 .. 39 of a 48 x 80 map, so a window of radius up to 13 is never clipped on its far sides and the radius shows in the support
    for mo in (0.1, 0.5, 0.7):
        h, w, mos = radius_family()
        sel = mos == mo
        n = int(sel.sum())
        gt = np.zeros((1, n, 8), F)
        gt[0, :, 0], gt[0, :, 1] = rng.uniform(-11, 11, n), rng.uniform(-38, 38, n)
        gt[0, :, 3], gt[0, :, 4], gt[0, :, 5] = h[sel], w[sel] * F(2), 1.0
        gt[0, :, 7] = np.arange(1, n + 1)
        names = ["r%d" % i for i in range(n)]
        cases.append(CenterCase("radius family overlap %g" % mo, gt, names, [names], W=48, H=80, overlap=mo, min_radius=0))
    return cases


# ============================================================================================ losses
def focal_chain(x, t, w, alpha, gamma):
    """SigmoidFocalClassificationLoss.forward (loss_utils.py:9-72), the reference's op chain, in the dtype of x"""
    p = torch.sigmoid(x)
    alpha_w = t * alpha + (1 - t) * (1 - alpha)
    pt = t * (1.0 - p) + (1.0 - t) * p
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))
    loss = alpha_w * torch.pow(pt, gamma) * bce
    return loss if w is None else loss * w.unsqueeze(-1)


def smooth_l1_chain(x, t, cw, w, beta, l1=None):
    """WeightedSmoothL1Loss.forward (loss_utils.py:75-136) in the dtype of x.  `beta < 1e-5` is a comparison of Python doubles; l1 overrides it where
    beta is handed over already rounded"""
    t = torch.where(torch.isnan(t), x, t)
    diff = x - t
    if cw is not None:
        diff = diff * cw.view(1, 1, -1)
    n = torch.abs(diff)
    loss = n if (beta < 1e-5 if l1 is None else l1) else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return loss if w is None else loss * w.unsqueeze(-1)


def chain_with_grad(fn, x, go, dtype, *args):
    """value and gradient w.r.t. x of the chain `fn` in `dtype` on the CPU with autograd"""
    cast = lambda a: a.to(dtype) if torch.is_tensor(a) else a
    xi = x.to(dtype).clone().requires_grad_(True)
    out = fn(xi, *[cast(a) for a in args])
    out.backward(go.to(dtype))
    return out.detach(), xi.grad


def focal_f64(x, t, w, go, alpha, gamma):
    """float64 value, gradient, their scales, and the mask of entries whose float64 gradient is not finite (gamma < 1 at pt = 0).
    Condition of the product alpha_w * pt^gamma * bce * w in units of eps32, written once:
      p carries eps * p, 1 - p an absolute eps (p rounds to 1 for x >~ 16.7), so pt = t (1 - p) + (1 - t) p carries  Dpt = |t| + |1 - t| p + pt;
      pt^gamma moves by  Dmod = max |(pt +- eps Dpt)^gamma - pt^gamma| / eps + pt^gamma  (a difference, not a derivative: for gamma < 1 the derivative
      is unbounded at 0, the difference is not), gamma pt^(gamma - 1) likewise, with 0 below pt = 0 (the kernel's documented value there);
      bce = max(x, 0) - x t + log1p(exp(-|x|)) carries  Dbce = 2 (|max(x, 0)| + |x t| + log1p(.));
      value scale = |w| alpha_w (Dmod bce + mod Dbce + 3 mod bce), and the gradient's the same rule on
      go w alpha_w (dmod dpt bce + mod dbce),  dpt = (1 - 2 t) p (1 - p),  dbce = [x >= 0] - t - sign(x) e / (1 + e)."""
    v64, g64 = chain_with_grad(focal_chain, x, go, torch.float64, t, w, alpha, gamma)
    v64, g64 = v64.numpy(), g64.numpy()
    X, T, GO = x.double().numpy(), t.double().numpy(), go.double().numpy()
    Wt = np.ones_like(X) if w is None else np.broadcast_to(w.double().numpy()[..., None], X.shape)
    p, q = 1 / (1 + np.exp(-X)), 1 / (1 + np.exp(X))
    aw = T * float(F(alpha)) + (1 - T) * (1 - float(F(alpha)))
    pt = T * q + (1 - T) * p
    Dpt = np.abs(T) + np.abs(1 - T) * p + pt
    lo, hi = np.maximum(pt - EPS32 * Dpt, 0), pt + EPS32 * Dpt
    powg = lambda v, e: np.where(v > 0, np.power(np.maximum(v, 1e-300), e), 0.0 if e != 0 else 1.0)
    mod = powg(pt, gamma) if gamma != 0 else np.ones_like(pt)
    Dmod = (np.maximum(np.abs(powg(hi, gamma) - mod), np.abs(mod - powg(lo, gamma))) / EPS32 if gamma != 0 else 0) + mod
    dm = lambda v: gamma * powg(v, gamma - 1) if gamma != 0 else np.zeros_like(v)
    dmod = dm(pt)
    Ddmod = np.maximum(np.abs(dm(hi) - dmod), np.abs(dmod - dm(lo))) / EPS32 + np.abs(dmod)
    e = np.exp(-np.abs(X))
    terms = np.maximum(X, 0) + np.abs(X * T) + np.log1p(e)
    bce = np.maximum(X, 0) - X * T + np.log1p(e)
    Dbce = 2 * terms
    dpt = (1 - 2 * T) * p * q
    Ddpt = np.abs(1 - 2 * T) * (p + 3 * p * q)
    dbce = (X >= 0) - T - np.sign(X) * e / (1 + e)
    Ddbce = (X >= 0) + np.abs(T) + 2 * e / (1 + e) + np.abs(dbce)
    sv = np.abs(Wt) * aw * (Dmod * np.abs(bce) + mod * Dbce + 3 * mod * np.abs(bce))
    sg = np.abs(GO * Wt) * aw * (Ddmod * np.abs(dpt * bce) + np.abs(dmod) * Ddpt * np.abs(bce) + np.abs(dmod * dpt) * Dbce + Dmod * np.abs(dbce) + mod * Ddbce
                                 + 3 * (np.abs(dmod * dpt * bce) + np.abs(mod * dbce)))
    return v64, g64, sv + UNDERFLOW, sg + UNDERFLOW * np.abs(GO), ~np.isfinite(g64)


def smooth_l1_f64(x, t, cw, w, go, beta):
    """float64 value and gradient of the chain with beta as the fp32 number the kernel is given (torch compares and divides an fp32 tensor by a
    Python scalar in fp32) and the L1 / smooth choice the reference makes on the Python double, and their scales.  d = (x - t) cw carries 2 eps |d|; below beta the value 0.5 d^2 / beta carries 6 of itself, above it
    |d| - 0.5 beta carries 2 |d| + 0.5 beta + l; times the anchor weight one rounding more.  Gradient go w cw d / beta: 3 |d / beta| + 3 of
    itself; above beta go w cw sign(d): the product's 3 roundings.  NaN targets: exact zeros (scale 0)."""
    b32 = float(F(beta))
    l1 = beta < 1e-5
    v64, g64 = chain_with_grad(smooth_l1_chain, x, go, torch.float64, t, cw, w, b32, l1)
    v64, g64 = v64.numpy(), g64.numpy()
    X, T, GO = x.double().numpy(), t.double().numpy(), go.double().numpy()
    CW = np.ones(X.shape[-1]) if cw is None else cw.double().numpy()
    Wt = np.ones_like(X) if w is None else np.broadcast_to(w.double().numpy()[..., None], X.shape)
    nan = np.isnan(T)
    d = np.where(nan, 0, (X - np.where(nan, X, T)) * CW)
    n = np.abs(d)
    quad = (n < b32) & (not l1)
    l = np.where(quad, 0.5 * n * n / max(b32, 1e-300), n - (0.0 if l1 else 0.5 * b32))
    Dl = np.where(quad, 6 * l, 2 * n + 0.5 * b32 + l)
    sv = np.abs(Wt) * (Dl + l)
    dl = np.where(quad, n / max(b32, 1e-300), 1.0)
    sg = np.abs(GO * Wt * CW) * np.where(quad, 6 * dl, 3.0)
    sv[nan], sg[nan] = 0, 0
    return v64, g64, sv, sg


# products below the smallest normal fp32 number (exp(-88) squared, say) are lost in fp32 and are whatever float64 makes of them: an absolute term
# of that size, in units of eps32, in every focal scale
UNDERFLOW = float(np.finfo(F).tiny) / EPS32
FOCAL_EDGE_LOGITS = [0.0, -0.0, 1e-8, -1e-8, 8.0, -8.0, 16.7, -16.7, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0]


class LossCase:
    def __init__(self, name, kind, x, t, w, go, **kw):
        self.name, self.kind, self.x, self.t, self.w, self.go, self.kw = name, kind, x, t, w, go, kw

    @functools.cached_property
    def ref(self):
        if self.kind == "focal":
            return focal_f64(self.x, self.t, self.w, self.go, self.kw["alpha"], self.kw["gamma"])
        return smooth_l1_f64(self.x, self.t, self.kw.get("cw"), self.w, self.go, self.kw["beta"]) + (None,)

    def chain32(self):
        """the reference's chain in torch-CPU fp32 (K_REF is measured on it)"""
        if self.kind == "focal":                                                # autograd's 0 * inf at an fp32 pt of 0 (gamma < 1): the documented 0 in its place
            v, g = chain_with_grad(focal_chain, self.x, self.go, torch.float32, self.t, self.w, self.kw["alpha"], self.kw["gamma"])
            return v, torch.where(torch.isfinite(g), g, torch.zeros_like(g))
        return chain_with_grad(smooth_l1_chain, self.x, self.go, torch.float32, self.t, self.kw.get("cw"), self.w, self.kw["beta"])

    def ratios(self, value, grad):
        """worst error / (eps32 scale) of value and gradient (numpy fp32); entries whose float64 gradient is not finite are left to check_documented"""
        v64, g64, sv, sg, inf = self.ref
        out = []
        for got, ref, sc, skip in ((value, v64, sv, None), (grad, g64, sg, inf)):
            err = np.abs(got.astype(np.float64) - ref)
            r = np.where(sc > 0, err / (EPS32 * np.maximum(sc, 1e-300)), np.where(err > 0, np.inf, 0.0))
            if skip is not None:
                r = np.where(skip, 0.0, r)
            r = np.where(np.isfinite(got), r, np.inf)
            out.append(float(r.max()) if r.size else 0.0)
        return out

    def documented_zero(self, grad):
        """where float64 gives a non-finite gradient (gamma < 1 at pt = 0) the kernel's documented gradient is 0"""
        inf = self.ref[4]
        return True if inf is None else bool((grad[inf] == 0).all())


def _focal_inputs(rng, rows, C, weights):
    """logits: the edge list in every target column, then random; targets 0, 1 and soft 0.3"""
    n = rows * C
    x = (rng.normal(0, 4, n)).astype(F)
    e = np.array(FOCAL_EDGE_LOGITS, F)
    x[:min(n, len(e) * 3)] = np.tile(e, 3)[:min(n, len(e) * 3)]
    t = rng.choice(np.array([0, 1, 0.3], F), n)
    m = min(n, len(e) * 3)
    t[:m] = np.repeat(np.array([0, 1, 0.3], F), len(e))[:m]
    w = {"none": None, "zero": np.zeros(rows, F), "random": rng.uniform(0, 2, rows).astype(F)}[weights]
    go = rng.normal(0, 1, n).astype(F)
    sh = (1, rows, C)
    return (torch.from_numpy(x).view(sh), torch.from_numpy(t).view(sh), None if w is None else torch.from_numpy(w).view(1, rows), torch.from_numpy(go).view(sh))


@functools.lru_cache(maxsize=None)
def focal_cases():
    rng = np.random.default_rng(31)
    cases = []
    shapes = [(1, 1), (1, 3), (255, 1), (257, 3), (255, 10), (257, 10), (85, 3)]     # rows x C; 85 x 3 = 255 elements: one element short of a block
    i = 0
    for gamma in (2.0, 1.5, 0.5, 0.0):
        for alpha in (0.25, 0.5):
            for weights in ("none", "zero", "random"):
                rows, C = shapes[i % len(shapes)]
                i += 1
                if rows * C < 42:
                    rows, C = 42, C
                if weights == "zero" and alpha == 0.5:
                    continue
                cases.append(LossCase("focal gamma=%g alpha=%g weights=%s rows=%d C=%d" % (gamma, alpha, weights, rows, C), "focal",
                                      *_focal_inputs(rng, rows, C, weights), alpha=alpha, gamma=gamma))
    for rows, C in ((1, 1), (1, 3), (255, 1), (257, 1)):
        cases.append(LossCase("focal rows=%d C=%d" % (rows, C), "focal", *_focal_inputs(rng, rows, C, "random"), alpha=0.25, gamma=2.0))
    return cases


def _smooth_inputs(rng, rows, C, beta, weights, code_weights):
    x = rng.normal(0, 0.3, (1, rows, C)).astype(F)
    t = rng.normal(0, 0.3, (1, rows, C)).astype(F)
    cw = None
    if code_weights:
        cw = np.resize(np.array([1.0, 2.0, 0.0, -1.5, 0.5, 1.0, 3.0, 1.0], F), C)
    b = F(beta)
    flat_x, flat_t = x.reshape(-1), t.reshape(-1)
    n = flat_x.size
    # |d| exactly beta: x = t + beta with t a multiple of 2^-10 (so the difference is beta exactly), in columns whose code weight is 1; +-0
    # differences; NaN targets
    for j in range(0, min(n, 64)):
        c = j % C
        if cw is not None and abs(cw[c]) != 1.0:
            continue
        base = b if j % 4 >= 2 else F(0)                                       # 2 beta - beta and beta - 0: both differences are beta exactly
        flat_t[j] = base
        flat_x[j] = base + b if j % 2 == 0 else base - b
        assert F(flat_x[j] - flat_t[j]) in (b, -b)
    if n > 80:
        flat_t[64:72] = flat_x[64:72]                                           # +0 difference
        flat_x[72:76], flat_t[72:76] = F(0.0), F(-0.0)
        flat_t[76:80] = np.nan
    w = {"none": None, "zero": np.zeros(rows, F), "random": rng.uniform(0, 2, rows).astype(F)}[weights]
    go = rng.normal(0, 1, (1, rows, C)).astype(F)
    return (torch.from_numpy(x), torch.from_numpy(t), None if w is None else torch.from_numpy(w).view(1, rows), torch.from_numpy(go),
            None if cw is None else torch.from_numpy(cw))


# the last one is float32(1e-5) as a double: below 1e-5, so the reference takes |d|, though it rounds to the same fp32 number as 1e-5 itself
# 0.7720242 (an fp32 number) is a beta at which the two branches differ in bits at |d| = beta: 0.5 (b b) / b = 0.38601214, b - 0.5 b = 0.3860121.
# The reference takes the second (`n < beta` is false), so `<` against `<=` shows in the value there; at 1/9, 1 and 1e-5 the branches agree.
BETA_BRANCHES_DIFFER = float(F(0.7720242))
SMOOTH_BETAS = [1.0 / 9.0, 1.0, 0.0, 1e-5, float(F(1e-5)), BETA_BRANCHES_DIFFER]


@functools.lru_cache(maxsize=None)
def smooth_l1_cases():
    rng = np.random.default_rng(32)
    cases = []
    shapes = [(255, 7), (257, 8), (85, 3), (1, 8), (257, 1), (1, 1), (255, 1)]
    i = 0
    for beta in SMOOTH_BETAS:
        for move in (0, 1, -1):
            if beta in (0.0, float(F(1e-5)), BETA_BRANCHES_DIFFER) and move != 0:
                continue
            bb = float(up(beta, move)) if move else beta                        # unmoved: the Python double itself, as a config gives it
            for weights, code_weights in (("random", True), ("none", False), ("zero", True)):
                if weights == "zero" and move != 0:
                    continue
                rows, C = shapes[i % len(shapes)]
                i += 1
                x, t, w, go, cw = _smooth_inputs(rng, rows, C, F(beta), weights, code_weights)     # |d| = the UNMOVED beta: the moved one is an ulp off it
                cases.append(LossCase("smooth-L1 beta=%.9g (%+d ulp) weights=%s cw=%s rows=%d C=%d" % (beta, move, weights, code_weights, rows, C),
                                      "smooth_l1", x, t, w, go, beta=bb, cw=cw))
    return cases


def stride_loss_inputs(kind):
    """one call of 1048576 + 300 elements: past the grid cap of 4096 blocks x 256 threads"""
    rng = np.random.default_rng(33)
    rows, C = (1048576 + 300) // 4, 4
    if kind == "focal":
        x, t, w, go = _focal_inputs(rng, rows, C, "random")
        return LossCase("focal stride loop", "focal", x, t, w, go, alpha=0.25, gamma=2.0)
    x, t, w, go, cw = _smooth_inputs(rng, rows, C, F(1.0 / 9.0), "random", True)
    return LossCase("smooth-L1 stride loop", "smooth_l1", x, t, w, go, beta=1.0 / 9.0, cw=cw)
