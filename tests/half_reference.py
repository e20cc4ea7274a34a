"""Float64 layer reference, derived tolerance and shared case list for the half-precision eval list (csrc/sparse_conv_half.hip, spconv/chain.py).

Reference of ONE layer, fed with the layer's own fp16 input and the fp16-rounded weights (both widened exactly to float64):
    y64 = relu?( scale * (sum_k sum_c x16 * w16 + bias) + shift + residual16 )                 through oracle.spconv's rulebook and conv_forward.

Tolerance (derived, not measured).  fp16 x fp16 products are exact in fp32, so the only errors are the fp32 sums, the epilogue's fp32 operations and the
final store.  With P = sum_k sum_c |x16| * |w16| (float64, through the rulebook) a sum of at most 27 * C_in fp32 terms in any order, followed by the
epilogue's additions and one fused multiply-add, satisfies
    E_acc = (27 * C_in + 4) * 2^-23 * ( |scale| * (P + |bias|) + |shift| + |residual| )
(the form of tests/dense_reference.py: 2^-23 is twice the unit roundoff of fp32), and
    tol = E_acc                                          for an fp32 store
    tol = E_acc + 2^-11 * (|y64| + E_acc) + 2^-25        for an fp16 store: half an ulp of a normal fp16 value, half the spacing of the subnormals (2^-24)
compared after the ReLU, which is 1-Lipschitz.  An absent scale is 1, an absent shift / bias / residual 0."""
import numpy as np
import torch

from oracle import spconv as osp

EPS32 = 2.0 ** -23
EPS16 = 2.0 ** -11
SUB16 = 2.0 ** -25
K_MAX = 27

# ---------------------------------------------------------------------------------------------------------------- the shared case list
CHANNELS = [(16, 16), (16, 32), (32, 64), (64, 64), (64, 128), (128, 128)]
SUBM_ROWS = [1, 15, 16, 17, 33, 300]        # 17 and 33: a last tile that is mostly padding; 300: 19 tiles with ragged masks
GRID = (9, 24, 24)                          # two scenes of it
STORES = ("float16", "float32")


def _sites(rng, n, batch, shape):
    """n distinct random sites, (n, 4) int32 [b, z, y, x], in ascending key order"""
    cells = batch * shape[0] * shape[1] * shape[2]
    keys = np.sort(rng.choice(cells, size=n, replace=False))
    x = keys % shape[2]
    t = keys // shape[2]
    y = t % shape[1]
    t //= shape[1]
    return np.stack([t // shape[0], t % shape[0], y, x], axis=1).astype(np.int32)


def tables():
    """[(tag, coords (N, 4) int32, batch, shape, ksize, stride, padding, subm)]: submanifold tables (K = 27) of SUBM_ROWS sites -- 300 on two scenes of GRID,
    the small ones in a box dense enough for neighbours --, a (3, 3, 3) stride-2 table and a (3, 1, 1) stride-(2, 1, 1) table (K = 3) on the 300 sites."""
    rng = np.random.default_rng(1600)
    out = []
    for n in SUBM_ROWS:
        batch, shape = (2, GRID) if n == 300 else (1, (3, 4, 6))
        out.append((f"subm {n} rows", _sites(rng, n, batch, shape), batch, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1), True))
    c300 = out[-1][1]
    out.append(("stride 2", c300, 2, GRID, (3, 3, 3), (2, 2, 2), (1, 1, 1), False))
    out.append(("(3,1,1) stride (2,1,1)", c300, 2, GRID, (3, 1, 1), (2, 1, 1), (0, 0, 0), False))
    return out


def oracle_table(t):
    """-> (nbr_out (K, n_out) int32, n_in) of a tables() entry, from the float64 oracle's rulebook builders"""
    tag, coords, batch, shape, ksize, stride, padding, subm = t
    if subm:
        return osp.rulebook_subm(coords, shape, ksize), len(coords)
    _, nbr_out, _, _ = osp.rulebook_sparse(coords, shape, ksize, stride, padding)
    return nbr_out, len(coords)


def operands(rng, n_in, n_out, K, cin, cout):
    """fp16 input rows, fp32 weights scaled like a trained layer's, and the four epilogue tensors (fp32; the residual already an fp16 value)"""
    x16 = torch.from_numpy(rng.normal(size=(n_in, cin)).astype(np.float32)).half()
    w = torch.from_numpy((rng.normal(size=(K, cin, cout)) * 1.5 / np.sqrt(0.4 * K * cin)).astype(np.float32))
    t = {"bias": rng.normal(size=cout), "scale": rng.uniform(0.5, 1.5, size=cout) * rng.choice([-1.0, 1.0], size=cout), "shift": rng.normal(size=cout)}
    t = {k: torch.from_numpy(v.astype(np.float32)) for k, v in t.items()}
    t["residual"] = torch.from_numpy(rng.normal(size=(n_out, cout)).astype(np.float32)).half()
    return x16, w, t


# ---------------------------------------------------------------------------------------------------------------- reference and bound
def products(x16, nbr, w):
    """(sum x16 * w16, sum |x16| * |w16|) in float64 through the rulebook; w fp32 (K, C_in, C_out), rounded to fp16 here"""
    x64 = x16.double().numpy()
    w64 = w.half().double().numpy()
    return osp.conv_forward(x64, nbr, w64), osp.conv_forward(np.abs(x64), nbr, np.abs(w64))


def expected(z, p, cin, terms, names, store):
    """(y64, tol) from products(): terms = {bias, scale, shift (C_out,) fp32; residual (n, C_out) fp16}, names = the terms in use (+ 'relu')"""
    one, zero = np.ones(z.shape[1]), np.zeros(z.shape[1])
    b = terms["bias"].double().numpy() if "bias" in names else zero
    sc = terms["scale"].double().numpy() if "scale" in names else one
    sh = terms["shift"].double().numpy() if "scale" in names else zero
    rs = terms["residual"].double().numpy() if "residual" in names else np.zeros_like(z)
    y = sc * (z + b) + sh + rs
    if "relu" in names:
        y = np.maximum(y, 0.0)
    e_acc = (K_MAX * cin + 4) * EPS32 * (np.abs(sc) * (p + np.abs(b)) + np.abs(sh) + np.abs(rs))
    tol = e_acc if store == "float32" else e_acc + EPS16 * (np.abs(y) + e_acc) + SUB16
    return y, tol


def excess(got, y64, tol):
    """largest |got - y64| / tol (inf when got has a NaN or an infinity the reference does not have)"""
    g = got.double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    if g.shape != y64.shape or not np.isfinite(g).all():
        return float("inf")
    return float((np.abs(g - y64) / tol).max()) if g.size else 0.0


def assert_within(got, y64, tol, name=""):
    worst = excess(got, y64, tol)
    assert worst <= 1.0, (name, "largest error / bound", worst)


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation (torch, CPU)
def truncate_half(v):
    """fp32 -> fp16 by dropping mantissa bits (toward zero) instead of rounding: a seeded fault"""
    h = v.half()
    over = h.float().abs() > v.abs()
    bits = h.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(torch.float16)               # one step toward zero (sign-magnitude: the magnitude bits shrink)


def emulate(x16, nbr, w, terms, names, store, fault=None):
    """The kernel's arithmetic in torch on the CPU: fp16-rounded operands widened to fp32, gathered, accumulated in fp32 offset by offset, fp32
    epilogue in the kernel's order, .half() (round to nearest even) or fp32.  fault: None | 'acc16' | 'no_residual' | 'truncate' | 'swap'."""
    xf, wf = x16.float(), w.half().float()
    nbr_t = torch.from_numpy(np.asarray(nbr)).long()
    n_out, cout = nbr_t.shape[1], w.shape[2]
    acc = torch.zeros((n_out, cout), dtype=torch.float16 if fault == "acc16" else torch.float32)
    for k in range(nbr_t.shape[0]):
        has = nbr_t[k] >= 0
        if bool(has.any()):
            part = xf[nbr_t[k][has]] @ wf[k]
            acc[has] = (acc[has].float() + part).to(acc.dtype)
    v = acc.float()
    if "bias" in names:
        v = v + terms["bias"]
    if "scale" in names:
        a, b = (terms["shift"], terms["scale"]) if fault == "swap" else (terms["scale"], terms["shift"])
        v = (v.double() * a.double() + b.double()).float()                      # one rounding: the fused multiply-add
    if "residual" in names and fault != "no_residual":
        v = v + terms["residual"].float()
    if "relu" in names:
        v = v.clamp_min(0)
    if store == "float32":
        return v
    return truncate_half(v) if fault == "truncate" else v.half()
