"""Hand-written restatement of the focal sparse conv expansion (numpy, plus a differentiable torch-double form of the feature step) and of the
reference's FocalLoss.  It follows the closed form -- selection, candidates, union in canonical order, one weight per input row -- not the
reference's sort / unique_consecutive / index_add_ sequence.

  s (n, 27) fp32 = sigmoid(imps): column 26 the voxel importance mv, column o < 26 the importance of OFFSETS[o].
  1. foreground: topk -- per scene the int(n_b * threshold) rows of largest mv, equal values lower row first; else mv > float32(threshold).
  2. candidates: foreground row j, offset o with s[j, o] >= float32(threshold) -> coords[j] + OFFSETS[o], kept iff 0 < c < dim on every axis.
  3. output set: input cells and kept candidates, each once, ascending ((b*Z + z)*Y + y)*X + x.
  4. features: new cell 0; input row i gets f[i] * (mv[i] if mask_multi) * w[i]; w[i] = (1 + sum s[j, o]) / (1 + c_i) over the c_i kept candidates
     landing on a foreground i, 1 for background rows and under skip_mask_kernel.
  5. gradients: autograd of step 4 with the selection constant (torch_features).
"""
import numpy as np

OFFSETS = np.array([(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)], np.int64)


def linear_key(coords, shape):
    c = np.asarray(coords, np.int64)
    return ((c[:, 0] * shape[0] + c[:, 1]) * shape[1] + c[:, 2]) * shape[2] + c[:, 3]


def select(s, coords, batch, topk, threshold):
    """fore (n) bool"""
    mv = np.asarray(s, np.float32)[:, 26]
    if not topk:
        return mv > np.float32(threshold)
    fore = np.zeros(len(mv), bool)
    for b in range(batch):
        rows = np.nonzero(coords[:, 0] == b)[0]
        k = min(int(len(rows) * threshold), len(rows))          # the float64 product Python forms: 0.29 * 100 -> 28
        order = sorted(rows, key=lambda r: (-float(mv[r]), int(r)))
        fore[np.array(order[:k], np.int64)] = True
    return fore


def candidates(s, coords, fore, shape, threshold):
    """The kept candidates as (j (m), o (m), cells (m, 4))."""
    s = np.asarray(s, np.float32)
    thr = np.float32(threshold)
    J, O, cells = [], [], []
    for j in np.nonzero(fore)[0]:
        for o in range(26):
            if s[j, o] >= thr:
                c = coords[j, 1:].astype(np.int64) + OFFSETS[o]
                if (c > 0).all() and (c < np.array(shape)).all():
                    J.append(j), O.append(o), cells.append((int(coords[j, 0]),) + tuple(int(v) for v in c))
    return np.array(J, np.int64), np.array(O, np.int64), np.array(cells, np.int64).reshape(-1, 4)


def expand(s, coords, shape, batch, topk, threshold):
    """-> dict(fore, out_coords (num_out, 4) int32, row_of_in (n), J, O, I): the structure of the expansion.  (J, O, I): kept candidate (j, o) lands on
    the FOREGROUND input row I (candidates on background rows or new cells carry no weight)."""
    coords = np.asarray(coords)
    fore = select(s, coords, batch, topk, threshold)
    J, O, cells = candidates(s, coords, fore, shape, threshold)
    in_key = linear_key(coords, shape)
    assert len(np.unique(in_key)) == len(in_key), "input coordinates must be distinct"
    all_cells = np.concatenate([coords.astype(np.int64), cells], axis=0)
    keys, first = np.unique(linear_key(all_cells, shape), return_index=True)
    out_coords = all_cells[first].astype(np.int32)
    row_of_in = np.searchsorted(keys, in_key).astype(np.int32)
    row_of_key = {int(k): i for i, k in enumerate(in_key)}
    land = np.array([row_of_key.get(int(k), -1) for k in linear_key(cells, shape)], np.int64)
    keep = (land >= 0) & fore[np.clip(land, 0, None)] if len(land) else np.zeros(0, bool)
    return dict(fore=fore, out_coords=out_coords, row_of_in=row_of_in, J=J[keep], O=O[keep], I=land[keep], n_candidates=len(J))


def features(f, s, ex, mask_multi, skip_mask_kernel, dtype=np.float64):
    """Step 4 in `dtype` -> (out (num_out, C), w (n), cnt (n))."""
    f, s = np.asarray(f, dtype), np.asarray(s, dtype)
    n = len(f)
    acc, cnt = np.ones(n, dtype), np.zeros(n, np.int64)
    if not skip_mask_kernel:
        order = np.lexsort((ex["O"], ex["I"]))                # per landing row, offsets ascending: the order the kernels add in
        for i, j, o in zip(ex["I"][order], ex["J"][order], ex["O"][order]):
            acc[i] += s[j, o]
            cnt[i] += 1
    w = acc / (1 + cnt).astype(dtype)
    rows = f * s[:, 26:27] if mask_multi else f
    out = np.zeros((len(ex["out_coords"]), f.shape[1]), dtype)
    out[ex["row_of_in"]] = rows * w[:, None]
    return out, w, cnt


def torch_features(f, s, ex, mask_multi, skip_mask_kernel):
    """Step 4 on torch double tensors f (n, C), s (n, 27) (requires_grad as the caller likes), differentiable; the selection in `ex` is constant."""
    import torch
    n = f.shape[0]
    I, J, O = (torch.from_numpy(ex[k]) for k in ("I", "J", "O"))
    w = torch.ones(n, dtype=f.dtype)
    if not skip_mask_kernel and len(I):
        total = torch.ones(n, dtype=f.dtype).index_add(0, I, s[J, O])
        cnt = torch.zeros(n, dtype=f.dtype).index_add(0, I, torch.ones(len(I), dtype=f.dtype))
        w = total / (1 + cnt)
    rows = f * s[:, 26:27] if mask_multi else f
    out = torch.zeros((len(ex["out_coords"]), f.shape[1]), dtype=f.dtype)
    return out.index_copy(0, torch.from_numpy(ex["row_of_in"].astype(np.int64)), rows * w[:, None])


def torch_focal_loss(scores, target, gamma=2.0, eps=1e-7):
    """focal_loss below on a torch double tensor, differentiable."""
    import torch
    p = torch.softmax(scores, dim=1).clamp(eps, 1 - eps)
    y = torch.eye(scores.shape[1], dtype=scores.dtype)[target.long()]
    return (-y * torch.log(p) * (1 - p) ** gamma).mean()


def focal_loss(scores, target, gamma=2.0, eps=1e-7):
    """The reference's FocalLoss on (n, classes) scores: softmax, clamp, -log(p) * (1 - p)^gamma at the target class, mean over all n * classes."""
    x = np.asarray(scores, np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p = np.clip(p / p.sum(1, keepdims=True), eps, 1 - eps)
    y = np.eye(x.shape[1])[np.asarray(target, np.int64)]
    return float((-y * np.log(p) * (1 - p) ** gamma).mean())
