"""Float64 restatement of the similarity-weighted online pseudo labels, written from the semantics (not collected; imported by the
tests and by the golden recorder).  Full-resolution tensors in.  Inputs, ``edge_case()`` and the ``loose`` / ``gap`` notions are those of
``online_plbl_restated``.

  valid pixel, prototype, sim, candidate order: as ``online_plbl_restated.generate``.
  sim weight    weight of a valid pixel = its inner product with the prototype of its label (may be negative); labels unchanged.
  soft weights  of a valid pixel over its candidates: softmax(sim / tau).
  live          a picture with at least one valid pixel.
  counted       mask set, id in [0, S), picture live.
  soft CE       p = softmax(logits / T); a valid pixel adds sum_c w_c * -log(p_c + 1e-8), a counted pixel with one candidate
                -log(p_c + 1e-8), with none 0; the mean runs over the counted pixels (0 without one).
  signed CE     mean of the non-zero weight * CE terms, negative ones included (0 without one).
"""
import numpy as np
import torch

import online_plbl_restated as R

EPS = 1e-8


def _probabilities(logits, temp):
    logits = np.asarray(logits, dtype=np.float64)
    N, C = logits.shape[:2]
    z = (logits / temp).reshape(N, C, -1)
    ez = np.exp(z - z.max(axis=1, keepdims=True))
    den = np.zeros((N, 1, z.shape[2]))
    for c in range(C):
        den[:, 0] += ez[:, c]
    return ez / den


def similarities(logits_p, feats, targets, spx, mask, temp, near=0.0):
    """-> dict: sims f64 [N,C,H,W] (NaN where undefined: off the candidates of the valid pixels), valid bool [N,H,W], live bool [N],
    loose bool [N,H,W] (``online_plbl_restated.generate``: the prototype pick of the superpixel depends on rounding within ``near``)"""
    prob = _probabilities(logits_p, temp)
    feats = np.asarray(feats, dtype=np.float64)
    targets, spx, mask = np.asarray(targets).astype(np.int64), np.asarray(spx).astype(np.int64), np.asarray(mask).astype(bool)
    N, C, H, W = np.asarray(logits_p).shape
    S = targets.shape[1]
    f = feats.reshape(N, feats.shape[1], -1)
    sims = np.full((N, C, H * W), np.nan)
    valid = np.zeros((N, H * W), dtype=bool)
    loose = np.zeros((N, H * W), dtype=bool)
    for n in range(N):
        ids, m = spx[n].reshape(-1), mask[n].reshape(-1)
        for s in range(S):
            if int(targets[n, s].sum()) <= 1:
                continue
            cands = np.nonzero(targets[n, s, :C])[0].tolist()
            px = np.nonzero(m & (ids == s))[0]
            if px.size == 0:
                continue
            valid[n, px] = True
            for c in cands:
                v = prob[n, c, px]
                q = int(px[np.nonzero(v == v.max())[0][0]])
                below = v[v < v.max()]
                if near and below.size and float(below.max()) >= (1.0 - near) * float(v.max()):
                    loose[n, px] = True
                sims[n, c, px] = (f[n][:, px] * f[n][:, [q]]).sum(axis=0)
    shape = (N, H, W)
    return dict(sims=sims.reshape(N, C, H, W), valid=valid.reshape(shape), live=valid.any(axis=1), loose=loose.reshape(shape))


def sim_weight(sims):
    """-> (labels int64 [N,H,W] with 255, weight f64 [N,H,W]): ascending class order, a later candidate replaces the best on strict '>'"""
    N, C, H, W = sims.shape
    best = np.full((N, H, W), -np.inf)
    lab = np.full((N, H, W), 255, dtype=np.int64)
    for c in range(C):
        v = sims[:, c]
        better = ~np.isnan(v) & ((lab == 255) | (np.nan_to_num(v, nan=-np.inf) > best))
        best = np.where(better, v, best)
        lab = np.where(better, c, lab)
    return lab, np.where(lab == 255, 0.0, best)


def soft_weights(sims, tau):
    """softmax(sim / tau) over the defined classes of every pixel; NaN where ``sims`` is"""
    z = sims / tau
    m = np.nanmax(np.where(np.isnan(z), -np.inf, z), axis=1, keepdims=True)
    e = np.exp(z - m)
    with np.errstate(invalid='ignore'):
        return e / np.nansum(e, axis=1, keepdims=True)


def soft_loss(logits, targets, spx, mask, softw, live, temp):
    """(value, gradient with respect to ``logits`` f64 numpy, counted pixels)"""
    z = torch.as_tensor(np.asarray(logits)).double().clone().requires_grad_(True)
    N, C, H, W = z.shape
    targets, spx, mask = np.asarray(targets).astype(np.int64), np.asarray(spx).astype(np.int64), np.asarray(mask).astype(bool)
    S = targets.shape[1]
    counted = mask & (spx >= 0) & (spx < S) & np.asarray(live).astype(bool)[:, None, None]
    tw = np.zeros((N, C, H, W))
    for n in range(N):
        rows = targets[n][np.clip(spx[n], 0, S - 1)]                    # [H,W,cols]
        multi = rows.sum(-1) > 1
        one = np.moveaxis(rows[..., :C], -1, 0).astype(np.float64)
        tw[n] = np.where(multi[None], np.nan_to_num(np.asarray(softw[n], dtype=np.float64), nan=0.0) * one, one) * counted[n][None]
    p = torch.softmax(z / temp, dim=1)
    total = (torch.from_numpy(tw) * -torch.log(p + EPS)).sum()
    cnt = int(counted.sum())
    val = total / cnt if cnt else total * 0.0
    (g,) = torch.autograd.grad(val, z)
    return float(val.detach()), g.numpy(), cnt


def signed_loss(logits, labels, weight, temp):
    """(value, gradient, counted terms, mean |term|): mean of the non-zero ``weight * CE``, whatever their sign"""
    z = torch.as_tensor(np.asarray(logits)).double().clone().requires_grad_(True)
    labels = torch.as_tensor(np.asarray(labels)).long()
    ce = torch.nn.functional.cross_entropy(z / temp, labels, ignore_index=255, reduction='none')
    term = torch.as_tensor(np.asarray(weight)).double() * ce
    nz = term != 0
    val = term[nz].mean() if bool(nz.any()) else term.sum() * 0.0
    (g,) = torch.autograd.grad(val, z)
    return float(val.detach()), g.numpy(), int(nz.sum()), float(term[nz].abs().mean().detach()) if bool(nz.any()) else 0.0


def negated_case(seed=23, c=20, ch=64, h=21, w=26, s=12, gmax=None):
    """Every non-prototype valid pixel's feature is the negation of its superpixel's prototypes: all prototypes of a superpixel share
    one unit vector u_s, every other valid pixel carries -u_s, so every similarity weight off the prototypes is -1 (a prototype pixel's
    own weight is its squared norm and cannot be negative).  Built at full
    resolution with the quarter maps equal to it (h x w from h x w: the upsampling is the identity).  Returns a dict like
    ``online_plbl_restated.edge_case`` plus ``proto``: bool [N,H,W], the prototype pixels.  The prototype pixels depend on the logits
    alone: with ``gmax`` (the library's arg-pixel table [N,S,C] for these logits and any features) they are read from it, so that no
    float32 near-tie of two probabilities can move one; without it they are the float64 arg-max."""
    zq_p, featq, zq, tgt, spx, msk = R.inputs(seed, 2, c, ch, h, w, h, w, s, frac=0.7)
    prob = _probabilities(zq_p, R.T)
    N = zq_p.shape[0]
    rs = np.random.RandomState(seed + 1)
    proto = np.zeros((N, h * w), dtype=bool)
    feat = featq.reshape(N, ch, -1).copy()
    for n in range(N):
        ids, m = spx[n].reshape(-1), msk[n].reshape(-1)
        for k in range(s):
            if int(tgt[n, k].sum()) <= 1:
                continue
            px = np.nonzero(m & (ids == k))[0]
            if px.size == 0:
                continue
            u = rs.standard_normal(ch)
            u = (u / np.sqrt((u * u).sum())).astype(np.float32)
            feat[n][:, px] = -u[:, None]
            for cls in np.nonzero(tgt[n, k, :c])[0]:
                if gmax is not None:
                    q = 0xffffffff - (int(np.asarray(gmax).view(np.uint64)[n, k, cls]) & 0xffffffff)
                else:
                    v = prob[n, cls, px]
                    q = int(px[np.nonzero(v == v.max())[0][0]])
                proto[n, q] = True
                feat[n][:, q] = u
    return dict(zq_p=zq_p, featq=np.ascontiguousarray(feat.reshape(N, ch, h, w)), zq=zq, tgt=tgt, spx=spx, msk=msk, size=(h, w), S=s, C=c,
                proto=proto.reshape(N, h, w))
