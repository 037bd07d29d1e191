"""Float64 numpy restatement of the local-prototype labels inside the queried superpixels and of their two evaluation modes, written
from the semantics (not collected; imported by the tests and by tools/gen_golden_within_multihot.py).  Full-resolution tensors in, as
the reference's ``pseudo_label_generation`` takes them.

  valid      mask set, id in [0, S), a non-empty target row (one-hot rows count).
  prototype  of (s, c), c in targets[s]: the valid pixel of s with the largest softmax(logits)[c], ties to the lowest pixel index.
  label      the class of the prototype of the pixel's own superpixel whose feature has the largest inner product with its own,
             candidates in ascending class order, replaced on strict '>'.
  'filt'     the label survives where it equals the first arg-max of the logits; a prototype pixel takes its own class, the highest
             when it is the prototype of several.
  below      per picture, the valid pixels whose winning similarity is below max_c (logit_c * Y_c); below_margin: the smallest distance
             between the two over the valid pixels.
  gaps       gap_sim: best similarity minus the best among the candidates with ANOTHER prototype pixel; gap_proto: over the candidates
             of the superpixel, the smallest difference between the largest and the next DIFFERENT probability; gap_arg: the two
             largest logits' difference.  gap = their minimum over the decisions the pixel's label goes through ('filt': a prototype
             pixel depends on gap_proto alone).  loose: some candidate's two largest different probabilities lie within ``near``
             (relative) of each other.  gap_sim: the same minimum without gap_proto (for a comparison that uses
             ``loose`` instead).  All inf / False off the valid pixels.
"""
import numpy as np
import torch

from mulactseg_amd import synth

import online_plbl_restated as O

# the golden case (tests/golden/g21_within_multihot.npz): the geometry of g15, three pictures, the third with nothing selected
SEED, N, C, CH, H, W, HQ, WQ, S, IGNORE = 21, 3, 20, 256, 40, 44, 10, 11, 48, 255


def ground_truth(seed, n, c, h, w, p_ignore=0.1):
    """int64 [n,h,w] in 0..c-1 with about ``p_ignore`` of the pixels at IGNORE"""
    rs = np.random.RandomState(seed + 3000)
    gt = np.stack([synth.class_map(seed + 3100 + i, h, w, c, blob=6) for i in range(n)]).astype(np.int64)
    gt[rs.random_sample(gt.shape) < p_ignore] = IGNORE
    return gt


def inputs(seed=SEED):
    """(zq, featq, targets u8 [N,S,C], spx int64 [N,H,W], mask bool [N,H,W], gt int64 [N,H,W]) as numpy.  Every superpixel has a
    non-empty row (else the reference raises), so the rows of the unselected ones are set without a valid pixel; picture 2 has nothing
    selected."""
    zq, featq, _, tgt, spx, msk = O.inputs(seed, N, C, CH, H, W, HQ, WQ, S)
    msk[2] = False
    gt = ground_truth(seed, N, C - 1, H, W)
    return zq, featq, tgt, spx, msk, gt


def generate(logits, feats, targets, spx, mask, mode='proto', near=1e-5):
    logits, feats = np.asarray(logits, dtype=np.float64), np.asarray(feats, dtype=np.float64)
    targets, spx, mask = np.asarray(targets).astype(np.int64), np.asarray(spx).astype(np.int64), np.asarray(mask).astype(bool)
    Nn, Cc, Hh, Ww = logits.shape
    Ss = targets.shape[1]
    z = logits.reshape(Nn, Cc, -1)
    ez = np.exp(z - z.max(axis=1, keepdims=True))
    den = np.zeros((Nn, 1, Hh * Ww))
    for c in range(Cc):
        den[:, 0] += ez[:, c]
    prob = ez / den
    f = feats.reshape(Nn, feats.shape[1], -1)
    labels = np.full((Nn, Hh * Ww), 255, dtype=np.int64)
    valid = np.zeros((Nn, Hh * Ww), dtype=bool)
    loose = np.zeros((Nn, Hh * Ww), dtype=bool)
    gap = np.full((Nn, Hh * Ww), np.inf)
    gap_sim = np.full((Nn, Hh * Ww), np.inf)
    below = np.zeros(Nn, dtype=np.int64)
    below_margin = np.inf
    nproto = 0
    for n in range(Nn):
        ids, m = spx[n].reshape(-1), mask[n].reshape(-1)
        for s in range(Ss):
            if int(targets[n, s].sum()) == 0:
                continue
            px = np.nonzero(m & (ids == s))[0]
            if px.size == 0:
                continue
            valid[n, px] = True
            cands = np.nonzero(targets[n, s, :Cc])[0].tolist()
            if not cands:
                continue
            protos, gap_proto = [], np.inf
            for c in cands:
                v = prob[n, c, px]
                protos.append(int(px[np.nonzero(v == v.max())[0][0]]))
                lower = v[v < v.max()]
                if lower.size:
                    gap_proto = min(gap_proto, float(v.max() - lower.max()))
                    if float(lower.max()) >= (1.0 - near) * float(v.max()):
                        loose[n, px] = True
            nproto += len(cands)
            sims = np.stack([(f[n][:, px] * f[n][:, [q]]).sum(axis=0) for q in protos], axis=1)        # [pixels, candidates]
            best = np.full(px.size, -np.inf)
            arg = np.zeros(px.size, dtype=np.int64)
            for j in range(len(cands)):
                better = sims[:, j] > best
                best = np.where(better, sims[:, j], best)
                arg = np.where(better, j, arg)
            pt = np.asarray(protos)
            second = np.where(pt[None, :] != pt[arg][:, None], sims, -np.inf).max(axis=1)
            lab = np.asarray(cands)[arg]
            gs = best - second
            g = np.minimum(gs, gap_proto)
            zz = z[n][:, px]
            row = np.zeros(Cc)
            row[cands] = 1.0
            glob = (zz * row[:, None]).max(axis=0)
            below[n] += int((best < glob).sum())
            below_margin = min(below_margin, float(np.abs(best - glob).min()))
            if mode == 'filt':
                top = zz.argmax(axis=0)
                two = np.sort(zz, axis=0)[-2:]
                g = np.minimum(g, two[1] - two[0])
                lab = np.where(top == lab, lab, 255)
                for q, c in zip(protos, cands):                         # ascending: the highest class is written last
                    lab[px == q] = c
                    g[px == q] = gap_proto
                gs = np.where(np.isin(px, protos), np.inf, np.minimum(gs, two[1] - two[0]))
            labels[n, px] = lab
            gap[n, px] = g
            gap_sim[n, px] = gs
    sh = (Nn, Hh, Ww)
    return dict(labels=labels.reshape(sh), valid=valid.reshape(sh), gap=gap.reshape(sh), gap_sim=gap_sim.reshape(sh),
                loose=loose.reshape(sh), below=below, nproto=nproto, below_margin=below_margin)


def counts(labels, gt, K, ignore=IGNORE):
    """seen / correct / positive of MeanIoU._after_step (utils/miou.py:23-38), then three zeros: int64 [3K+3]"""
    labels, gt = np.asarray(labels).astype(np.int64).ravel(), np.asarray(gt).astype(np.int64).ravel()
    keep = gt != ignore
    out = np.zeros(3 * K + 3, dtype=np.int64)
    for c in range(K):
        out[c] = int((keep & (gt == c)).sum())
        out[K + c] = int((keep & (gt == c) & (labels == c)).sum())
        out[2 * K + c] = int((keep & (labels == c)).sum())
    return out


def sim_err_f32(feats, mask):
    """the largest |float32 - float64| inner product of torch.mm among the selected pixels' features of one picture each"""
    feats, mask = torch.as_tensor(feats), torch.as_tensor(mask)
    err = 0.0
    for i in range(feats.shape[0]):
        vf = feats[i].permute(1, 2, 0).reshape(-1, feats.shape[1])[mask[i].reshape(-1)]
        if vf.shape[0]:
            err = max(err, float((torch.mm(vf, vf.T).double() - torch.mm(vf.double(), vf.double().T)).abs().max()))
    return err


def edge_case():
    """``online_plbl_restated.edge_case`` (37 x 45, four pictures) with three additions: in picture 0 a selected superpixel whose row is
    emptied (``empty``: its pixels stay 255) and selected pixels with an id outside [0, S) (``stray``, a bool map of picture 0); picture 2
    (one-hot rows only) now has labels; picture 3 keeps the superpixel ``pair`` whose two classes share their prototype pixel.  Plus a
    ground truth."""
    e = O.edge_case()
    spx0, m0 = e['spx'][0], e['msk'][0]
    sel = np.unique(spx0[m0 & (spx0 < e['S'])])
    empty = int(sel[0])
    e['tgt'][0, empty] = 0
    ys, xs = np.nonzero(m0 & (spx0 == int(sel[1])))
    stray = np.zeros_like(m0)
    stray[ys[:3], xs[:3]] = True
    spx0[stray] = e['S'] + 7
    h, w = e['size']
    e.update(empty=empty, stray=stray, gt=ground_truth(7, 4, e['C'] - 1, h, w))
    return e
