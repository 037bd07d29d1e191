"""Float64 torch restatement of the online local-prototype pseudo labels and the cross entropy on them, written from the semantics
(not collected; imported by the tests and by the golden recorder).  Full-resolution tensors in, as the reference's classes take them.

  generate   valid pixel = mask set, id in [0, S), more than one target bit.  Prototype of (s, c), c in targets[s] = the valid pixel of s
             with the largest softmax(logits / T)[c], ties to the lowest pixel index.  A valid pixel takes the class of the prototype of
             its own superpixel whose feature has the largest inner product with its own, candidates in ascending class order, replaced
             on strict '>'.  weight = softmax(logits / T)[label]; with weight_wo_proto a prototype pixel's weight is 1.
             gap = best similarity minus the best similarity among the candidates with ANOTHER prototype pixel (inf when there is none):
             how far the label is from depending on rounding.
  loss       'plain': mean CE over the labelled pixels (0 without one); 'weighted': mean of the non-zero weight * CE (0 without one);
             'joint': the same, NaN without one; th: (th < weight) instead of weight.
"""
import numpy as np
import torch
import torch.nn.functional as F

from mulactseg_amd import synth

# the golden case (tests/golden/g15_online_plbl.npz): quarter-resolution maps 10 x 11 -> 40 x 44, both temperatures T
SEED, N, C, CH, H, W, HQ, WQ, S, T, TH = 15, 2, 20, 256, 40, 44, 10, 11, 48, 0.1, 0.5
P_COUNTS = (0.40, 0.35, 0.15, 0.10)         # raised multi-hot share: at least a third of the selected superpixels are multi-hot




def inputs(seed=SEED, n=N, c=C, ch=CH, h=H, w=W, hq=HQ, wq=WQ, s=S, frac=0.45, p_counts=P_COUNTS):
    """(zq_p, featq, zq, targets u8 [n,s,c], spx int64 [n,h,w], mask bool [n,h,w]) as numpy"""
    zq_p = synth.logits(seed, n, c, hq, wq)
    zq = synth.logits(seed + 1000, n, c, hq, wq)
    rs = np.random.RandomState(seed + 2000)
    f = rs.standard_normal((n, ch, hq, wq)).astype(np.float32)
    featq = F.normalize(torch.from_numpy(f), dim=1).numpy()
    spx, msk = [], []
    for i in range(n):
        a, b = synth.train_crop(seed * 17 + i, h, w, s, frac_selected=frac)
        spx.append(a)
        msk.append(b)
    tgt = np.stack([synth.multi_hot_targets(seed * 19 + i, s, c, p_counts=p_counts) for i in range(n)])
    return zq_p, featq, zq, tgt, np.stack(spx), np.stack(msk)


def upsample(q, size):
    return F.interpolate(torch.as_tensor(q), size=tuple(size), mode='bilinear', align_corners=False)


def upsample_f32(q, size):
    """The bilinear tap of csrc/upsample_tap.h in numpy float32, one rounding per operation: what the kernels compute, on every machine
    (ATen's vectorised CPU kernel may contract operations differently from one processor to the next)."""
    q = np.asarray(q, dtype=np.float32)
    f = np.float32

    def taps(n_in, n_out):
        s = f(n_in) / f(n_out) * (np.arange(n_out, dtype=np.float32) + f(0.5)) - f(0.5)
        s = np.maximum(s, f(0.0)).astype(np.float32)
        i0 = s.astype(np.int64)
        i1 = i0 + (i0 < n_in - 1)
        l1 = (s - i0.astype(np.float32)).astype(np.float32)
        return i0, i1, (f(1.0) - l1).astype(np.float32), l1

    y0, y1, ly0, ly1 = taps(q.shape[-2], size[0])
    x0, x1, lx0, lx1 = taps(q.shape[-1], size[1])
    top = lx0 * q[..., y0, :][..., x0] + lx1 * q[..., y0, :][..., x1]
    bot = lx0 * q[..., y1, :][..., x0] + lx1 * q[..., y1, :][..., x1]
    return torch.from_numpy((ly0[:, None] * top + ly1[:, None] * bot).astype(np.float32))


def generate(logits, feats, targets, spx, mask, temp, weight_wo_proto=False, near=0.0):
    """logits [N,C,H,W], feats [N,Ch,H,W], targets [N,S,C] (0/1), spx [N,H,W] ids, mask [N,H,W] bool -> (labels int64 [N,H,W] with
    255, weight f64 [N,H,W], gap f64 [N,H,W] (inf off the valid pixels)); with ``near`` > 0 a fourth value: bool [N,H,W], the pixels
    of superpixels in which some candidate's two largest DIFFERENT probabilities lie within ``near`` (relative) of each other -- there the
    choice of the prototype pixel itself depends on rounding"""
    # numpy float64 throughout, plain operations (no vectorised library softmax: identical pixels must give identical probabilities)
    logits, feats = np.asarray(logits, dtype=np.float64), np.asarray(feats, dtype=np.float64)
    targets, spx, mask = np.asarray(targets).astype(np.int64), np.asarray(spx).astype(np.int64), np.asarray(mask).astype(bool)
    N, C, H, W = logits.shape
    S = targets.shape[1]
    z = (logits / temp).reshape(N, C, -1)
    ez = np.exp(z - z.max(axis=1, keepdims=True))
    den = np.zeros((N, 1, H * W))
    for c in range(C):
        den[:, 0] += ez[:, c]
    prob = ez / den
    f = feats.reshape(N, feats.shape[1], -1)
    labels = np.full((N, H * W), 255, dtype=np.int64)
    weight = np.zeros((N, H * W))
    gap = np.full((N, H * W), np.inf)
    loose = np.zeros((N, H * W), dtype=bool)
    for n in range(N):
        ids, m = spx[n].reshape(-1), mask[n].reshape(-1)
        for s in range(S):
            cands = np.nonzero(targets[n, s, :C])[0].tolist()
            if int(targets[n, s].sum()) <= 1:
                continue
            px = np.nonzero(m & (ids == s))[0]
            if px.size == 0 or not cands:
                continue
            protos = []
            for c in cands:
                v = prob[n, c, px]
                protos.append(int(px[np.nonzero(v == v.max())[0][0]]))
                below = v[v < v.max()]              # (pixels that tie exactly read the same numbers: the lowest index, in any precision)
                if near and below.size and float(below.max()) >= (1.0 - near) * float(v.max()):
                    loose[n, px] = True
            sims = np.stack([(f[n][:, px] * f[n][:, [q]]).sum(axis=0) for q in protos], axis=1)        # [pixels, candidates]
            best = np.full(px.size, -np.inf)
            arg = np.zeros(px.size, dtype=np.int64)
            for j in range(len(cands)):
                better = sims[:, j] > best
                best = np.where(better, sims[:, j], best)
                arg = np.where(better, j, arg)
            pt = np.asarray(protos)
            other = pt[None, :] != pt[arg][:, None]                     # candidates whose prototype is another pixel
            second = np.where(other, sims, -np.inf).max(axis=1)
            lab = np.asarray(cands)[arg]
            labels[n, px] = lab
            weight[n, px] = prob[n][lab, px]
            gap[n, px] = best - second
            if weight_wo_proto:
                weight[n, pt] = 1.0
    out = tuple(torch.from_numpy(a.reshape(N, H, W)) for a in (labels, weight, gap))
    return out + (torch.from_numpy(loose.reshape(N, H, W)),) if near else out


def loss(kind, logits, labels, weight, temp, th=None):
    """(value, gradient with respect to ``logits``), both float64 numpy; ``logits`` [N,C,H,W] full resolution"""
    z = torch.as_tensor(logits).double().clone().requires_grad_(True)
    labels = torch.as_tensor(labels).long()
    ce = torch.nn.functional.cross_entropy(z / temp, labels, ignore_index=255, reduction='none')
    if kind == 'plain':
        n = int((labels != 255).sum())
        val = ce.sum() / n if n else ce.sum() * 0.0
    else:
        w = torch.as_tensor(weight).double()
        term = (w if th is None else (th < w).double()) * ce
        nz = term != 0
        if bool(nz.any()):
            val = term[nz].mean()
        else:
            val = term.sum() * (float('nan') if kind == 'joint' else 0.0)
    (g,) = torch.autograd.grad(val, z)
    return float(val), np.nan_to_num(g.numpy(), nan=0.0)


def quarter(n):
    """ops.quarter_size without importing the library"""
    return ((int(n) - 1) // 2) // 2 + 1


def edge_case(seed=7, c=20, ch=256, h=37, w=45, s=40):
    """Four pictures at a size that is no multiple of 4, from its quarter size: 0 = an ordinary crop; 1 = no selected pixel; 2 = selected
    pixels but only one-hot superpixels; 3 = hand-made: every superpixel selected and multi-hot except one whose ids are out of range
    (>= s) and unselected, one superpixel with all ``c`` bits, class channels 3 and 11 equal everywhere (so both classes share their
    prototype pixel wherever both are candidates, and superpixel ``pair`` has exactly those two), and logit peaks of two classes in the
    first and the last quarter-resolution cell, so a prototype is pixel 0, in the picture's border row and border column.  Returns a dict."""
    hq, wq = quarter(h), quarter(w)
    zq_p, featq, zq, tgt, spx, msk = inputs(seed, 4, c, ch, h, w, hq, wq, s)
    msk[1] = False
    tgt[2] = synth.multi_hot_targets(seed + 5, s, c, p_counts=(1.0,))
    ids = synth.superpixel_map(seed + 9, h, w, s)
    first, last = int(ids[0, 0]), int(ids[h - 1, w - 1])
    free = [k for k in range(s) if k not in (first, last)]
    gone, full, pair = free[0], free[1], free[2]
    t3 = synth.multi_hot_targets(seed + 6, s, c, p_counts=(0.0, 0.6, 0.3, 0.1))
    t3[full] = 1
    t3[pair] = 0
    t3[pair, [3, 11]] = 1
    t3[first, 5] = 1
    t3[last, 8] = 1
    zq_p[3, 11] = zq_p[3, 3]
    zq_p[3, 5, 0, 0] += 1.0
    zq_p[3, 8, hq - 1, wq - 1] += 1.0
    m3 = ids != gone
    ids = ids.copy()
    ids[~m3] = s + 5
    spx[3], msk[3], tgt[3] = ids, m3, t3
    return dict(zq_p=zq_p, featq=featq, zq=zq, tgt=tgt, spx=spx, msk=msk, size=(h, w), S=s, C=c, full=full, pair=pair, first=first, last=last)
