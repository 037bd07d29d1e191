"""numpy restatement of ``mas_ms_iou_counts`` (mulactseg_amd/csrc/ms_naive.hip, evaluation mode), written from its normative comment:
the mean logits of tests/ms_naive_restated.py (stage 1, the flip, stage 2, the sum in source order, / n), the two first arg-maxes with
torch.max's NaN rule, and the counters as the per-class ``sum(==)`` loops of the reference's meters (``utils/miou.py:23-38`` for
``MeanIoU``, ``utils/miou_evalignore.py:20-32`` for ``IoUIgnore``) -- plus the inputs the GPU cases share."""
import numpy as np

import ms_ensemble_restated as E
import ms_naive_restated as N


def argmaxes(m, K):
    """(o_cls, o_all) int64 [H,W] of the mean logits m [CH,H,W]: the first arg-max over the channels [0, K) and over all CH."""
    return N.first_argmax(m[:K]), N.first_argmax(m)


def counts_of(o_cls, o_all, targets, K, ignore_label, with_undefined):
    """int64 [3K+3] in the layout of ``MeanIoU._counts``: seen[K], correct[K], positive[K] over the pixels whose target is not
    ignore_label; then (seen, correct, positive) of the "undefined" class over every pixel when with_undefined, zeros otherwise."""
    o, oa, t = np.asarray(o_cls).reshape(-1), np.asarray(o_all).reshape(-1), np.asarray(targets).reshape(-1)
    out = np.zeros(3 * K + 3, dtype=np.int64)
    ok, tk = o[t != ignore_label], t[t != ignore_label]
    for i in range(K):
        out[i] = np.sum(tk == i)
        out[K + i] = np.sum((tk == i) & (ok == tk))
        out[2 * K + i] = np.sum(ok == i)
    if with_undefined:
        out[3 * K] = np.sum(t == ignore_label)
        out[3 * K + 1] = np.sum((t == ignore_label) & (oa == K))
        out[3 * K + 2] = np.sum(oa == K)
    return out


def counts_from_mean(m, targets, K, ignore_label):
    """The counters of mean logits m [CH,H,W] (CH = K or K + 1) against targets [H,W]."""
    o_cls, o_all = argmaxes(m, K)
    return counts_of(o_cls, o_all, targets, K, ignore_label, m.shape[0] > K)


def ms_iou_counts(logits_q, sizes, flips, out_size, targets, K, ignore_label):
    """-> (counts int64 [3K+3], o_cls int64 [H,W], o_all, m f32 [CH,H,W])."""
    m = N.mean_logits(logits_q, sizes, flips, out_size)
    o_cls, o_all = argmaxes(m, K)
    return counts_of(o_cls, o_all, targets, K, ignore_label, m.shape[0] > K), o_cls, o_all, m


# -- the sources and inputs of the GPU cases ------------------------------------------------------------------------------------------
def sources(kind, H, W):
    """(sizes, flips): 'one' = the picture itself; 'two' = the picture and a flipped three-quarter copy; 'ten' = the default
    TestTimeAugmentation list; 'big' = factors (1.0, 1.75, 2.0) and their flips (the largest LDS extents)."""
    if kind == 'one':
        return [(H, W)], [False]
    if kind == 'two':
        return [(H, W), (int(0.75 * H), int(0.75 * W))], [False, True]
    if kind == 'ten':
        return E.tta_sizes(H, W)
    if kind == 'big':
        return E.tta_sizes(H, W, factors=(1.0, 1.75, 2.0))
    raise ValueError(kind)


def make_case(seed, sizes, H, W, CH, K):
    """Quarter-resolution logits per source and targets [H,W] that exercise both arg-maxes: seeded noise; channels 2 and 4 equal in
    every source and above the rest in the top third (exact ties at the maximum); with CH = K + 1, channel K above the rest in the
    middle third (o_all leaves o_cls); one NaN in a class channel and one in the last channel of the finest source;
    targets with 255, values above K - 1 and -1."""
    rs = np.random.RandomState(seed)
    lq = []
    for Hs, Ws in sizes:
        hq, wq = E.quarter_size(Hs), E.quarter_size(Ws)
        z = rs.uniform(-1, 1, (CH, hq, wq)).astype(np.float32)
        top, mid = max(1, hq // 3), max(2, (2 * hq) // 3)
        z[2, :top] += 4.0
        z[4] = z[2]
        if CH > K:
            z[K, top:mid] += 4.0
        lq.append(z)
    big = lq[int(np.argmax([z.shape[1] * z.shape[2] for z in lq]))]      # (a NaN spreads over its taps: the finest map keeps it local)
    big[5, -1, big.shape[2] // 2] = np.nan
    big[CH - 1, -1, 0] = np.nan
    t = rs.randint(0, K, size=(H, W)).astype(np.int64)
    t[rs.uniform(size=t.shape) < 0.15] = 255
    t[rs.uniform(size=t.shape) < 0.05] = K + 3
    t[rs.uniform(size=t.shape) < 0.03] = -1
    return lq, t


def exercised(m, o_cls, o_all, cnt, targets, K):
    """The conditions a case must meet before it is compared (None when it does; otherwise what is missing)."""
    CH = m.shape[0]
    cls_max = np.fmax.reduce(m[:K], axis=0)
    if not np.any((m[2] == m[4]) & (m[2] == cls_max)):
        return "no exact tie at the class maximum"
    if not np.isnan(m).any():
        return "no NaN"
    if not np.any(targets == 255) or not np.any((targets != 255) & ((targets < 0) | (targets >= K))):
        return "targets lack 255 or out-of-range values"
    if CH > K:
        if not np.any(o_cls != o_all):
            return "o_cls == o_all everywhere"
        if not np.all(cnt[3 * K:] > 0):
            return "an 'undefined' counter is zero: %s" % cnt[3 * K:].tolist()
    elif np.any(cnt[3 * K:]) or np.any(o_cls != o_all):
        return "CH == K must leave the 'undefined' triple alone"
    return None
