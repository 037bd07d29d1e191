"""numpy restatement of ``mas_ms_naive_plbl`` (mulactseg_amd/csrc/ms_naive.hip), written from its normative comment: the mean logits of
tests/ms_ensemble_restated.py (stage 1, the flip, stage 2, the sum in source order, / n), the first arg-max over the channels with
torch.max's NaN rule, and the tally of csrc/iou_tally.h without the "undefined" triple -- plus the reference's MeanIoU loop it
replaces (``utils/miou.py:23-38``)."""
import numpy as np

import ms_ensemble_restated as E
import lowres_iou_restated as L


def mean_logits(logits_q, sizes, flips, out_size):
    """f32 [C,H,W]: the sources' logits at the original size, summed in list order and divided by n."""
    H, W = out_size
    return E.mean(logits_q, sizes, flips, H, W)


def first_argmax(m):
    """int64 [H,W] of m [C,H,W]: the first maximum over the channels; a NaN wins where it first appears (torch.max; np.argmax agrees)."""
    return np.argmax(m, axis=0).astype(np.int64)


def labels(logits_q, sizes, flips, out_size):
    return first_argmax(mean_logits(logits_q, sizes, flips, out_size))


def counts(lab, targets, K, ignore_label):
    """int64 [3K+3]: seen / correct / positive per class over the pixels whose target is not ignore_label; the last three stay 0."""
    lab = np.asarray(lab, dtype=np.int64)
    return L.tally(lab, lab, targets, K, ignore_label, False)


def meaniou_loop(lab, targets, K, ignore_label):
    """The reference's ``MeanIoU._after_step`` (``utils/miou.py:23-38``): per class, numpy sums over the pixels kept; laid out as
    ``MeanIoU._counts`` (seen[K], correct[K], positive[K], three zeros)."""
    o, t = np.asarray(lab).reshape(-1), np.asarray(targets).reshape(-1)
    o, t = o[t != ignore_label], t[t != ignore_label]
    out = np.zeros(3 * K + 3, dtype=np.int64)
    for i in range(K):
        out[i] += np.sum(t == i)
        out[K + i] += np.sum((t == i) & (o == t))
        out[2 * K + i] += np.sum(o == i)
    return out
