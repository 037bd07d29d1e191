"""numpy restatement of the evaluation counters of csrc/lowres_iou.hip, written from its normative comment: the upsampling of
tests/naive_plbl_restated.py, the two arg-maxes of k_logits_iou (csrc/metrics.hip) and the tally of csrc/iou_tally.h."""
import numpy as np

import naive_plbl_restated as R


def argmaxes(z, C):
    """(o_cls, o_all) int64 [N,H,W] of z [N,CH,H,W]: o_cls starts at channel 0 and moves to c < C only when z_c > best (the first
    maximum wins; a NaN never moves it); o_all is C when CH = C + 1 and z_C > best, o_cls otherwise."""
    best = z[:, 0].copy()
    o_cls = np.zeros(best.shape, dtype=np.int64)
    for c in range(1, C):
        up = z[:, c] > best
        best = np.where(up, z[:, c], best)
        o_cls[up] = c
    o_all = o_cls.copy()
    if z.shape[1] > C:
        o_all[z[:, C] > best] = C
    return o_cls, o_all


def tally(o_cls, o_all, targets, C, ignore_label, with_ignore):
    """int64 [3C+3]: seen / correct / positive per class over the pixels whose target is not ignore_label (a target outside [0, C)
    counts no "seen", its prediction still counts "positive"), then those of the "undefined" class when with_ignore."""
    t = np.asarray(targets, dtype=np.int64).reshape(-1)
    o, oa = o_cls.reshape(-1), o_all.reshape(-1)
    keep = t != ignore_label
    out = np.zeros(3 * C + 3, dtype=np.int64)
    for c in range(C):
        out[c] = np.sum(keep & (t == c))
        out[C + c] = np.sum(keep & (t == c) & (o == c))
        out[2 * C + c] = np.sum(keep & (o == c))
    if with_ignore:
        tig, oig = t == ignore_label, oa == C
        out[3 * C:] = [np.sum(tig), np.sum(tig & oig), np.sum(oig)]
    return out


def lowres_iou_counts(zq, targets, H, W, C, ignore_label):
    """The counters of quarter-resolution logits zq f32 [N,CH,h,w] against targets [N,H,W] (CH = C or C + 1)."""
    z = R.upsample(zq, H, W)
    o_cls, o_all = argmaxes(z, C)
    return tally(o_cls, o_all, targets, C, ignore_label, z.shape[1] > C)
