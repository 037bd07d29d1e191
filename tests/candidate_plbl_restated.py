"""numpy restatement of csrc/candidate_plbl.hip and of k_stage2_assign_labels (csrc/stage2.hip), written from their normative
comments: one label per pixel from the (upsampled) logits, the mask and either the superpixel's candidate row or a label map, a
confidence-thresholded top-1 outside the mask, and MeanIoU's counters of the result."""
import numpy as np

import naive_plbl_restated as R

F32 = np.float32


def inv_temperature(T):
    """float32(1 / float32(T)), as the ABI forms it."""
    return F32(1.0) / F32(T)


def candidate_argmax(y, rows, spx):
    """int64 [N,H,W]: per pixel the first maximum over the channels of y_c * (float)row_c of the pixel's superpixel (the product taken
    literally: +-0 for an excluded channel, NaN for a NaN or an infinity times 0; the first NaN wins); 255 for an id outside the rows."""
    N, C, H, W = y.shape
    S = rows.shape[1]
    ok = (spx >= 0) & (spx < S)
    ids = np.clip(spx, 0, S - 1)
    lab = np.empty((N, H, W), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for n in range(N):
            mult = rows[n][ids[n]].astype(F32).transpose(2, 0, 1)          # [C,H,W] of 0.0 / 1.0
            lab[n] = np.argmax((y[n] * mult).astype(F32), axis=0)
    return np.where(ok, lab, 255)


def pmax(y, inv_T):
    """1 / sum_c exp((y_c - y_max) * inv_T), channel order from 0, in float32 (the kernel's expf is not numpy's exp); NaN for a NaN."""
    m = np.max(y, axis=1)
    s = np.zeros(m.shape, dtype=F32)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(y.shape[1]):
            s = (s + np.exp(((y[:, c] - m).astype(F32) * F32(inv_T)).astype(F32))).astype(F32)
        p = (F32(1) / s).astype(F32)
    p[np.isnan(y).any(axis=1)] = np.nan
    return p


def pmax64(y, inv_T=1.0):
    """The same quantity in float64 (for "away from the threshold")."""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return 1.0 / np.exp((y - y.max(axis=1, keepdims=True)) * float(inv_T)).sum(axis=1)


def labels(zq, H, W, mask, rows=None, spx=None, inner=None, fallback=False, th=0.0, inv_T=1.0):
    """int64 [N,H,W].  Under the mask: candidate_argmax (rows u8 [N,S,C] with spx int64 [N,H,W]) or inner narrowed to u8; outside it
    255, or with the fallback the first arg-max where pmax > th."""
    assert (rows is None) == (spx is None) and (rows is None) != (inner is None)
    y = R.upsample(zq, H, W)
    mask = np.asarray(mask).astype(bool)
    if inner is not None:
        under = np.asarray(inner).astype(np.uint8).astype(np.int64)
    else:
        under = candidate_argmax(y, np.asarray(rows), np.asarray(spx))
    out = np.full(mask.shape, 255, dtype=np.int64)
    if fallback:
        with np.errstate(invalid='ignore'):
            keep = pmax(y, inv_T) > F32(th)
        out = np.where(keep, R.first_argmax(y).astype(np.int64), out)
    return np.where(mask, under, out)


def meaniou_counts(lab, targets, K, ignore_label=255):
    """int64 [3K+3]: MeanIoU(K, ignore_label)._after_step -- seen, correct, positive per class over the targets that are not ignored;
    the last three stay 0."""
    lab, targets = np.asarray(lab).reshape(-1), np.asarray(targets).reshape(-1)
    keep = targets != ignore_label
    o, t = lab[keep], targets[keep]
    c = np.zeros(3 * K + 3, dtype=np.int64)
    for i in range(K):
        c[i] = np.sum(t == i)
        c[K + i] = np.sum((t == i) & (o == t))
        c[2 * K + i] = np.sum(o == i)
    return c


def iou_table(counts, K):
    """The table string the generators print: MeanIoU._after_epoch's IoUs in percent (utils/miou.py:63-70: correct / (seen + positive -
    correct) * 100, an unseen class counts as 100), their mean first, '%.2f' each."""
    c = np.asarray(counts, dtype=np.float64)
    ious = [100.0 if c[i] == 0 else c[K + i] / (c[i] + c[2 * K + i] - c[K + i]) * 100 for i in range(K)]
    return ','.join(['%.2f' % np.mean(ious)] + ['%.2f' % v for v in ious])


def assign_labels(nn, p_cls):
    """k_stage2_assign_labels: p_cls[nn] where nn >= 0, 255 elsewhere."""
    nn, p_cls = np.asarray(nn), np.asarray(p_cls)
    return np.where(nn >= 0, p_cls[np.maximum(nn, 0)], 255).astype(np.int64)
