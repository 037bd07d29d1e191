// iou_tally.h -- one pixel's contribution to the mIoU counters (metrics.hip, lowres_iou.hip), counted into per-workgroup LDS
// histograms that the caller flushes with one 64-bit global atomic per non-zero counter.
//
// counts layout: seen[C], correct[C], positive[C], then (ignore_seen, ignore_correct, ignore_positive).
// Reference: utils/miou.py:23-38 (MeanIoU._after_step: a target equal to ignore_label counts nowhere; a target outside [0, C)
// counts no "seen", its prediction still counts "positive") and utils/miou_evalignore.py:20-32 (IoUIgnore over every pixel).
#pragma once

__device__ __forceinline__ void tally(unsigned* s_cnt, int C, long long t, long long o_cls, long long o_all, long long ignore_label,
                                      bool with_ignore_iou) {
    if (t != ignore_label) {
        if (t >= 0 && t < C) {
            atomicAdd(&s_cnt[t], 1u);
            if (o_cls == t) atomicAdd(&s_cnt[C + t], 1u);
        }
        if (o_cls >= 0 && o_cls < C) atomicAdd(&s_cnt[2 * C + o_cls], 1u);
    }
    if (with_ignore_iou) {
        const bool tig = (t == ignore_label), oig = (o_all == C);
        if (tig) atomicAdd(&s_cnt[3 * C], 1u);
        if (tig && oig) atomicAdd(&s_cnt[3 * C + 1], 1u);
        if (oig) atomicAdd(&s_cnt[3 * C + 2], 1u);
    }
}
