// ms_naive.hip -- naive arg-max pseudo labels of the VOC generators (single-scale and multi-scale + flip) and their IoU counters, in
// one launch per picture from the network's quarter-resolution logits (mas_ms_naive_plbl); and, from the same sources and the same mean
// logits, the counters of the evaluation loop (mas_ms_iou_counts: multi-scale + flip evaluation of a checkpoint, eval_naive_ms).
//
// Reference: trainer/eval_save_cosplbl_naive_voc.py:54-67 and trainer/eval_save_cosplbl_naive_voc_ms.py:55-92.  Every source k (the
// picture itself, or one of the ten TestTimeAugmentation copies) went through feat_forward (logits upsampled x4 to the scaled size
// (Hs, Ws)), was flipped back, resized to the original (H, W), averaged over the sources; label = outputs.max(dim=1)[1] over all C
// channels, then MeanIoU(K, ignore)._after_step(label, targets).  Materialised that is C channels at every scaled size and again at
// the original size per source; here the scaled-size values live in LDS and the mean logits in registers, one channel block at a time.
//
// Arithmetic (normative; tests/ms_naive_restated.py restates it in numpy).  Per channel and output pixel, source k's value is that of
// k_ms_ensemble (ms_ensemble.hip) for its logits:
//   1. stage 1, quarter (hq, wq) -> scaled (Hs, Ws), the tap and expression of k_upsample_fwd (upsample_tap.h);
//   2. flip: stage-2 taps in flipped coordinates, stage-1 column j read as column Ws-1-j;
//   3. stage 2, scaled -> original (H, W), the same tap and expression;
//   4. acc = v_0 + v_1 + ... + v_{n-1} in source order, m = acc / (float)n.
//   5. label: the first arg-max of m over the channels in channel order (strict '>'; a NaN takes the place and keeps it: torch.max;
//      arg_update of upsample_tap.h).  The comparison is on m, not on acc: the division can make two sums equal.
//   6. counters: tally() of iou_tally.h with K = num_classes, no "undefined" triple, into per-workgroup LDS u32 counters; one 64-bit
//      global atomic per non-zero counter, added to the caller's buffer.  Integer sums: deterministic.
// So labels == torch.max(mas_ms_ensemble's logits, 1)[1] for any input, and with n = 1 and the geometry (hq, wq, H, W, 0) labels ==
// torch.max(mas_upsample_bilinear_fwd(z_q, H, W), 1)[1].
//
// Evaluation mode (k_ms_naive<true>, mas_ms_iou_counts; tests/ms_eval_restated.py restates it).  Steps 1-4 unchanged; C = K or K + 1
// channels with K = num_classes (the stage-2 model of eval_naive carries one "undefined" channel):
//   5'. o_cls = the first arg-max of m over the channels [0, K), o_all = the first arg-max over all C channels, both with the rule of
//       step 5.  One walk: channel K moves o_all away from o_cls exactly when arg_update would move the arg-max.
//   6'. tally(K, t, o_cls, o_all, ignore_label, C == K + 1): the MeanIoU(K) triples and, with the extra channel, the "undefined" triple
//       of IoUIgnore (reference trainer/eval_naive.py:61-63 applied to the mean logits).  pred (optional) receives o_cls.
//
// Shape: the two-stage tile of ms_tile.h, the tiling of k_ms_ensemble.  After the last source of a channel block the mean updates the
// running arg-max, kept in registers across the blocks.  The thread's int64 target is loaded before the channel walk, so its latency
// hides behind it.
#include "common.h"
#include "iou_tally.h"
#include "ms_tile.h"

namespace {
constexpr int kMaxCnt = 3 * (MAS_MAX_CLASSES + 1);
constexpr size_t kStaticLds = sizeof(unsigned) * kMaxCnt;

struct NvArgs {
    MsTile t;
    const float* logit[MAS_MS_MAX_SOURCES];   // [C, hq, wq] per source
    const long long* tgt;         // [H, W] or NULL (no counters)
    unsigned char* labels;        // [H, W]; evaluation mode: o_cls, or NULL
    mas_u64* counts;              // [3K+3] or NULL (evaluation mode: never NULL)
    long long ignore_label;
    int C, K;
};

// grid: ms_tile_grid; dynamic LDS: ms_tile_extents.  kEval: the two arg-maxes and the tally of the evaluation loop instead of the one
// arg-max of the pseudo labels; the mean is the same code.
template <bool kEval>
__global__ __launch_bounds__(kThreads) void k_ms_naive(const NvArgs a) {
    extern __shared__ float lds[];
    __shared__ unsigned s_cnt[kMaxCnt];
    const int tid = threadIdx.x, C = a.C;
    const MsPixel p = ms_tile_pixel(a.t);
    const size_t pix = (size_t)p.cy * a.t.W + p.cx;
    const bool counting = a.counts != nullptr;
    const long long t = counting && p.live ? a.tgt[pix] : 0;
    if (counting)
        for (int i = tid; i < 3 * a.K + 3; i += kThreads) s_cnt[i] = 0;   // (the first barrier below orders it before the tally)
    float best = 0.0f;
    int idx = 0;
    bool all_is_k = false;                               // (kEval) channel K holds the arg-max over all channels
    for (int ch0 = 0; ch0 < C; ch0 += kCB) {
        const int nb = min(kCB, C - ch0);
        float acc[kCB];
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) acc[cb] = 0.0f;
        for (int k = 0; k < a.t.n; ++k) {
            const size_t qplane = (size_t)a.t.src[k].hq * a.t.src[k].wq;
            const float* q = a.logit[k] + (size_t)ch0 * qplane;
            if (!ms_tile_add(a.t, k, p, nb, [=](int cb) { return q + (size_t)cb * qplane; }, lds, acc)) return;
        }
        const float fn = (float)a.t.n;
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
            if (cb < nb) {
                const float m = acc[cb] / fn;
                if (ch0 + cb == 0) best = m;
                else if (!kEval || ch0 + cb < a.K) arg_update(m, ch0 + cb, best, idx);
                else all_is_k = best == best && (m > best || m != m);   // (C == K + 1: the last channel; arg_update's rule)
            }
        }
    }
    if (p.live && (!kEval || a.labels)) a.labels[pix] = (unsigned char)idx;
    if (!counting) return;
    if (p.live) tally(s_cnt, a.K, t, idx, kEval && all_is_k ? a.K : idx, a.ignore_label, kEval && C > a.K);
    __syncthreads();
    for (int i = tid; i < 3 * a.K + 3; i += kThreads)
        if (s_cnt[i]) atomicAdd(&a.counts[i], (mas_u64)s_cnt[i]);
}

// Fills the sources and the LDS extents of `a` from the caller's tables and launches the kernel; both entry points refuse the same
// geometries (ms_tile_sources) and a tile whose buffers and counters together exceed the LDS of a workgroup.
template <bool kEval>
int launch(NvArgs& a, const float* const* logits_q, const int32_t* geometry, int n, int H, int W, void* stream) {
    for (int k = 0; k < n; ++k) {
        if (!logits_q[k]) return MAS_ERR_NULL;
        a.logit[k] = logits_q[k];
    }
    if (int st = ms_tile_sources(a.t, geometry, n, H, W)) return st;
    const size_t lds = ms_tile_extents(a.t);
    if (lds + kStaticLds > kMaxLds) return MAS_ERR_RANGE;
    hipLaunchKernelGGL(k_ms_naive<kEval>, ms_tile_grid(a.t), dim3(kThreads), lds, static_cast<hipStream_t>(stream), a);
    return mas_launch_status();
}
}  // namespace

extern "C" int mas_ms_naive_plbl(const float* const* logits_q, const int32_t* geometry, int n, int C, int H, int W, const int64_t* targets,
                                 int num_classes, int64_t ignore_label, uint8_t* labels, uint64_t* counts, void* stream) {
    if (!logits_q || !geometry || !labels || (counts && !targets)) return MAS_ERR_NULL;
    if (n < 1 || n > MAS_MS_MAX_SOURCES) return MAS_ERR_RANGE;
    if (C < 1 || C > 255) return MAS_ERR_CLASSES;
    if (counts && (num_classes < C || num_classes > MAS_MAX_CLASSES)) return MAS_ERR_CLASSES;
    if (H < 1 || W < 1 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    NvArgs a = {};
    a.tgt = counts ? reinterpret_cast<const long long*>(targets) : nullptr;
    a.labels = labels;
    a.counts = reinterpret_cast<mas_u64*>(counts);
    a.ignore_label = (long long)ignore_label;
    a.C = C, a.K = counts ? num_classes : 0;
    return launch<false>(a, logits_q, geometry, n, H, W, stream);
}

extern "C" int mas_ms_iou_counts(const float* const* logits_q, const int32_t* geometry, int n, int CH, int H, int W, const int64_t* targets,
                                 int num_classes, int64_t ignore_label, uint64_t* counts, uint8_t* pred, void* stream) {
    if (!logits_q || !geometry || !targets || !counts) return MAS_ERR_NULL;
    if (n < 1 || n > MAS_MS_MAX_SOURCES) return MAS_ERR_RANGE;
    if (num_classes < 1 || num_classes > MAS_MAX_CLASSES || (CH != num_classes && CH != num_classes + 1)) return MAS_ERR_CLASSES;
    if (H < 1 || W < 1 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    NvArgs a = {};
    a.tgt = reinterpret_cast<const long long*>(targets);
    a.labels = pred;
    a.counts = reinterpret_cast<mas_u64*>(counts);
    a.ignore_label = (long long)ignore_label;
    a.C = CH, a.K = num_classes;
    return launch<true>(a, logits_q, geometry, n, H, W, stream);
}

extern "C" int64_t mas_ms_iou_lds_bytes(const int32_t* geometry, int n, int H, int W) {
    if (!geometry) return MAS_ERR_NULL;
    if (n < 1 || n > MAS_MS_MAX_SOURCES) return MAS_ERR_RANGE;
    if (H < 1 || W < 1 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    MsTile t;
    if (int st = ms_tile_sources(t, geometry, n, H, W)) return st;
    return (int64_t)(ms_tile_extents(t) + kStaticLds);
}
