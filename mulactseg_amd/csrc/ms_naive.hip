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
//      the rule of naive_plbl.hip).  The comparison is on m, not on acc: the division can make two sums equal.
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
// Shape: the tiling of k_ms_ensemble.  A workgroup owns an 8 x 32 output tile, one pixel per thread, and walks the channels in blocks
// of kCB, sources innermost; per (block, source):
//   A. every (quarter row, stage-1 column) position the tile needs, lerped horizontally for the block's channels into LDS.  A thread
//      issues the loads of all its positions and channels first and stores to LDS after, so a step waits on one round of load
//      latency rather than on one per value;
//   B. the stage-1 rows the tile needs, combined vertically from A, into LDS;
//   C. stage 2 for the thread's pixel, accumulated in registers.
// After the last source of a block the mean updates the running arg-max, kept in registers across the blocks.  The thread's int64
// target is loaded before the channel walk, so its latency hides behind it.  LDS extents are the exact maxima over tiles and sources,
// computed on the host with the kernel's tap arithmetic.
#include "common.h"
#include "iou_tally.h"
#include "upsample_tap.h"

namespace {
constexpr int kTH = 8, kTW = 32;           // output tile
constexpr int kThreads = kTH * kTW;        // one output pixel per thread
constexpr int kCB = 8;                     // channels per LDS block
constexpr int kPos = 2;                    // (quarter row, stage-1 column) positions per thread and load round in A
constexpr int kWaves = kThreads / MAS_WAVE;
constexpr size_t kMaxLds = 64 * 1024;      // of one workgroup: the dynamic buffers and the static counters together
constexpr int kMaxCnt = 3 * (MAS_MAX_CLASSES + 1);
constexpr size_t kStaticLds = sizeof(unsigned) * kMaxCnt;

struct NvSrc {
    const float* logit;           // [C, hq, wq]
    int hq, wq, hs, ws, flip;
    float s1h, s1w, s2h, s2w;     // stage-1 (quarter -> scaled) and stage-2 (scaled -> original) scales
};

struct NvArgs {
    NvSrc src[MAS_MS_MAX_SOURCES];
    const long long* t;           // [H, W] or NULL (no counters)
    unsigned char* labels;        // [H, W]; evaluation mode: o_cls, or NULL
    mas_u64* counts;              // [3K+3] or NULL (evaluation mode: never NULL)
    long long ignore_label;
    int n, C, K, H, W;
    int nrq, nr1, nc1;            // LDS extents: quarter rows, stage-1 rows, stage-1 columns of one tile
};

// stage-1 row range [r_lo, r_hi] and quarter row range [q_lo, q_hi] of output rows y0..y1 (unflipped axis)
__host__ __device__ __forceinline__ void row_span(const NvSrc& s, int y0, int y1, int& r_lo, int& r_hi, int& q_lo, int& q_hi) {
    r_lo = make_tap(s.s2h, y0, s.hs).i0;
    r_hi = make_tap(s.s2h, y1, s.hs).i1;
    q_lo = make_tap(s.s1h, r_lo, s.hq).i0;
    q_hi = make_tap(s.s1h, r_hi, s.hq).i1;
}

// stage-1 column range [c_lo, c_hi] (unflipped stage-1 coordinates) of output columns x0..x1
__host__ __device__ __forceinline__ void col_span(const NvSrc& s, int x0, int x1, int& c_lo, int& c_hi) {
    const int b_lo = make_tap(s.s2w, x0, s.ws).i0, b_hi = make_tap(s.s2w, x1, s.ws).i1;
    c_lo = s.flip ? s.ws - 1 - b_hi : b_lo;
    c_hi = s.flip ? s.ws - 1 - b_lo : b_hi;
}

// first maximum wins; a NaN replaces a number and is never replaced (torch.max; naive_plbl.hip)
__device__ __forceinline__ void arg_update(float v, int c, float& best, int& idx) {
    if (best != best) return;
    if (v > best || v != v) {
        best = v;
        idx = c;
    }
}

// grid: (ceil(W / kTW), ceil(H / kTH)); dynamic LDS: kCB * (nrq + nr1) * nc1 floats.  kEval: the two arg-maxes and the tally of the
// evaluation loop instead of the one arg-max of the pseudo labels; staging and stage 2 are the same code.
template <bool kEval>
__global__ __launch_bounds__(kThreads) void k_ms_naive(const NvArgs a) {
    extern __shared__ float lds[];
    __shared__ unsigned s_cnt[kMaxCnt];
    float* hbuf = lds;                                   // [kCB][nrq][nc1]: quarter rows lerped horizontally
    float* sbuf = lds + kCB * a.nrq * a.nc1;             // [kCB][nr1][nc1]: stage-1 values
    const int tid = threadIdx.x, lane = tid & (MAS_WAVE - 1), wave = tid / MAS_WAVE;
    const int H = a.H, W = a.W, C = a.C;
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    const int y1 = min(y0 + kTH, H) - 1, x1 = min(x0 + kTW, W) - 1;
    const int py = y0 + tid / kTW, px = x0 + tid % kTW;
    const bool live = py < H && px < W;
    const int cy = min(py, y1), cx = min(px, x1);        // taps of a pixel outside the picture: those of the tile's last one
    const size_t pix = (size_t)cy * W + cx;
    const bool counting = a.counts != nullptr;
    const long long t = counting && live ? a.t[pix] : 0;
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
        for (int k = 0; k < a.n; ++k) {
            const NvSrc& s = a.src[k];
            int r_lo, r_hi, q_lo, q_hi, c_lo, c_hi;
            row_span(s, y0, y1, r_lo, r_hi, q_lo, q_hi);
            col_span(s, x0, x1, c_lo, c_hi);
            const int nq = q_hi - q_lo + 1, nr = r_hi - r_lo + 1, nc = c_hi - c_lo + 1;
            if (nq > a.nrq || nr > a.nr1 || nc > a.nc1) return;   // (uniform over the workgroup; the host sized these -- never taken)
            const size_t qplane = (size_t)s.hq * s.wq;
            const float* q = s.logit + (size_t)ch0 * qplane;
            // A: horizontal lerp of the quarter rows, once per needed stage-1 column; loads of a round first, LDS stores after
            const int npos = nq * nc;
            for (int p0 = 0; p0 < npos; p0 += kPos * kThreads) {
                float v0[kPos][kCB], v1[kPos][kCB], w0[kPos], w1[kPos];
                int dst[kPos];
#pragma unroll
                for (int u = 0; u < kPos; ++u) {
                    const int p = p0 + u * kThreads + tid;
                    dst[u] = -1;
                    w0[u] = w1[u] = 0.0f;
                    if (p < npos) {
                        const int r = p / nc, c = p - r * nc;
                        const Tap tc = make_tap(s.s1w, c_lo + c, s.wq);
                        const float* row = q + (size_t)(q_lo + r) * s.wq;
                        dst[u] = r * a.nc1 + c;
                        w0[u] = tc.l0, w1[u] = tc.l1;
#pragma unroll
                        for (int cb = 0; cb < kCB; ++cb) {
                            if (cb < nb) {
                                v0[u][cb] = row[(size_t)cb * qplane + tc.i0];
                                v1[u][cb] = row[(size_t)cb * qplane + tc.i1];
                            }
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < kPos; ++u) {
                    if (dst[u] >= 0) {
#pragma unroll
                        for (int cb = 0; cb < kCB; ++cb)
                            if (cb < nb) hbuf[cb * a.nrq * a.nc1 + dst[u]] = w0[u] * v0[u][cb] + w1[u] * v1[u][cb];
                    }
                }
            }
            __syncthreads();
            // B: vertical combination into the stage-1 values the tile needs
            for (int r = wave; r < nr; r += kWaves) {
                const Tap tr = make_tap(s.s1h, r_lo + r, s.hq);
                const int h0 = tr.i0 - q_lo, h1 = tr.i1 - q_lo;
                for (int cb = 0; cb < nb; ++cb) {
                    const float* hb = hbuf + cb * a.nrq * a.nc1;
                    float* sb = sbuf + (cb * a.nr1 + r) * a.nc1;
                    for (int c = lane; c < nc; c += MAS_WAVE) sb[c] = tr.l0 * hb[h0 * a.nc1 + c] + tr.l1 * hb[h1 * a.nc1 + c];
                }
            }
            __syncthreads();
            // C: stage 2 for this thread's pixel (flipped sources: taps in flipped coordinates, column j read as Ws-1-j)
            const Tap ty = make_tap(s.s2h, cy, s.hs), tx = make_tap(s.s2w, cx, s.ws);
            const int r0 = ty.i0 - r_lo, r1 = ty.i1 - r_lo;
            const int c0 = (s.flip ? s.ws - 1 - tx.i0 : tx.i0) - c_lo, c1 = (s.flip ? s.ws - 1 - tx.i1 : tx.i1) - c_lo;
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb) {
                if (cb < nb) {
                    const float* sb = sbuf + cb * a.nr1 * a.nc1;
                    const float v = ty.l0 * (tx.l0 * sb[r0 * a.nc1 + c0] + tx.l1 * sb[r0 * a.nc1 + c1]) +
                                    ty.l1 * (tx.l0 * sb[r1 * a.nc1 + c0] + tx.l1 * sb[r1 * a.nc1 + c1]);
                    acc[cb] = k == 0 ? v : acc[cb] + v;
                }
            }
            // (no barrier here: the next A writes hbuf, which every thread finished reading before the barrier above; the next B
            // writes sbuf only after the barrier that follows the next A, which every thread reaches after its C)
        }
        const float fn = (float)a.n;
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
    if (live && (!kEval || a.labels)) a.labels[pix] = (unsigned char)idx;
    if (!counting) return;
    if (live) tally(s_cnt, a.K, t, idx, kEval && all_is_k ? a.K : idx, a.ignore_label, kEval && C > a.K);
    __syncthreads();
    for (int i = tid; i < 3 * a.K + 3; i += kThreads)
        if (s_cnt[i]) atomicAdd(&a.counts[i], (mas_u64)s_cnt[i]);
}

// The sources of a.n, a.H, a.W from the caller's tables and the LDS extents of one tile: the exact maxima over tiles and sources (same
// tap arithmetic as the kernel).  logits_q == NULL: geometry only (mas_ms_iou_lds_bytes).  *lds: the dynamic LDS of the launch.
static int set_sources(NvArgs& a, const float* const* logits_q, const int32_t* geometry, size_t* lds) {
    const int n = a.n, H = a.H, W = a.W;
    for (int k = 0; k < MAS_MS_MAX_SOURCES; ++k) a.src[k] = NvSrc{};
    for (int k = 0; k < n; ++k) {
        const int32_t* g = geometry + 5 * k;
        NvSrc& s = a.src[k];
        if (logits_q) {
            if (!logits_q[k]) return MAS_ERR_NULL;
            s.logit = logits_q[k];
        }
        s.hq = g[0], s.wq = g[1], s.hs = g[2], s.ws = g[3], s.flip = g[4] != 0;
        // stage 1 is an upsampling (the network's x4); the scaled picture is not empty (the rules of mas_ms_ensemble)
        if (s.hq < 1 || s.wq < 1 || s.hs < 1 || s.ws < 1 || s.hq > s.hs || s.wq > s.ws) return MAS_ERR_SHAPE;
        s.s1h = (float)s.hq / (float)s.hs, s.s1w = (float)s.wq / (float)s.ws;
        s.s2h = (float)s.hs / (float)H, s.s2w = (float)s.ws / (float)W;
    }
    int nrq = 1, nr1 = 1, nc1 = 1;
    for (int k = 0; k < n; ++k) {
        const NvSrc& s = a.src[k];
        for (int y0 = 0; y0 < H; y0 += kTH) {
            int r_lo, r_hi, q_lo, q_hi;
            row_span(s, y0, (y0 + kTH < H ? y0 + kTH : H) - 1, r_lo, r_hi, q_lo, q_hi);
            nr1 = r_hi - r_lo + 1 > nr1 ? r_hi - r_lo + 1 : nr1;
            nrq = q_hi - q_lo + 1 > nrq ? q_hi - q_lo + 1 : nrq;
        }
        for (int x0 = 0; x0 < W; x0 += kTW) {
            int c_lo, c_hi;
            col_span(s, x0, (x0 + kTW < W ? x0 + kTW : W) - 1, c_lo, c_hi);
            nc1 = c_hi - c_lo + 1 > nc1 ? c_hi - c_lo + 1 : nc1;
        }
    }
    a.nrq = nrq, a.nr1 = nr1, a.nc1 = nc1;
    *lds = sizeof(float) * kCB * (size_t)(nrq + nr1) * nc1;
    // a stage-2 downsample beyond what one tile's LDS holds (x2, the largest factor of an evaluation, fits; the VOC factors stop at 1.5)
    return *lds + kStaticLds > kMaxLds ? MAS_ERR_RANGE : 0;
}
}  // namespace

extern "C" int mas_ms_naive_plbl(const float* const* logits_q, const int32_t* geometry, int n, int C, int H, int W, const int64_t* targets,
                                 int num_classes, int64_t ignore_label, uint8_t* labels, uint64_t* counts, void* stream) {
    if (!logits_q || !geometry || !labels || (counts && !targets)) return MAS_ERR_NULL;
    if (n < 1 || n > MAS_MS_MAX_SOURCES) return MAS_ERR_RANGE;
    if (C < 1 || C > 255) return MAS_ERR_CLASSES;
    if (counts && (num_classes < C || num_classes > MAS_MAX_CLASSES)) return MAS_ERR_CLASSES;
    if (H < 1 || W < 1 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    NvArgs a;
    a.t = counts ? reinterpret_cast<const long long*>(targets) : nullptr;
    a.labels = labels;
    a.counts = reinterpret_cast<mas_u64*>(counts);
    a.ignore_label = (long long)ignore_label;
    a.n = n, a.C = C, a.K = counts ? num_classes : 0, a.H = H, a.W = W;
    size_t lds;
    const int st = set_sources(a, logits_q, geometry, &lds);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_ms_naive<false>, dim3((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH)), dim3(kThreads), lds,
                       static_cast<hipStream_t>(stream), a);
    return mas_launch_status();
}

extern "C" int mas_ms_iou_counts(const float* const* logits_q, const int32_t* geometry, int n, int CH, int H, int W, const int64_t* targets,
                                 int num_classes, int64_t ignore_label, uint64_t* counts, uint8_t* pred, void* stream) {
    if (!logits_q || !geometry || !targets || !counts) return MAS_ERR_NULL;
    if (n < 1 || n > MAS_MS_MAX_SOURCES) return MAS_ERR_RANGE;
    if (num_classes < 1 || num_classes > MAS_MAX_CLASSES || (CH != num_classes && CH != num_classes + 1)) return MAS_ERR_CLASSES;
    if (H < 1 || W < 1 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    NvArgs a;
    a.t = reinterpret_cast<const long long*>(targets);
    a.labels = pred;
    a.counts = reinterpret_cast<mas_u64*>(counts);
    a.ignore_label = (long long)ignore_label;
    a.n = n, a.C = CH, a.K = num_classes, a.H = H, a.W = W;
    size_t lds;
    const int st = set_sources(a, logits_q, geometry, &lds);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_ms_naive<true>, dim3((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH)), dim3(kThreads), lds,
                       static_cast<hipStream_t>(stream), a);
    return mas_launch_status();
}

extern "C" int64_t mas_ms_iou_lds_bytes(const int32_t* geometry, int n, int H, int W) {
    if (!geometry) return MAS_ERR_NULL;
    if (n < 1 || n > MAS_MS_MAX_SOURCES) return MAS_ERR_RANGE;
    if (H < 1 || W < 1 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    NvArgs a;
    a.n = n, a.H = H, a.W = W;
    size_t lds;
    const int st = set_sources(a, nullptr, geometry, &lds);
    return st == 0 || st == MAS_ERR_RANGE ? (int64_t)(lds + kStaticLds) : (int64_t)st;
}
