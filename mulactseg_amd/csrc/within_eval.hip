// within_eval.hip -- quality of the local-prototype pseudo labels inside the queried superpixels of the labelled set, for gfx950.
//
// Reference: trainer/eval_cosplbl_within_multihot.py:84-179, eval_cosplbl_filt_within_multihot.py:68-173,
// eval_maxcosplbl_within_multihot.py:71-176 and eval_ensemble_plbl_within_multihot.py (the same generation): per picture nonzero() /
// scatter_max / unique and a dense nproto x nvalid torch.mm on feat_forward's full-resolution [N,256,H,W] features, then MeanIoU on the
// int64 label map.  Here one call per batch:
//   prologue         every check, the memset of the work buffer, and the group scan of losses.hip (MAS_LOSS_GROUP, quarter-resolution
//                    form, temperature 1), which leaves the arg-pixel of every (superpixel, candidate class) -- one-hot rows included.
//   k_within_eval    one lane per pixel.  A valid pixel interpolates its logits (arg-max, the global similarity of the maxcos
//                    diagnostic) and, channel by channel, its own feature and the features of its superpixel's prototype pixels
//                    (kSweep candidates per sweep, the scheme of k_online_assign: nothing is staged, so nothing is sized by a
//                    device-side count), keeps the nearest, applies the mode (within_eval.h) and tallies the label against the ground
//                    truth into the workgroup's LDS histogram; every other pixel tallies 255.  One flush of 64-bit atomics per
//                    workgroup.  The label map is written only when the caller wants it; no [N,C,H,W] or [N,Ch,H,W] tensor exists.
//   mas_within_eval_reference   the same on host pointers, a plain loop through within_eval.h: the statement the kernel is tested
//                    against bit for bit.
#include "common.h"
#include "within_eval.h"
#include "iou_tally.h"

namespace {
constexpr int kThreads = 256;
constexpr int kPerThread = 4;              // pixels per lane, kThreads apart
constexpr int kSweep = 4;                  // candidates per sweep over the feature channels
constexpr int kMaxCnt = 3 * (MAS_MAX_CLASSES + 1);
constexpr int kDiag = 4;

struct Geo { int C, Ch, h, w, H, W, S; float sh, sw; };

inline Geo make_geo(int C, int Ch, int h, int w, int H, int W, int S) {
    return Geo{C, Ch, h, w, H, W, S, (float)h / (float)H, (float)w / (float)W};
}

// The candidates Yc of a pixel with tap t, kSweep per pass over the channels of fb (the picture's features): emit(class, similarity,
// is_prototype) sees them class-ascending.  gm: the pixel's row of the table.
template <typename Emit>
__device__ __forceinline__ void sweep_candidates(const float* __restrict__ fb, const mas_u64* __restrict__ gm, unsigned Yc, const OplTap& t,
                                                 int pix, const Geo& g, Emit emit) {
    const unsigned HW = (unsigned)(g.H * g.W);
    const size_t hw = (size_t)g.h * g.w;
    while (Yc) {
        int cls[kSweep];
        OplTap tp[kSweep];
        float acc[kSweep];
        bool proto[kSweep];
#pragma unroll
        for (int u = 0; u < kSweep; ++u) {
            cls[u] = -1;
            tp[u] = t;
            acc[u] = 0.0f;
            proto[u] = false;
            if (Yc) {
                const int c = __ffs(Yc) - 1;
                Yc &= Yc - 1u;
                unsigned pp;
                if (mas_we_word_proto(gm[c], HW, &pp)) {        // (always, for a valid pixel: it is in the scan itself)
                    cls[u] = c;
                    tp[u] = mas_opl_tap(g.sh, g.sw, (int)pp / g.W, (int)pp % g.W, g.h, g.w);
                    proto[u] = pp == (unsigned)pix;
                }
            }
        }
        for (int k = 0; k < g.Ch; ++k) {
            const float* fk = fb + (size_t)k * hw;
            const float fx = mas_opl_at(fk, t);
#pragma unroll
            for (int u = 0; u < kSweep; ++u)
                if (cls[u] >= 0) acc[u] = mas_fmaf(mas_opl_at(fk, tp[u]), fx, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < kSweep; ++u)
            if (cls[u] >= 0) emit(cls[u], acc[u], proto[u]);
    }
}

template <typename IdT>
__global__ __launch_bounds__(kThreads) void k_within_eval(const float* __restrict__ zq, const float* __restrict__ featq,
                                                           const IdT* __restrict__ spx, const unsigned char* __restrict__ mask,
                                                           const unsigned* __restrict__ bits, const long long* __restrict__ gt,
                                                           const mas_u64* __restrict__ gmax, const Geo g, long long total, long long n_table,
                                                           int mode, int K, long long ignore_label, unsigned char* __restrict__ labels,
                                                           mas_u64* __restrict__ counts, mas_u64* __restrict__ diag) {
    __shared__ unsigned s_cnt[kMaxCnt + kDiag];
    const int ncnt = 3 * K + 3;
    for (int i = threadIdx.x; i < ncnt + kDiag; i += kThreads) s_cnt[i] = 0;
    __syncthreads();
    unsigned* s_diag = s_cnt + ncnt;
    const int C = g.C;
    const int HW = g.H * g.W;
    const size_t hw = (size_t)g.h * g.w;

    // diag[1]: the table entries that hold a prototype
    unsigned n_proto = 0;
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < n_table; j += (long long)gridDim.x * kThreads) {
        unsigned pp;
        n_proto += mas_we_word_proto(gmax[j], (unsigned)HW, &pp) ? 1u : 0u;
    }
    if (n_proto) atomicAdd(&s_diag[1], n_proto);

    const long long base = (long long)blockIdx.x * (kThreads * kPerThread) + threadIdx.x;
    for (int it = 0; it < kPerThread; ++it) {
        const long long i = base + (long long)it * kThreads;
        if (i >= total) break;
        const int n = (int)(i / HW);
        const int pix = (int)(i - (long long)n * HW);
        int label = 255;
        const unsigned char mb = mask[i];
        const int id = mb ? mas_load_id(spx, (size_t)i) : -1;
        const unsigned Y = mas_we_valid_bits(mb, id, g.S, bits + (size_t)n * g.S);
        if (Y) {
            const OplTap t = mas_opl_tap(g.sh, g.sw, pix / g.W, pix % g.W, g.h, g.w);
            int amax = 0;
            float top = 0.0f, glob = 0.0f;
            const float* zb = zq + (size_t)n * C * hw;
#pragma unroll 4
            for (int c = 0; c < C; ++c) mas_we_logit_step(c, mas_opl_at(zb + (size_t)c * hw, t), Y, &top, &amax, &glob);
            float best = 0.0f;
            int arg = -1, proto_hi = -1;
            sweep_candidates(featq + (size_t)n * g.Ch * hw, gmax + ((size_t)n * g.S + id) * C, mas_we_cands(Y, C), t, pix, g,
                             [&](int c, float sim, bool proto) {
                                 if (proto) proto_hi = c;                 // (ascending: the last is the highest)
                                 if (arg < 0 || sim > best) {
                                     best = sim;
                                     arg = c;
                                 }
                             });
            int removed;
            label = mas_we_label(mode, arg, amax, proto_hi, &removed);
            atomicAdd(&s_diag[0], 1u);
            if (arg >= 0 && best < glob) atomicAdd(&s_diag[2], 1u);
            if (removed) atomicAdd(&s_diag[3], 1u);
        }
        tally(s_cnt, K, gt[i], (long long)label, -1, ignore_label, false);
        if (labels) labels[i] = (unsigned char)label;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ncnt + kDiag; i += kThreads) {
        const unsigned v = s_cnt[i];
        if (v) atomicAdd(i < ncnt ? &counts[i] : &diag[i - ncnt], (mas_u64)v);
    }
}

template <typename F>
int for_id_type(const void* spx, int spx_dtype, F f) {
    switch (spx_dtype) {
        case MAS_ID_I64: return f(static_cast<const long long*>(spx));
        case MAS_ID_I32: return f(static_cast<const int*>(spx));
        case MAS_ID_U16: return f(static_cast<const unsigned short*>(spx));
        default: return MAS_ERR_DTYPE;
    }
}

// every check both entry points share (the ranges of mas_online_plbl_labels); nothing is launched when one fails
int check_args(const float* zq, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
               const uint32_t* bits, const int64_t* gt, int N, int C, int H, int W, int S, int mode, int K, const uint64_t* counts,
               const uint64_t* diag) {
    if (!zq || !featq || !spx || !mask || !bits || !gt || !counts || !diag) return MAS_ERR_NULL;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (N <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W) return MAS_ERR_SHAPE;
    if ((long long)H * W > 0x7fffffffLL / 2 || (long long)N * H * W > 0x7fffffffLL) return MAS_ERR_SHAPE;
    if (C < 2 || C > MAS_MAX_CLASSES || K < C || K > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    if (Ch < 1 || Ch > MAS_OPL_MAX_FEAT) return MAS_ERR_RANGE;
    if (mode != MAS_WE_PROTO && mode != MAS_WE_FILT) return MAS_ERR_RANGE;
    if (spx_dtype != MAS_ID_I64 && spx_dtype != MAS_ID_I32 && spx_dtype != MAS_ID_U16) return MAS_ERR_DTYPE;
    if ((uintptr_t)counts % 8 != 0 || (uintptr_t)diag % 8 != 0 || (uintptr_t)bits % 4 != 0 || (uintptr_t)gt % 8 != 0) return MAS_ERR_ALIGN;
    return 0;
}

long long host_id(const void* spx, int spx_dtype, size_t i) {
    if (spx_dtype == MAS_ID_I64) return (int)static_cast<const long long*>(spx)[i];         // (the kernel's mas_load_id)
    if (spx_dtype == MAS_ID_I32) return static_cast<const int*>(spx)[i];
    return static_cast<const unsigned short*>(spx)[i];
}
}  // namespace

extern "C" size_t mas_within_eval_work_bytes(int N, int S, int C) {
    if (N <= 0 || S <= 0 || C <= 0) return 0;
    return (8 + (size_t)N * S * C) * sizeof(mas_u64);
}

extern "C" int mas_within_eval_counts(const float* zq, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype,
                                      const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, const int64_t* gt,
                                      int mode, int K, int64_t ignore_label, void* work, size_t work_bytes, uint64_t* counts, uint64_t* diag,
                                      uint8_t* labels, void* stream) {
    if (int e = check_args(zq, featq, Ch, h, w, spx, spx_dtype, mask, bits, gt, N, C, H, W, S, mode, K, counts, diag)) return e;
    if (!work) return MAS_ERR_NULL;
    const size_t need = mas_within_eval_work_bytes(N, S, C);
    if (work_bytes < need) return MAS_ERR_WORKSPACE;
    if ((uintptr_t)work % 8 != 0) return MAS_ERR_ALIGN;
    const long long total = (long long)N * H * W;
    const long long per_block = (long long)kThreads * kPerThread;
    const long long nblk = (total + per_block - 1) / per_block;
    if (nblk > 0x7fffffffLL) return MAS_ERR_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t me = hipMemsetAsync(work, 0, need, st);
    if (me != hipSuccess) return (int)me;
    uint64_t* acc = static_cast<uint64_t*>(work);
    const mas_u64* gmax = reinterpret_cast<const mas_u64*>(acc + 8);
    if (int e = mas_partial_loss_fwd_lowres(zq, h, w, spx, spx_dtype, mask, bits, N, C, H, W, S, 1.0f, MAS_LOSS_GROUP, acc + 8, acc, stream))
        return e;
    const Geo g = make_geo(C, Ch, h, w, H, W, S);
    return for_id_type(spx, spx_dtype, [&](auto ids) {
        hipLaunchKernelGGL(k_within_eval, dim3((unsigned)nblk), dim3(kThreads), 0, st, zq, featq, ids, mask, bits,
                           reinterpret_cast<const long long*>(gt), gmax, g, total, (long long)N * S * C, mode, K, (long long)ignore_label, labels,
                           reinterpret_cast<mas_u64*>(counts), reinterpret_cast<mas_u64*>(diag));
        return mas_launch_status();
    });
}

// ---- the CPU-side statement: host pointers, plain loops through within_eval.h.  No device is touched. ---------------------------------
extern "C" int mas_within_eval_reference(const float* zq, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype,
                                         const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, const int64_t* gt,
                                         int mode, int K, int64_t ignore_label, uint64_t* counts, uint64_t* diag, uint8_t* labels,
                                         uint64_t* gmax) {
    if (int e = check_args(zq, featq, Ch, h, w, spx, spx_dtype, mask, bits, gt, N, C, H, W, S, mode, K, counts, diag)) return e;
    const size_t HW = (size_t)H * W, hw = (size_t)h * w;
    const Geo g = make_geo(C, Ch, h, w, H, W, S);
    uint64_t* table = gmax ? gmax : new uint64_t[(size_t)N * S * C];
    for (size_t i = 0; i < (size_t)N * S * C; ++i) table[i] = 0;
    // the arg-pixel table of the valid pixels (what the group scan leaves)
    for (int n = 0; n < N; ++n) {
        for (size_t pix = 0; pix < HW; ++pix) {
            const size_t gi = (size_t)n * HW + pix;
            const long long id = mask[gi] ? host_id(spx, spx_dtype, gi) : -1;
            const uint32_t Y = mas_we_valid_bits(mask[gi], id, S, bits + (size_t)n * S);
            if (!Y) continue;
            const OplTap t = mas_opl_tap(g.sh, g.sw, (int)(pix / W), (int)(pix % W), h, w);
            float p[MAS_MAX_CLASSES];
            mas_opl_logits<MAS_MAX_CLASSES>(zq + (size_t)n * C * hw, hw, t, C, p);
            mas_opl_softmax<MAS_MAX_CLASSES>(p, C, 1.0f);
            uint64_t* gm = table + ((size_t)n * S + (size_t)id) * C;
            for (int c = 0; c < C; ++c) {
                if (!((Y >> c) & 1u)) continue;
                const uint64_t word = mas_opl_pack(p[c], (uint32_t)pix);
                if (word > gm[c]) gm[c] = word;
            }
        }
    }
    for (size_t i = 0; i < (size_t)N * S * C; ++i) {
        uint32_t pp;
        if (mas_we_word_proto(table[i], (uint32_t)HW, &pp)) diag[1] += 1;
    }
    for (int n = 0; n < N; ++n) {
        const float* fb = featq + (size_t)n * Ch * hw;
        for (size_t pix = 0; pix < HW; ++pix) {
            const size_t gi = (size_t)n * HW + pix;
            int label = 255;
            const long long id = mask[gi] ? host_id(spx, spx_dtype, gi) : -1;
            const uint32_t Y = mas_we_valid_bits(mask[gi], id, S, bits + (size_t)n * S);
            if (Y) {
                const OplTap t = mas_opl_tap(g.sh, g.sw, (int)(pix / W), (int)(pix % W), h, w);
                int amax = 0;
                float top = 0.0f, glob = 0.0f;
                for (int c = 0; c < C; ++c) mas_we_logit_step(c, mas_opl_at(zq + ((size_t)n * C + c) * hw, t), Y, &top, &amax, &glob);
                const uint64_t* gm = table + ((size_t)n * S + (size_t)id) * C;
                const uint32_t Yc = mas_we_cands(Y, C);
                float best = 0.0f;
                int arg = -1, proto_hi = -1;
                for (int c = 0; c < C; ++c) {
                    uint32_t pp;
                    if (!((Yc >> c) & 1u) || !mas_we_word_proto(gm[c], (uint32_t)HW, &pp)) continue;
                    const OplTap tp = mas_opl_tap(g.sh, g.sw, (int)(pp / W), (int)(pp % W), h, w);
                    float s = 0.0f;
                    for (int k = 0; k < Ch; ++k) s = mas_fmaf(mas_opl_at(fb + (size_t)k * hw, tp), mas_opl_at(fb + (size_t)k * hw, t), s);
                    if (pp == (uint32_t)pix) proto_hi = c;
                    if (arg < 0 || s > best) { best = s; arg = c; }
                }
                int removed;
                label = mas_we_label(mode, arg, amax, proto_hi, &removed);
                diag[0] += 1;
                if (arg >= 0 && best < glob) diag[2] += 1;
                if (removed) diag[3] += 1;
            }
            // MeanIoU._after_step on the label map (iou_tally.h without the ignore-class counters)
            const long long tg = gt[gi];
            if (tg != ignore_label) {
                if (tg >= 0 && tg < K) {
                    counts[tg] += 1;
                    if (label == tg) counts[K + tg] += 1;
                }
                if (label < K) counts[2 * K + label] += 1;
            }
            if (labels) labels[gi] = (uint8_t)label;
        }
    }
    if (!gmax) delete[] table;
    return 0;
}
