// online_plbl.hip -- online local-prototype pseudo labels and the cross entropy on them, for gfx950.
//
// Reference: trainer/active_onlineplbl_multi_predignore.py:25-141 (LocalProtoCE), active_onlinewplbl_multi_predignore.py:20-148
// (LocalWProtoCE), active_onlinewplblonly_multi_predignore.py:20-137 (JointLocalProtoCE): a Python loop over the pictures with
// nonzero() / scatter_max / unique per picture on feat_forward's full-resolution [N,256,H,W] features.  Here, per batch:
//   mas_online_plbl_labels   memset of the work buffer -> the group scan of losses.hip (MAS_LOSS_GROUP | MAS_LOSS_GROUP_ONLY_MULTI,
//                            quarter-resolution form), which leaves the arg-pixel of every (superpixel, candidate class) ->
//                            k_online_assign: one lane per pixel; a valid pixel interpolates its own feature and the features of its
//                            superpixel's prototype pixels channel by channel from the quarter-resolution map (four candidates per sweep
//                            over the channels) and keeps the nearest; label u8 and weight f32 are written for every pixel.  Prototype
//                            features are re-interpolated per use: nothing is staged, so nothing is sized by a device-side count.
//   k_label_ce_fwd / _bwd    the labelled pixels of a 4 x 256 tile are compacted into an LDS queue and processed one per lane (the
//                            scheme of k_partial_loss_fwd / _bwd); sums are integers (u64 fixed point), the gradient of zq is added
//                            through the four taps into an LDS image of the tile's quarter-resolution footprint and from there into
//                            the int64 accumulator -- no float atomics, run-to-run identical bytes.
//   mas_online_plbl_reference   the same through online_plbl.h on host pointers.
//
// The similarity-weighted siblings: trainer/active_onlinesimwplbl_multi_predignore.py:15-148 (LocalsimWProtoCE: the same labels, the
// weight is the inner product with the chosen prototype -- MAS_OPL_WEIGHT_SIM in k_online_assign, a signed sum with MAS_LCE_SIGNED in
// k_label_ce_fwd) and trainer/active_pwce_multi_predignore.py:17-155 (JointLocalProtoWeightingCE: no hard label):
//   mas_online_soft_weights  memsets -> the same group scan -> k_online_soft: one lane per pixel with the sweep of k_online_assign;
//                            every candidate's raw similarity goes to its plane of softw [N,C,H,W], the pixel's own entries are
//                            normalised in place, the picture is marked live.
//   k_soft_ce_fwd / _bwd     the tile queue of k_label_ce_fwd / _bwd holding the counted pixels (mask set, id in range, live picture);
//                            cross entropy against the soft target, the same LDS image and int64 gradient.
//   mas_simw_plbl_reference  the same on host pointers.
#include "common.h"
#include "online_plbl.h"

namespace {
constexpr int kThreads = 256;
constexpr int kTileW = 256;
constexpr int kTileH = 4;
constexpr int kTilePx = kTileW * kTileH;
constexpr int kSweep = 4;                  // candidates per sweep over the feature channels

struct Geo { int C, Ch, h, w, H, W, S; float sh, sw; };

inline Geo make_geo(int C, int Ch, int h, int w, int H, int W, int S) {
    return Geo{C, Ch, h, w, H, W, S, (float)h / (float)H, (float)w / (float)W};
}

template <int CT, bool EXACT, typename IdT>
__global__ __launch_bounds__(kThreads) void k_online_assign(const float* __restrict__ zq, const float* __restrict__ featq,
                                                             const IdT* __restrict__ spx, const unsigned char* __restrict__ mask,
                                                             const unsigned* __restrict__ bits, const mas_u64* __restrict__ gmax,
                                                             const Geo g, long long total, float invT, int flags,
                                                             unsigned char* __restrict__ labels, float* __restrict__ weight) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int C = EXACT ? CT : g.C;
    const int HW = g.H * g.W;
    const size_t hw = (size_t)g.h * g.w;
    const int n = (int)(i / HW);
    const int pix = (int)(i - (long long)n * HW);
    int label = 255;
    float wgt = 0.0f;
    if (mask[i]) {
        const int id = mas_load_id(spx, (size_t)i);
        if (id >= 0 && id < g.S) {
            const unsigned Y = bits[(size_t)n * g.S + id];
            if (__popc(Y) > 1) {
                const OplTap t = mas_opl_tap(g.sh, g.sw, pix / g.W, pix % g.W, g.h, g.w);
                const mas_u64* gm = gmax + ((size_t)n * g.S + id) * C;
                const float* fb = featq + (size_t)n * g.Ch * hw;
                unsigned Yc = C < 32 ? (Y & ((1u << C) - 1u)) : Y;
                float best = 0.0f;
                int arg = -1;
                bool is_proto = false;
                while (Yc) {
                    int cls[kSweep];
                    OplTap tp[kSweep];
                    float acc[kSweep];
#pragma unroll
                    for (int u = 0; u < kSweep; ++u) {
                        cls[u] = -1;
                        tp[u] = t;
                        acc[u] = 0.0f;
                        if (Yc) {
                            const int c = __ffs(Yc) - 1;
                            Yc &= Yc - 1u;
                            const mas_u64 w64 = gm[c];
                            const unsigned pp = mas_opl_word_pixel(w64);
                            if ((unsigned)(w64 >> 32) != 0u && pp < (unsigned)HW) {     // (always, for a valid pixel: it is in the scan itself)
                                cls[u] = c;
                                tp[u] = mas_opl_tap(g.sh, g.sw, (int)pp / g.W, (int)pp % g.W, g.h, g.w);
                                is_proto = is_proto || pp == (unsigned)pix;
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
                    for (int u = 0; u < kSweep; ++u) {
                        if (cls[u] >= 0 && (arg < 0 || acc[u] > best)) {
                            best = acc[u];
                            arg = cls[u];
                        }
                    }
                }
                if (arg >= 0) {
                    label = arg;
                    if (flags & MAS_OPL_WEIGHT_SIM) {                            // (uniform) the similarity itself, sign and all
                        wgt = best;
                    } else {
                        float v[CT];
                        mas_opl_logits<CT>(zq + (size_t)n * C * hw, hw, t, C, v);
                        mas_opl_softmax<CT>(v, C, invT);
                        wgt = mas_opl_pick<CT>(v, C, arg);
                        if ((flags & MAS_OPL_WEIGHT_WO_PROTO) && is_proto) wgt = 1.0f;
                    }
                }
            }
        }
    }
    labels[i] = (unsigned char)label;
    weight[i] = wgt;
}

// ---- cross entropy on a label map ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void queue_push(bool sel, unsigned short off, unsigned short* queue, int* qcount) {
    const unsigned long long bal = __ballot(sel);
    if (bal == 0) return;
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    int base = 0;
    if (lane == 0) base = atomicAdd(qcount, (int)__popcll(bal));
    base = __shfl(base, 0, MAS_WAVE);
    if (sel) queue[base + (int)__popcll(bal & ((1ull << lane) - 1ull))] = off;
}

// the labelled pixels of the tile (one row per wave) into the queue as (row << 8 | column)
__device__ __forceinline__ void tile_compact(const unsigned char* __restrict__ lb, int C, int H, int W, int tx, int ty,
                                             unsigned short* queue, int* qcount) {
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    const int ry = threadIdx.x / MAS_WAVE;
    const int y = ty * kTileH + ry;
    if (y >= H) return;                       // (wave-uniform)
    const size_t row = (size_t)y * W;
#pragma unroll
    for (int k = 0; k < kTileW / MAS_WAVE; ++k) {
        const int rx = k * MAS_WAVE + lane;
        const int x = tx * kTileW + rx;
        const bool sel = (x < W) && ((int)lb[row + (x < W ? x : 0)] < C);
        queue_push(sel, (unsigned short)((ry << 8) | rx), queue, qcount);
    }
}

struct CeArgs {
    const float* zq; const unsigned char* labels; const float* weight;
    Geo g; float invT; int mode; float th; int tiles_x, tiles_y; int sgn;
};

// probabilities of the queued pixel, its label and the weight its mode gives it
template <int CT, bool EXACT>
__device__ __forceinline__ void ce_pixel(const CeArgs& a, int n, int py, int px, float (&v)[CT], OplTap& t, int& lab, float& wgt) {
    const int C = EXACT ? CT : a.g.C;
    const size_t hw = (size_t)a.g.h * a.g.w;
    const size_t pix = (size_t)n * a.g.H * a.g.W + (size_t)py * a.g.W + px;
    lab = a.labels[pix];
    t = mas_opl_tap(a.g.sh, a.g.sw, py, px, a.g.h, a.g.w);
    mas_opl_logits<CT>(a.zq + (size_t)n * C * hw, hw, t, C, v);
    mas_opl_softmax<CT>(v, C, a.invT);
    wgt = mas_opl_mode_weight(a.mode, a.mode == MAS_LCE_UNWEIGHTED ? 1.0f : a.weight[pix], a.th);
}

template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_label_ce_fwd(const CeArgs a, mas_u64* __restrict__ acc) {
    __shared__ int qcount[2];
    __shared__ unsigned short queue[kTilePx];
    __shared__ mas_u64 s_red[kThreads / MAS_WAVE][2];
    const int C = EXACT ? CT : a.g.C;
    if (threadIdx.x == 0) qcount[0] = 0;
    __syncthreads();
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x; bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int n = bid / a.tiles_y;
    tile_compact(a.labels + (size_t)n * a.g.H * a.g.W, C, a.g.H, a.g.W, tx, ty, queue, qcount);
    __syncthreads();
    const int nq = qcount[0];
    if (nq == 0) return;                      // (uniform)
    mas_u64 sum = 0, cnt = 0;
    for (int i = threadIdx.x; i < nq; i += kThreads) {
        const unsigned off = queue[i];
        float v[CT];
        OplTap t;
        int lab;
        float wgt;
        ce_pixel<CT, EXACT>(a, n, ty * kTileH + (int)(off >> 8), tx * kTileW + (int)(off & 255u), v, t, lab, wgt);
        int counted;
        const float term = mas_opl_term(a.mode, wgt, mas_opl_ce(mas_opl_pick<CT>(v, C, lab)), &counted);
        if (counted) {
            sum += mas_opl_fix_term(term, a.sgn);
            cnt += 1;
        }
    }
    const int lane = threadIdx.x & (MAS_WAVE - 1), wave = threadIdx.x / MAS_WAVE;
#pragma unroll
    for (int off = MAS_WAVE / 2; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, MAS_WAVE);
        cnt += __shfl_down(cnt, off, MAS_WAVE);
    }
    if (lane == 0) { s_red[wave][0] = sum; s_red[wave][1] = cnt; }
    __syncthreads();
    if (threadIdx.x < 2) {
        mas_u64 r = 0;
        for (int wv = 0; wv < kThreads / MAS_WAVE; ++wv) r += s_red[wv][threadIdx.x];
        if (r) atomicAdd(&acc[threadIdx.x], r);
    }
}

__global__ void k_label_ce_value(const mas_u64* __restrict__ acc, int flags, float* __restrict__ loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    loss[0] = mas_opl_value(acc[0], acc[1], flags);
}

// The quarter-resolution footprint of a 4 x 256 tile (<= 4 rows x 72 columns per class for the x4 ratio of the model) is summed in LDS
// first; only its non-zero entries go to memory.  Taps outside that image (other ratios) go to memory directly.
template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_label_ce_bwd(const CeArgs a, const mas_u64* __restrict__ acc, const float* __restrict__ grad,
                                                            mas_u64* __restrict__ dq) {
    constexpr int kLR = 4, kLC = 72;
    __shared__ int qcount[2];
    __shared__ unsigned short queue[kTilePx];
    __shared__ mas_u64 s_acc[EXACT ? CT * kLR * kLC : 1];
    const int C = EXACT ? CT : a.g.C;
    if (threadIdx.x == 0) qcount[0] = 0;
    __syncthreads();
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x; bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int n = bid / a.tiles_y;
    tile_compact(a.labels + (size_t)n * a.g.H * a.g.W, C, a.g.H, a.g.W, tx, ty, queue, qcount);
    __syncthreads();
    const int nq = qcount[0];
    if (nq == 0) return;                      // (uniform)
    const int hw = a.g.h * a.g.w;
    mas_u64* qb = dq + (size_t)n * C * hw;
    const int ry0 = make_tap(a.g.sh, ty * kTileH, a.g.h).i0;
    const int rx0 = make_tap(a.g.sw, tx * kTileW, a.g.w).i0;
    if (EXACT) {
        for (int i = threadIdx.x; i < CT * kLR * kLC; i += kThreads) s_acc[i] = 0;
        __syncthreads();
    }
    // r, x: the tap's place in the LDS image, or r < 0 when it lies outside (then the add goes to memory)
    auto place = [&](int o, int& r, int& x) {
        r = o / a.g.w - ry0;
        x = o % a.g.w - rx0;
        if (!EXACT || r >= kLR || x >= kLC) r = -1;
    };
    auto add_q = [&](int c, int o, int r, int x, long long val) {
        if (EXACT && r >= 0) atomicAdd(&s_acc[(c * kLR + r) * kLC + x], (mas_u64)val);
        else atomicAdd(qb + (size_t)c * hw + o, (mas_u64)val);
    };
    const float scale = (grad[0] / (float)acc[1]) * a.invT;
    for (int i = threadIdx.x; i < nq; i += kThreads) {
        const unsigned off = queue[i];
        float v[CT];
        OplTap t;
        int lab;
        float wgt;
        ce_pixel<CT, EXACT>(a, n, ty * kTileH + (int)(off >> 8), tx * kTileW + (int)(off & 255u), v, t, lab, wgt);
        int counted;
        (void)mas_opl_term(a.mode, wgt, mas_opl_ce(mas_opl_pick<CT>(v, C, lab)), &counted);
        if (!counted) continue;
        const float k = scale * wgt;
        const float w00 = t.l0h * t.l0w, w01 = t.l0h * t.l1w, w10 = t.l1h * t.l0w, w11 = t.l1h * t.l1w;
        int r00, x00, r01, x01, r10, x10, r11, x11;
        place(t.o00, r00, x00);
        place(t.o01, r01, x01);
        place(t.o10, r10, x10);
        place(t.o11, r11, x11);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (EXACT || c < C) {
                const float d = k * (v[c] - ((c == lab) ? 1.0f : 0.0f));
                add_q(c, t.o00, r00, x00, mas_opl_grad_fix(d * w00));
                add_q(c, t.o01, r01, x01, mas_opl_grad_fix(d * w01));
                add_q(c, t.o10, r10, x10, mas_opl_grad_fix(d * w10));
                add_q(c, t.o11, r11, x11, mas_opl_grad_fix(d * w11));
            }
        }
    }
    if (EXACT) {
        __syncthreads();
        for (int i = threadIdx.x; i < CT * kLR * kLC; i += kThreads) {
            const mas_u64 val = s_acc[i];
            if (val) {
                const int c = i / (kLR * kLC), rem = i - c * (kLR * kLC);
                const int r = rem / kLC, x = rem - r * kLC;
                atomicAdd(qb + (size_t)c * hw + (size_t)(ry0 + r) * a.g.w + (rx0 + x), val);
            }
        }
    }
}

// ---- soft targets from the prototype similarities, and the cross entropy against them ------------------------------------------------
// One lane per pixel, the sweep of k_online_assign: every candidate's raw similarity goes to its plane of softw [N,C,H,W], then the
// pixel's own entries are normalised in place (mas_opl_soft_normalise).  Only the candidate planes of valid pixels are written.
template <typename IdT>
__global__ __launch_bounds__(kThreads) void k_online_soft(const float* __restrict__ featq, const IdT* __restrict__ spx,
                                                           const unsigned char* __restrict__ mask, const unsigned* __restrict__ bits,
                                                           const mas_u64* __restrict__ gmax, const Geo g, long long total, float invtau,
                                                           float* softw, int* __restrict__ live) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    if (!mask[i]) return;
    const int id = mas_load_id(spx, (size_t)i);
    if (id < 0 || id >= g.S) return;
    const int HW = g.H * g.W;
    const int n = (int)(i / HW);
    const int pix = (int)(i - (long long)n * HW);
    const unsigned Y = bits[(size_t)n * g.S + id];
    if (__popc(Y) <= 1) return;
    live[n] = 1;
    const size_t hw = (size_t)g.h * g.w;
    const OplTap t = mas_opl_tap(g.sh, g.sw, pix / g.W, pix % g.W, g.h, g.w);
    const mas_u64* gm = gmax + ((size_t)n * g.S + id) * g.C;
    const float* fb = featq + (size_t)n * g.Ch * hw;
    float* sw = softw + (size_t)n * g.C * HW + pix;
    unsigned Yc = g.C < 32 ? (Y & ((1u << g.C) - 1u)) : Y;
    unsigned done = 0;
    while (Yc) {
        int cls[kSweep];
        OplTap tp[kSweep];
        float acc[kSweep];
#pragma unroll
        for (int u = 0; u < kSweep; ++u) {
            cls[u] = -1;
            tp[u] = t;
            acc[u] = 0.0f;
            if (Yc) {
                const int c = __ffs(Yc) - 1;
                Yc &= Yc - 1u;
                const mas_u64 w64 = gm[c];
                const unsigned pp = mas_opl_word_pixel(w64);
                if ((unsigned)(w64 >> 32) != 0u && pp < (unsigned)HW) {     // (always, for a valid pixel: it is in the scan itself)
                    cls[u] = c;
                    tp[u] = mas_opl_tap(g.sh, g.sw, (int)pp / g.W, (int)pp % g.W, g.h, g.w);
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
        for (int u = 0; u < kSweep; ++u) {
            if (cls[u] >= 0) {
                sw[(size_t)cls[u] * HW] = acc[u];
                done |= 1u << cls[u];
            }
        }
    }
    mas_opl_soft_normalise(sw, (size_t)HW, done, invtau);
}

struct SoftArgs {
    const float* zq; const void* spx; const unsigned char* mask; const unsigned* bits; const float* softw; const int* live;
    Geo g; float invT; int spx_dtype; int tiles_x, tiles_y;
};

__device__ __forceinline__ int load_id_any(const void* spx, int dtype, size_t i) {          // (dtype is uniform)
    if (dtype == MAS_ID_I64) return (int)static_cast<const long long*>(spx)[i];
    if (dtype == MAS_ID_I32) return static_cast<const int*>(spx)[i];
    return (int)static_cast<const unsigned short*>(spx)[i];
}

// the counted pixels of the tile (mask set, id in range; the caller has seen that the picture is live) into the queue
__device__ __forceinline__ void tile_compact_soft(const SoftArgs& a, int n, int tx, int ty, unsigned short* queue, int* qcount) {
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    const int ry = threadIdx.x / MAS_WAVE;
    const int y = ty * kTileH + ry;
    if (y >= a.g.H) return;                   // (wave-uniform)
    const size_t row = ((size_t)n * a.g.H + y) * a.g.W;
#pragma unroll
    for (int k = 0; k < kTileW / MAS_WAVE; ++k) {
        const int rx = k * MAS_WAVE + lane;
        const int x = tx * kTileW + rx;
        bool sel = false;
        if (x < a.g.W && a.mask[row + x]) {
            const int id = load_id_any(a.spx, a.spx_dtype, row + x);
            sel = id >= 0 && id < a.g.S;
        }
        queue_push(sel, (unsigned short)((ry << 8) | rx), queue, qcount);
    }
}

// probabilities of the queued pixel, its candidates, whether they carry soft weights, and where those start
template <int CT, bool EXACT>
__device__ __forceinline__ void soft_pixel(const SoftArgs& a, int n, int py, int px, float (&v)[CT], OplTap& t, unsigned& Yc, int& multi,
                                           const float*& sw) {
    const int C = EXACT ? CT : a.g.C;
    const size_t hw = (size_t)a.g.h * a.g.w, HW = (size_t)a.g.H * a.g.W;
    const size_t pix = (size_t)py * a.g.W + px;
    const int id = load_id_any(a.spx, a.spx_dtype, (size_t)n * HW + pix);
    Yc = mas_opl_cands(a.bits[(size_t)n * a.g.S + id], C, &multi);
    sw = a.softw + (size_t)n * C * HW + pix;
    t = mas_opl_tap(a.g.sh, a.g.sw, py, px, a.g.h, a.g.w);
    mas_opl_logits<CT>(a.zq + (size_t)n * C * hw, hw, t, C, v);
    mas_opl_softmax<CT>(v, C, a.invT);
}

template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_soft_ce_fwd(const SoftArgs a, mas_u64* __restrict__ acc) {
    __shared__ int qcount[2];
    __shared__ unsigned short queue[kTilePx];
    __shared__ mas_u64 s_red[kThreads / MAS_WAVE][2];
    const int C = EXACT ? CT : a.g.C;
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x; bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int n = bid / a.tiles_y;
    if (!a.live[n]) return;                   // (uniform) a picture without a valid pixel adds nothing
    if (threadIdx.x == 0) qcount[0] = 0;
    __syncthreads();
    tile_compact_soft(a, n, tx, ty, queue, qcount);
    __syncthreads();
    const int nq = qcount[0];
    if (nq == 0) return;                      // (uniform)
    mas_u64 sum = 0, cnt = 0;
    for (int i = threadIdx.x; i < nq; i += kThreads) {
        const unsigned off = queue[i];
        float v[CT];
        OplTap t;
        unsigned Yc;
        int multi;
        const float* sw;
        soft_pixel<CT, EXACT>(a, n, ty * kTileH + (int)(off >> 8), tx * kTileW + (int)(off & 255u), v, t, Yc, multi, sw);
        float A;
        const float term = mas_opl_soft_term<CT>(v, C, Yc, multi, sw, (size_t)a.g.H * a.g.W, &A);
        sum += mas_fix(term, MAS_LOSS_FRAC_BITS);
        cnt += 1;
    }
    const int lane = threadIdx.x & (MAS_WAVE - 1), wave = threadIdx.x / MAS_WAVE;
#pragma unroll
    for (int off = MAS_WAVE / 2; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, MAS_WAVE);
        cnt += __shfl_down(cnt, off, MAS_WAVE);
    }
    if (lane == 0) { s_red[wave][0] = sum; s_red[wave][1] = cnt; }
    __syncthreads();
    if (threadIdx.x < 2) {
        mas_u64 r = 0;
        for (int wv = 0; wv < kThreads / MAS_WAVE; ++wv) r += s_red[wv][threadIdx.x];
        if (r) atomicAdd(&acc[threadIdx.x], r);
    }
}

// the LDS image of k_label_ce_bwd for the tile's quarter-resolution footprint; other class counts add to memory directly
template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_soft_ce_bwd(const SoftArgs a, const mas_u64* __restrict__ acc, const float* __restrict__ grad,
                                                           mas_u64* __restrict__ dq) {
    constexpr int kLR = 4, kLC = 72;
    __shared__ int qcount[2];
    __shared__ unsigned short queue[kTilePx];
    __shared__ mas_u64 s_acc[EXACT ? CT * kLR * kLC : 1];
    const int C = EXACT ? CT : a.g.C;
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x; bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int n = bid / a.tiles_y;
    if (!a.live[n]) return;                   // (uniform)
    if (threadIdx.x == 0) qcount[0] = 0;
    __syncthreads();
    tile_compact_soft(a, n, tx, ty, queue, qcount);
    __syncthreads();
    const int nq = qcount[0];
    if (nq == 0) return;                      // (uniform)
    const int hw = a.g.h * a.g.w;
    const size_t HW = (size_t)a.g.H * a.g.W;
    mas_u64* qb = dq + (size_t)n * C * hw;
    const int ry0 = make_tap(a.g.sh, ty * kTileH, a.g.h).i0;
    const int rx0 = make_tap(a.g.sw, tx * kTileW, a.g.w).i0;
    if (EXACT) {
        for (int i = threadIdx.x; i < CT * kLR * kLC; i += kThreads) s_acc[i] = 0;
        __syncthreads();
    }
    auto place = [&](int o, int& r, int& x) {
        r = o / a.g.w - ry0;
        x = o % a.g.w - rx0;
        if (!EXACT || r >= kLR || x >= kLC) r = -1;
    };
    auto add_q = [&](int c, int o, int r, int x, long long val) {
        if (EXACT && r >= 0) atomicAdd(&s_acc[(c * kLR + r) * kLC + x], (mas_u64)val);
        else atomicAdd(qb + (size_t)c * hw + o, (mas_u64)val);
    };
    const float k = (grad[0] / (float)acc[1]) * a.invT;
    for (int i = threadIdx.x; i < nq; i += kThreads) {
        const unsigned off = queue[i];
        float v[CT];
        OplTap t;
        unsigned Yc;
        int multi;
        const float* sw;
        soft_pixel<CT, EXACT>(a, n, ty * kTileH + (int)(off >> 8), tx * kTileW + (int)(off & 255u), v, t, Yc, multi, sw);
        float A;
        (void)mas_opl_soft_term<CT>(v, C, Yc, multi, sw, HW, &A);
        const float w00 = t.l0h * t.l0w, w01 = t.l0h * t.l1w, w10 = t.l1h * t.l0w, w11 = t.l1h * t.l1w;
        int r00, x00, r01, x01, r10, x10, r11, x11;
        place(t.o00, r00, x00);
        place(t.o01, r01, x01);
        place(t.o10, r10, x10);
        place(t.o11, r11, x11);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (EXACT || c < C) {
                const int in_y = (int)((Yc >> c) & 1u);
                const float wj = (in_y && multi) ? sw[(size_t)c * HW] : 1.0f;
                const float d = k * mas_opl_soft_dir(v[c], A, in_y, wj);
                add_q(c, t.o00, r00, x00, mas_opl_grad_fix(d * w00));
                add_q(c, t.o01, r01, x01, mas_opl_grad_fix(d * w01));
                add_q(c, t.o10, r10, x10, mas_opl_grad_fix(d * w10));
                add_q(c, t.o11, r11, x11, mas_opl_grad_fix(d * w11));
            }
        }
    }
    if (EXACT) {
        __syncthreads();
        for (int i = threadIdx.x; i < CT * kLR * kLC; i += kThreads) {
            const mas_u64 val = s_acc[i];
            if (val) {
                const int c = i / (kLR * kLC), rem = i - c * (kLR * kLC);
                const int r = rem / kLC, x = rem - r * kLC;
                atomicAdd(qb + (size_t)c * hw + (size_t)(ry0 + r) * a.g.w + (rx0 + x), val);
            }
        }
    }
}

template <int CT, bool EXACT>
int launch_soft_ce(const SoftArgs& a, unsigned nblk, const mas_u64* acc_in, const float* grad, mas_u64* out, bool backward, hipStream_t st) {
    if (!backward) hipLaunchKernelGGL((k_soft_ce_fwd<CT, EXACT>), dim3(nblk), dim3(kThreads), 0, st, a, out);
    else hipLaunchKernelGGL((k_soft_ce_bwd<CT, EXACT>), dim3(nblk), dim3(kThreads), 0, st, a, acc_in, grad, out);
    return mas_launch_status();
}

int dispatch_soft_ce(const SoftArgs& a0, int N, const mas_u64* acc_in, const float* grad, mas_u64* out, bool backward, hipStream_t st) {
    SoftArgs a = a0;
    a.tiles_x = (a.g.W + kTileW - 1) / kTileW;
    a.tiles_y = (a.g.H + kTileH - 1) / kTileH;
    const long long nblk = (long long)N * a.tiles_x * a.tiles_y;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return MAS_ERR_SHAPE;
    switch (a.g.C) {
        case 19: return launch_soft_ce<19, true>(a, (unsigned)nblk, acc_in, grad, out, backward, st);
        case 20: return launch_soft_ce<20, true>(a, (unsigned)nblk, acc_in, grad, out, backward, st);
        case 21: return launch_soft_ce<21, true>(a, (unsigned)nblk, acc_in, grad, out, backward, st);
        default: return launch_soft_ce<MAS_MAX_CLASSES, false>(a, (unsigned)nblk, acc_in, grad, out, backward, st);
    }
}

template <int CT, bool EXACT>
int launch_assign(int spx_dtype, const float* zq, const float* featq, const void* spx, const unsigned char* mask, const unsigned* bits,
                  const mas_u64* gmax, const Geo& g, long long total, float invT, int flags, unsigned char* labels, float* weight,
                  hipStream_t st) {
    const dim3 grid((unsigned)((total + kThreads - 1) / kThreads)), block(kThreads);
#define MAS_OPL_ASSIGN(IDT)                                                                                                              \
    hipLaunchKernelGGL((k_online_assign<CT, EXACT, IDT>), grid, block, 0, st, zq, featq, static_cast<const IDT*>(spx), mask, bits, gmax, g, \
                       total, invT, flags, labels, weight)
    switch (spx_dtype) {
        case MAS_ID_I64: MAS_OPL_ASSIGN(long long); break;
        case MAS_ID_I32: MAS_OPL_ASSIGN(int); break;
        case MAS_ID_U16: MAS_OPL_ASSIGN(unsigned short); break;
        default: return MAS_ERR_DTYPE;
    }
#undef MAS_OPL_ASSIGN
    return mas_launch_status();
}

template <int CT, bool EXACT>
int launch_ce(const CeArgs& a, unsigned nblk, const mas_u64* acc_in, const float* grad, mas_u64* out, bool backward, hipStream_t st) {
    if (!backward) hipLaunchKernelGGL((k_label_ce_fwd<CT, EXACT>), dim3(nblk), dim3(kThreads), 0, st, a, out);
    else hipLaunchKernelGGL((k_label_ce_bwd<CT, EXACT>), dim3(nblk), dim3(kThreads), 0, st, a, acc_in, grad, out);
    return mas_launch_status();
}

int dispatch_ce(const CeArgs& a0, int N, const mas_u64* acc_in, const float* grad, mas_u64* out, bool backward, hipStream_t st) {
    CeArgs a = a0;
    a.tiles_x = (a.g.W + kTileW - 1) / kTileW;
    a.tiles_y = (a.g.H + kTileH - 1) / kTileH;
    const long long nblk = (long long)N * a.tiles_x * a.tiles_y;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return MAS_ERR_SHAPE;
    switch (a.g.C) {
        case 19: return launch_ce<19, true>(a, (unsigned)nblk, acc_in, grad, out, backward, st);
        case 20: return launch_ce<20, true>(a, (unsigned)nblk, acc_in, grad, out, backward, st);
        case 21: return launch_ce<21, true>(a, (unsigned)nblk, acc_in, grad, out, backward, st);
        default: return launch_ce<MAS_MAX_CLASSES, false>(a, (unsigned)nblk, acc_in, grad, out, backward, st);
    }
}

// shape / range checks shared by the entry points; nothing is launched when one fails
int check_geometry(int N, int C, int h, int w, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W) return MAS_ERR_SHAPE;
    if ((long long)H * W > 0x7fffffffLL / 2 || (long long)N * H * W > 0x7fffffffLL) return MAS_ERR_SHAPE;
    if (C < 2 || C > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    return 0;
}

int check_ce(const float* zq, const unsigned char* labels, const float* weight, int N, int C, int h, int w, int H, int W, int flags) {
    if (!zq || !labels) return MAS_ERR_NULL;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    const int mode = flags & 3;
    if ((flags & ~(3 | MAS_LCE_EMPTY_NAN | MAS_LCE_SIGNED)) || mode == 3) return MAS_ERR_RANGE;
    if ((flags & MAS_LCE_SIGNED) && mode != MAS_LCE_WEIGHTED) return MAS_ERR_RANGE;
    if (mode != MAS_LCE_UNWEIGHTED && !weight) return MAS_ERR_NULL;
    return 0;
}

// MAS_OPL_WEIGHT_SIM never reads the prototype flag: both at once is a caller's mistake
bool weight_flags_ok(int flags) {
    if (flags & ~(MAS_OPL_WEIGHT_WO_PROTO | MAS_OPL_WEIGHT_SIM)) return false;
    return (flags & (MAS_OPL_WEIGHT_WO_PROTO | MAS_OPL_WEIGHT_SIM)) != (MAS_OPL_WEIGHT_WO_PROTO | MAS_OPL_WEIGHT_SIM);
}

bool id_dtype_ok(int spx_dtype) { return spx_dtype == MAS_ID_I64 || spx_dtype == MAS_ID_I32 || spx_dtype == MAS_ID_U16; }
}  // namespace

extern "C" size_t mas_online_plbl_work_bytes(int N, int S, int C) {
    if (N <= 0 || S <= 0 || C <= 0) return 0;
    return (8 + (size_t)N * S * C) * sizeof(mas_u64);
}

extern "C" int mas_online_plbl_labels(const float* zq_p, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype,
                                      const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, float invT, int flags,
                                      void* work, size_t work_bytes, uint8_t* labels, float* weight, void* stream) {
    if (!zq_p || !featq || !spx || !mask || !bits || !work || !labels || !weight) return MAS_ERR_NULL;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    if (Ch < 1 || Ch > MAS_OPL_MAX_FEAT || !weight_flags_ok(flags)) return MAS_ERR_RANGE;
    if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
    const size_t need = mas_online_plbl_work_bytes(N, S, C);
    if (work_bytes < need) return MAS_ERR_WORKSPACE;
    if ((uintptr_t)work % 8 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t me = hipMemsetAsync(work, 0, need, st);
    if (me != hipSuccess) return (int)me;
    mas_u64* acc = static_cast<mas_u64*>(work);
    mas_u64* gmax = acc + 8;
    // the per-(superpixel, class) arg-pixel table: the existing group scan and its key encoding
    if (int e = mas_partial_loss_fwd_lowres(zq_p, h, w, spx, spx_dtype, mask, bits, N, C, H, W, S, invT,
                                            MAS_LOSS_GROUP | MAS_LOSS_GROUP_ONLY_MULTI, reinterpret_cast<uint64_t*>(gmax),
                                            reinterpret_cast<uint64_t*>(acc), stream))
        return e;
    const Geo g = make_geo(C, Ch, h, w, H, W, S);
    const long long total = (long long)N * H * W;
    switch (C) {
        case 19: return launch_assign<19, true>(spx_dtype, zq_p, featq, spx, mask, bits, gmax, g, total, invT, flags, labels, weight, st);
        case 20: return launch_assign<20, true>(spx_dtype, zq_p, featq, spx, mask, bits, gmax, g, total, invT, flags, labels, weight, st);
        case 21: return launch_assign<21, true>(spx_dtype, zq_p, featq, spx, mask, bits, gmax, g, total, invT, flags, labels, weight, st);
        default: return launch_assign<MAS_MAX_CLASSES, false>(spx_dtype, zq_p, featq, spx, mask, bits, gmax, g, total, invT, flags, labels,
                                                              weight, st);
    }
}

extern "C" int mas_label_ce_value(const uint64_t* acc, int flags, float* loss, void* stream) {
    if (!acc || !loss) return MAS_ERR_NULL;
    hipLaunchKernelGGL(k_label_ce_value, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const mas_u64*>(acc), flags,
                       loss);
    return mas_launch_status();
}

extern "C" int mas_label_ce_fwd_lowres(const float* zq, int h, int w, const uint8_t* labels, const float* weight, int N, int C, int H, int W,
                                       float invT, int flags, float th, uint64_t* acc, float* loss, void* stream) {
    if (!acc) return MAS_ERR_NULL;
    if (int e = check_ce(zq, labels, weight, N, C, h, w, H, W, flags)) return e;
    if ((uintptr_t)acc % 8 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t me = hipMemsetAsync(acc, 0, 2 * sizeof(uint64_t), st);
    if (me != hipSuccess) return (int)me;
    const CeArgs a{zq, labels, weight, make_geo(C, 0, h, w, H, W, 0), invT, flags & 3, th, 0, 0, (flags & MAS_LCE_SIGNED) ? 1 : 0};
    if (int e = dispatch_ce(a, N, nullptr, nullptr, reinterpret_cast<mas_u64*>(acc), false, st)) return e;
    return loss ? mas_label_ce_value(acc, flags, loss, stream) : 0;
}

extern "C" int mas_label_ce_bwd_lowres(const float* zq, int h, int w, const uint8_t* labels, const float* weight, const uint64_t* acc,
                                       const float* grad, int N, int C, int H, int W, float invT, int flags, float th, int64_t* dzq_fix,
                                       float* dzq, void* stream) {
    if (!acc || !grad || !dzq_fix) return MAS_ERR_NULL;
    if (int e = check_ce(zq, labels, weight, N, C, h, w, H, W, flags)) return e;
    if ((uintptr_t)dzq_fix % 8 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nq = (size_t)N * C * h * w;
    const hipError_t me = hipMemsetAsync(dzq_fix, 0, nq * sizeof(int64_t), st);
    if (me != hipSuccess) return (int)me;
    const CeArgs a{zq, labels, weight, make_geo(C, 0, h, w, H, W, 0), invT, flags & 3, th, 0, 0, (flags & MAS_LCE_SIGNED) ? 1 : 0};
    if (int e = dispatch_ce(a, N, reinterpret_cast<const mas_u64*>(acc), grad, reinterpret_cast<mas_u64*>(dzq_fix), true, st)) return e;
    return dzq ? mas_fix_to_float(dzq_fix, (int64_t)nq, MAS_GRAD_FRAC_BITS, dzq, stream) : 0;
}

namespace {
int check_soft(const float* zq, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits, const float* softw, const int* live,
               int N, int C, int h, int w, int H, int W, int S) {
    if (!zq || !spx || !mask || !bits || !softw || !live) return MAS_ERR_NULL;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
    return 0;
}
}  // namespace

extern "C" int mas_online_soft_weights(const float* zq_p, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype,
                                       const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, float invT, float invtau,
                                       void* work, size_t work_bytes, float* softw, int32_t* live, void* stream) {
    if (!zq_p || !featq || !spx || !mask || !bits || !work || !softw || !live) return MAS_ERR_NULL;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    if (Ch < 1 || Ch > MAS_OPL_MAX_FEAT || !(invtau > 0.0f)) return MAS_ERR_RANGE;
    if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
    const size_t need = mas_online_plbl_work_bytes(N, S, C);
    if (work_bytes < need) return MAS_ERR_WORKSPACE;
    if ((uintptr_t)work % 8 != 0 || (uintptr_t)live % 4 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t me = hipMemsetAsync(work, 0, need, st);
    if (me != hipSuccess) return (int)me;
    me = hipMemsetAsync(live, 0, (size_t)N * sizeof(int32_t), st);
    if (me != hipSuccess) return (int)me;
    mas_u64* acc = static_cast<mas_u64*>(work);
    mas_u64* gmax = acc + 8;
    if (int e = mas_partial_loss_fwd_lowres(zq_p, h, w, spx, spx_dtype, mask, bits, N, C, H, W, S, invT,
                                            MAS_LOSS_GROUP | MAS_LOSS_GROUP_ONLY_MULTI, reinterpret_cast<uint64_t*>(gmax),
                                            reinterpret_cast<uint64_t*>(acc), stream))
        return e;
    const Geo g = make_geo(C, Ch, h, w, H, W, S);
    const long long total = (long long)N * H * W;
    const dim3 grid((unsigned)((total + kThreads - 1) / kThreads)), block(kThreads);
#define MAS_OPL_SOFT(IDT)                                                                                                               \
    hipLaunchKernelGGL((k_online_soft<IDT>), grid, block, 0, st, featq, static_cast<const IDT*>(spx), mask, bits, gmax, g, total, invtau, \
                       softw, live)
    switch (spx_dtype) {
        case MAS_ID_I64: MAS_OPL_SOFT(long long); break;
        case MAS_ID_I32: MAS_OPL_SOFT(int); break;
        default: MAS_OPL_SOFT(unsigned short); break;
    }
#undef MAS_OPL_SOFT
    return mas_launch_status();
}

extern "C" int mas_soft_ce_fwd_lowres(const float* zq, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits,
                                      const float* softw, const int32_t* live, int N, int C, int H, int W, int S, float invT, uint64_t* acc,
                                      float* loss, void* stream) {
    if (!acc) return MAS_ERR_NULL;
    if (int e = check_soft(zq, spx, spx_dtype, mask, bits, softw, live, N, C, h, w, H, W, S)) return e;
    if ((uintptr_t)acc % 8 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t me = hipMemsetAsync(acc, 0, 2 * sizeof(uint64_t), st);
    if (me != hipSuccess) return (int)me;
    const SoftArgs a{zq, spx, mask, bits, softw, live, make_geo(C, 0, h, w, H, W, S), invT, spx_dtype, 0, 0};
    if (int e = dispatch_soft_ce(a, N, nullptr, nullptr, reinterpret_cast<mas_u64*>(acc), false, st)) return e;
    return loss ? mas_label_ce_value(acc, 0, loss, stream) : 0;
}

extern "C" int mas_soft_ce_bwd_lowres(const float* zq, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits,
                                      const float* softw, const int32_t* live, const uint64_t* acc, const float* grad, int N, int C, int H,
                                      int W, int S, float invT, int64_t* dzq_fix, float* dzq, void* stream) {
    if (!acc || !grad || !dzq_fix) return MAS_ERR_NULL;
    if (int e = check_soft(zq, spx, spx_dtype, mask, bits, softw, live, N, C, h, w, H, W, S)) return e;
    if ((uintptr_t)dzq_fix % 8 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nq = (size_t)N * C * h * w;
    const hipError_t me = hipMemsetAsync(dzq_fix, 0, nq * sizeof(int64_t), st);
    if (me != hipSuccess) return (int)me;
    const SoftArgs a{zq, spx, mask, bits, softw, live, make_geo(C, 0, h, w, H, W, S), invT, spx_dtype, 0, 0};
    if (int e = dispatch_soft_ce(a, N, reinterpret_cast<const mas_u64*>(acc), grad, reinterpret_cast<mas_u64*>(dzq_fix), true, st)) return e;
    return dzq ? mas_fix_to_float(dzq_fix, (int64_t)nq, MAS_GRAD_FRAC_BITS, dzq, stream) : 0;
}

// ---- the CPU-side statement: host pointers, plain loops through online_plbl.h.  No device is touched. ---------------------------------
namespace {
long long host_id(const void* spx, int spx_dtype, size_t i) {
    if (spx_dtype == MAS_ID_I64) return static_cast<const long long*>(spx)[i];
    if (spx_dtype == MAS_ID_I32) return static_cast<const int*>(spx)[i];
    return static_cast<const unsigned short*>(spx)[i];
}

// bits[n, id] of a valid pixel (mask set, id in range, more than one bit), 0 otherwise
uint32_t host_valid_bits(const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits, int n, int S, size_t g, long long* id) {
    if (!mask[g]) return 0;
    *id = (int)host_id(spx, spx_dtype, g);         // (the kernels' mas_load_id)
    if (*id < 0 || *id >= S) return 0;
    const uint32_t Y = bits[(size_t)n * S + (size_t)*id];
    return __builtin_popcount(Y) > 1 ? Y : 0;
}

// the arg-pixel table [N,S,C] of the valid pixels (what the group scan leaves)
void host_table(const float* zq_p, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits, int N, int C, int H,
                int W, int S, float invT, uint64_t* table) {
    const size_t HW = (size_t)H * W, hw = (size_t)h * w;
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    for (size_t i = 0; i < (size_t)N * S * C; ++i) table[i] = 0;
    for (int n = 0; n < N; ++n) {
        for (size_t pix = 0; pix < HW; ++pix) {
            const size_t gi = (size_t)n * HW + pix;
            long long id = 0;
            const uint32_t Y = host_valid_bits(spx, spx_dtype, mask, bits, n, S, gi, &id);
            if (!Y) continue;
            const OplTap t = mas_opl_tap(sh, sw, (int)(pix / W), (int)(pix % W), h, w);
            float p[MAS_MAX_CLASSES];
            mas_opl_logits<MAS_MAX_CLASSES>(zq_p + (size_t)n * C * hw, hw, t, C, p);
            mas_opl_softmax<MAS_MAX_CLASSES>(p, C, invT);
            uint64_t* gm = table + ((size_t)n * S + (size_t)id) * C;
            for (int c = 0; c < C; ++c) {
                if (!((Y >> c) & 1u)) continue;
                const uint64_t word = mas_opl_pack(p[c], (uint32_t)pix);
                if (word > gm[c]) gm[c] = word;
            }
        }
    }
}

// similarity of the pixel with tap t to the prototype of candidate c; false when c is no candidate with a prototype
bool host_sim(const uint64_t* gm, uint32_t Y, int c, const float* fb, int Ch, size_t hw, const Geo& g, const OplTap& t, uint32_t pix,
              float* sim, bool* is_proto) {
    if (!((Y >> c) & 1u) || (gm[c] >> 32) == 0) return false;
    const uint32_t pp = mas_opl_word_pixel(gm[c]);
    if (pp >= (uint32_t)(g.H * g.W)) return false;
    const OplTap tp = mas_opl_tap(g.sh, g.sw, (int)(pp / g.W), (int)(pp % g.W), g.h, g.w);
    float s = 0.0f;
    for (int k = 0; k < Ch; ++k) s = mas_fmaf(mas_opl_at(fb + (size_t)k * hw, tp), mas_opl_at(fb + (size_t)k * hw, t), s);
    *sim = s;
    *is_proto = pp == pix;
    return true;
}
}  // namespace

extern "C" int mas_online_plbl_reference(const float* zq_p, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype,
                                         const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, float invT, int flags,
                                         uint64_t* gmax, uint8_t* labels, float* weight, const float* zq, float invT_ce, int ce_flags,
                                         float th, const float* grad, uint64_t* acc, float* loss, int64_t* dzq_fix) {
    if (!labels) return MAS_ERR_NULL;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    const size_t HW = (size_t)H * W, hw = (size_t)h * w;
    const Geo g = make_geo(C, Ch, h, w, H, W, S);
    if (zq_p) {
        if (!featq || !spx || !mask || !bits || !weight) return MAS_ERR_NULL;
        if (S <= 0) return MAS_ERR_SHAPE;
        if (Ch < 1 || Ch > MAS_OPL_MAX_FEAT || !weight_flags_ok(flags)) return MAS_ERR_RANGE;
        if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
        uint64_t* table = gmax ? gmax : new uint64_t[(size_t)N * S * C];
        host_table(zq_p, h, w, spx, spx_dtype, mask, bits, N, C, H, W, S, invT, table);
        for (int n = 0; n < N; ++n) {
            const float* fb = featq + (size_t)n * Ch * hw;
            for (size_t pix = 0; pix < HW; ++pix) {
                const size_t gi = (size_t)n * HW + pix;
                labels[gi] = 255;
                weight[gi] = 0.0f;
                long long id = 0;
                const uint32_t Y = host_valid_bits(spx, spx_dtype, mask, bits, n, S, gi, &id);
                if (!Y) continue;
                const OplTap t = mas_opl_tap(g.sh, g.sw, (int)(pix / W), (int)(pix % W), h, w);
                const uint64_t* gm = table + ((size_t)n * S + (size_t)id) * C;
                float best = 0.0f;
                int arg = -1;
                bool is_proto = false;
                for (int c = 0; c < C; ++c) {
                    float sim;
                    bool proto;
                    if (!host_sim(gm, Y, c, fb, Ch, hw, g, t, (uint32_t)pix, &sim, &proto)) continue;
                    is_proto = is_proto || proto;
                    if (arg < 0 || sim > best) { best = sim; arg = c; }
                }
                if (arg < 0) continue;
                labels[gi] = (uint8_t)arg;
                if (flags & MAS_OPL_WEIGHT_SIM) {
                    weight[gi] = best;
                } else if ((flags & MAS_OPL_WEIGHT_WO_PROTO) && is_proto) {
                    weight[gi] = 1.0f;
                } else {
                    float p[MAS_MAX_CLASSES];
                    mas_opl_logits<MAS_MAX_CLASSES>(zq_p + (size_t)n * C * hw, hw, t, C, p);
                    mas_opl_softmax<MAS_MAX_CLASSES>(p, C, invT);
                    weight[gi] = p[arg];
                }
            }
        }
        if (!gmax) delete[] table;
    }
    if (!zq) return 0;
    if (!acc) return MAS_ERR_NULL;
    if (int e = check_ce(zq, labels, weight, N, C, h, w, H, W, ce_flags)) return e;
    if (dzq_fix && !grad) return MAS_ERR_NULL;
    const int mode = ce_flags & 3;
    acc[0] = acc[1] = 0;
    for (int pass = 0; pass < (dzq_fix ? 2 : 1); ++pass) {
        float scale = 0.0f;
        if (pass == 1) {
            scale = (grad[0] / (float)acc[1]) * invT_ce;
            for (size_t i = 0; i < (size_t)N * C * hw; ++i) dzq_fix[i] = 0;
        }
        for (int n = 0; n < N; ++n) {
            for (size_t pix = 0; pix < HW; ++pix) {
                const size_t gi = (size_t)n * HW + pix;
                const int lab = labels[gi];
                if (lab >= C) continue;
                const OplTap t = mas_opl_tap(g.sh, g.sw, (int)(pix / W), (int)(pix % W), h, w);
                float p[MAS_MAX_CLASSES];
                mas_opl_logits<MAS_MAX_CLASSES>(zq + (size_t)n * C * hw, hw, t, C, p);
                mas_opl_softmax<MAS_MAX_CLASSES>(p, C, invT_ce);
                const float wgt = mas_opl_mode_weight(mode, mode == MAS_LCE_UNWEIGHTED ? 1.0f : weight[gi], th);
                int counted;
                const float term = mas_opl_term(mode, wgt, mas_opl_ce(p[lab]), &counted);
                if (!counted) continue;
                if (pass == 0) {
                    acc[0] += mas_opl_fix_term(term, (ce_flags & MAS_LCE_SIGNED) ? 1 : 0);
                    acc[1] += 1;
                    continue;
                }
                const float k = scale * wgt;
                const float w00 = t.l0h * t.l0w, w01 = t.l0h * t.l1w, w10 = t.l1h * t.l0w, w11 = t.l1h * t.l1w;
                for (int c = 0; c < C; ++c) {
                    int64_t* q = dzq_fix + ((size_t)n * C + c) * hw;
                    const float d = k * (p[c] - ((c == lab) ? 1.0f : 0.0f));
                    q[t.o00] += mas_opl_grad_fix(d * w00);
                    q[t.o01] += mas_opl_grad_fix(d * w01);
                    q[t.o10] += mas_opl_grad_fix(d * w10);
                    q[t.o11] += mas_opl_grad_fix(d * w11);
                }
            }
        }
        if (pass == 0 && loss) loss[0] = mas_opl_value(acc[0], acc[1], ce_flags);
    }
    return 0;
}

extern "C" int mas_simw_plbl_reference(const float* zq_p, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype,
                                       const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, float invT, float invtau,
                                       float* softw, int32_t* live, const float* zq, float invT_ce, const float* grad, uint64_t* acc,
                                       float* loss, int64_t* dzq_fix) {
    if (!spx || !mask || !bits || !softw || !live) return MAS_ERR_NULL;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
    const size_t HW = (size_t)H * W, hw = (size_t)h * w;
    const Geo g = make_geo(C, Ch, h, w, H, W, S);
    if (zq_p) {
        if (!featq) return MAS_ERR_NULL;
        if (Ch < 1 || Ch > MAS_OPL_MAX_FEAT || !(invtau > 0.0f)) return MAS_ERR_RANGE;
        uint64_t* table = new uint64_t[(size_t)N * S * C];
        host_table(zq_p, h, w, spx, spx_dtype, mask, bits, N, C, H, W, S, invT, table);
        for (int n = 0; n < N; ++n) {
            const float* fb = featq + (size_t)n * Ch * hw;
            live[n] = 0;
            for (size_t pix = 0; pix < HW; ++pix) {
                const size_t gi = (size_t)n * HW + pix;
                long long id = 0;
                const uint32_t Y = host_valid_bits(spx, spx_dtype, mask, bits, n, S, gi, &id);
                if (!Y) continue;
                live[n] = 1;
                const OplTap t = mas_opl_tap(g.sh, g.sw, (int)(pix / W), (int)(pix % W), h, w);
                const uint64_t* gm = table + ((size_t)n * S + (size_t)id) * C;
                float* sw = softw + (size_t)n * C * HW + pix;
                uint32_t done = 0;
                for (int c = 0; c < C; ++c) {
                    float sim;
                    bool proto;
                    if (!host_sim(gm, Y, c, fb, Ch, hw, g, t, (uint32_t)pix, &sim, &proto)) continue;
                    sw[(size_t)c * HW] = sim;
                    done |= 1u << c;
                }
                mas_opl_soft_normalise(sw, HW, done, invtau);
            }
        }
        delete[] table;
    }
    if (!zq) return 0;
    if (!acc) return MAS_ERR_NULL;
    if (dzq_fix && !grad) return MAS_ERR_NULL;
    acc[0] = acc[1] = 0;
    for (int pass = 0; pass < (dzq_fix ? 2 : 1); ++pass) {
        float k = 0.0f;
        if (pass == 1) {
            k = (grad[0] / (float)acc[1]) * invT_ce;
            for (size_t i = 0; i < (size_t)N * C * hw; ++i) dzq_fix[i] = 0;
        }
        for (int n = 0; n < N; ++n) {
            if (!live[n]) continue;
            for (size_t pix = 0; pix < HW; ++pix) {
                const size_t gi = (size_t)n * HW + pix;
                if (!mask[gi]) continue;
                const long long id = (int)host_id(spx, spx_dtype, gi);
                if (id < 0 || id >= S) continue;
                int multi;
                const uint32_t Yc = mas_opl_cands(bits[(size_t)n * S + (size_t)id], C, &multi);
                const float* sw = softw + (size_t)n * C * HW + pix;
                const OplTap t = mas_opl_tap(g.sh, g.sw, (int)(pix / W), (int)(pix % W), h, w);
                float p[MAS_MAX_CLASSES];
                mas_opl_logits<MAS_MAX_CLASSES>(zq + (size_t)n * C * hw, hw, t, C, p);
                mas_opl_softmax<MAS_MAX_CLASSES>(p, C, invT_ce);
                float A;
                const float term = mas_opl_soft_term<MAS_MAX_CLASSES>(p, C, Yc, multi, sw, HW, &A);
                if (pass == 0) {
                    acc[0] += mas_fix(term, MAS_LOSS_FRAC_BITS);
                    acc[1] += 1;
                    continue;
                }
                const float w00 = t.l0h * t.l0w, w01 = t.l0h * t.l1w, w10 = t.l1h * t.l0w, w11 = t.l1h * t.l1w;
                for (int c = 0; c < C; ++c) {
                    int64_t* q = dzq_fix + ((size_t)n * C + c) * hw;
                    const int in_y = (int)((Yc >> c) & 1u);
                    const float wj = (in_y && multi) ? sw[(size_t)c * HW] : 1.0f;
                    const float d = k * mas_opl_soft_dir(p[c], A, in_y, wj);
                    q[t.o00] += mas_opl_grad_fix(d * w00);
                    q[t.o01] += mas_opl_grad_fix(d * w01);
                    q[t.o10] += mas_opl_grad_fix(d * w10);
                    q[t.o11] += mas_opl_grad_fix(d * w11);
                }
            }
        }
        if (pass == 0 && loss) loss[0] = mas_opl_value(acc[0], acc[1], 0);
    }
    return 0;
}
