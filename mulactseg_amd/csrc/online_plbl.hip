// online_plbl.hip -- online local-prototype pseudo labels and the cross entropy on them, for gfx950.
//
// Reference: trainer/active_onlineplbl_multi_predignore.py:25-141 (LocalProtoCE), active_onlinewplbl_multi_predignore.py:20-148
// (LocalWProtoCE), active_onlinewplblonly_multi_predignore.py:20-137 (JointLocalProtoCE), and the similarity-weighted siblings
// active_onlinesimwplbl_multi_predignore.py:15-148 (LocalsimWProtoCE) and active_pwce_multi_predignore.py:17-155
// (JointLocalProtoWeightingCE, no hard label): a Python loop over the pictures with nonzero() / scatter_max / unique per picture on
// feat_forward's full-resolution [N,256,H,W] features.  Here every piece exists once and the two families are its two users:
//   scan_prototypes     the prologue of mas_online_plbl_labels and mas_online_soft_weights: checks, memset of the work buffer, the
//                       group scan of losses.hip (MAS_LOSS_GROUP | MAS_LOSS_GROUP_ONLY_MULTI, quarter-resolution form), which leaves the
//                       arg-pixel of every (superpixel, candidate class).
//   sweep_candidates    one lane per pixel: a valid pixel interpolates its own feature and the features of its superpixel's prototype
//                       pixels channel by channel from the quarter-resolution map (kSweep candidates per sweep over the channels) and
//                       hands every (class, similarity, is_prototype) to its caller.  Prototype features are re-interpolated per use:
//                       nothing is staged, so nothing is sized by a device-side count.
//                         k_online_assign  keeps the nearest; label u8 and weight f32 (the label's probability, 1 on a prototype with
//                                          MAS_OPL_WEIGHT_WO_PROTO, the similarity itself with MAS_OPL_WEIGHT_SIM) for every pixel.
//                         k_online_soft    stores every similarity to its plane of softw [N,C,H,W], normalises the pixel's own
//                                          entries in place and marks the picture live.
//   ce_fwd / ce_bwd     the tile-queue core: the selected pixels of a 4 x 256 tile are compacted into an LDS queue and processed one
//                       per lane (the scheme of k_partial_loss_fwd / _bwd); sums are integers (u64 fixed point), the gradient of zq is
//                       added through the four taps into QuarterImage, an LDS image of the tile's quarter-resolution footprint, and from
//                       there into the int64 accumulator -- no float atomics, run-to-run identical bytes.  A policy says which pictures
//                       and pixels take part and what a queued pixel yields:
//                         LabelCe  (k_label_ce_fwd / _bwd)  the labelled pixels; the mode's weight, MAS_LCE_SIGNED sums.
//                         SoftCe   (k_soft_ce_fwd / _bwd)   the counted pixels (mask set, id in range) of the live pictures; cross
//                                                           entropy against the soft target.
//                         HierCe   (k_hier_fwd / _bwd)      the hierarchical group term (hier_group.h): the selected pixels of the fine
//                                                           superpixels that hold an arg-pixel of the group scan, weighted per class
//                                                           by the pair table `mult` that k_hier_pairs builds between the two scans.
//   host_ce             the same two passes on host pointers through online_plbl.h, with host policies of its own:
//                       mas_online_plbl_reference and mas_simw_plbl_reference, the statement the kernels are tested against.
// losses.hip keeps a twin of queue_push, the tile compaction and the LDS image (another tap struct, the benchmarked training step).
#include <type_traits>

#include "common.h"
#include "online_plbl.h"
#include "hier_group.h"

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

// ---- the per-pixel kernels -----------------------------------------------------------------------------------------------------------
// The candidates Yc of a pixel with tap t, kSweep per pass over the channels of fb: the prototype pixel of each is decoded from its
// word of gm, the similarity is the chain of online_plbl.h (sim), and emit(class, similarity, is_prototype) sees them class-ascending.
template <typename Emit>
__device__ __forceinline__ void sweep_candidates(const float* __restrict__ fb, const mas_u64* __restrict__ gm, unsigned Yc, const OplTap& t,
                                                 int pix, const Geo& g, Emit emit) {
    const int HW = g.H * g.W;
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
                const mas_u64 w64 = gm[c];
                const unsigned pp = mas_opl_word_pixel(w64);
                if ((unsigned)(w64 >> 32) != 0u && pp < (unsigned)HW) {     // (always, for a valid pixel: it is in the scan itself)
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
                float best = 0.0f;
                int arg = -1;
                bool is_proto = false;
                sweep_candidates(featq + (size_t)n * g.Ch * hw, gmax + ((size_t)n * g.S + id) * C, C < 32 ? (Y & ((1u << C) - 1u)) : Y, t,
                                 pix, g, [&](int c, float sim, bool proto) {
                                     is_proto = is_proto || proto;
                                     if (arg < 0 || sim > best) {
                                         best = sim;
                                         arg = c;
                                     }
                                 });
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

// Only the candidate planes of valid pixels are written.
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
    float* sw = softw + (size_t)n * g.C * HW + pix;
    unsigned done = 0;
    sweep_candidates(featq + (size_t)n * g.Ch * hw, gmax + ((size_t)n * g.S + id) * g.C, g.C < 32 ? (Y & ((1u << g.C) - 1u)) : Y, t, pix, g,
                     [&](int c, float sim, bool) {
                         sw[(size_t)c * HW] = sim;
                         done |= 1u << c;
                     });
    mas_opl_soft_normalise(sw, (size_t)HW, done, invtau);
}

// ---- the tile-queue cross entropy ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void queue_push(bool sel, unsigned short off, unsigned short* queue, int* qcount) {
    const unsigned long long bal = __ballot(sel);
    if (bal == 0) return;
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    int base = 0;
    if (lane == 0) base = atomicAdd(qcount, (int)__popcll(bal));
    base = __shfl(base, 0, MAS_WAVE);
    if (sel) queue[base + (int)__popcll(bal & ((1ull << lane) - 1ull))] = off;
}

// The workgroup's tile (n, ty, tx) and, in the queue as (row << 8 | column), the pixels of it that the policy selects (one row per
// wave).  Returns their number (uniform); 0 also for a picture the policy leaves out.
template <typename P>
__device__ __forceinline__ int tile_queue(const P& a, int C, unsigned short* queue, int* qcount, int& n, int& ty, int& tx) {
    int bid = blockIdx.x;
    tx = bid % a.tiles_x; bid /= a.tiles_x;
    ty = bid % a.tiles_y;
    n = bid / a.tiles_y;
    if (!a.runs(n)) return 0;                 // (uniform)
    if (threadIdx.x == 0) qcount[0] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    const int ry = threadIdx.x / MAS_WAVE;
    const int y = ty * kTileH + ry;
    if (y < a.g.H) {                          // (wave-uniform)
        const size_t row = ((size_t)n * a.g.H + y) * a.g.W;
#pragma unroll
        for (int k = 0; k < kTileW / MAS_WAVE; ++k) {
            const int rx = k * MAS_WAVE + lane;
            const int x = tx * kTileW + rx;
            const bool sel = (x < a.g.W) && a.selects(row + (x < a.g.W ? x : 0), C);
            queue_push(sel, (unsigned short)((ry << 8) | rx), queue, qcount);
        }
    }
    __syncthreads();
    return qcount[0];
}

// probabilities of pixel (py, px) of picture n and its tap
template <int CT, bool EXACT>
__device__ __forceinline__ void ce_probs(const float* __restrict__ zq, const Geo& g, float invT, int n, int py, int px, float (&v)[CT],
                                         OplTap& t) {
    const int C = EXACT ? CT : g.C;
    const size_t hw = (size_t)g.h * g.w;
    t = mas_opl_tap(g.sh, g.sw, py, px, g.h, g.w);
    mas_opl_logits<CT>(zq + (size_t)n * C * hw, hw, t, C, v);
    mas_opl_softmax<CT>(v, C, invT);
}

// A policy of the core is the kernel's argument struct (zq, g, invT, tiles_x, tiles_y and its own) with
//   runs(n)                   whether picture n takes part at all;
//   selects(i, C)             whether pixel i of [N,H,W] goes into the queue;
//   pixel(n, py, px, v, t, s, term)   probabilities v and tap t of a queued pixel, the policy's state s and the pixel's term;
//                             returns whether it is counted;
//   fix(term)                 what a counted term adds to the u64 sum;
//   count(s)                  what a counted pixel adds to the count;
//   scale(grad, count)        the backward's common factor from the upstream gradient and the forward's count;
//   k(s, scale), dir(s, c, p_c)   the gradient of class c is k * dir.
struct LabelCe {
    const float* zq; const unsigned char* labels; const float* weight;
    Geo g; float invT; int mode; float th; int tiles_x, tiles_y; int sgn;
    struct Px { int lab; float wgt; };

    __device__ __forceinline__ bool runs(int) const { return true; }
    __device__ __forceinline__ bool selects(size_t i, int C) const { return (int)labels[i] < C; }
    template <int CT, bool EXACT>
    __device__ __forceinline__ bool pixel(int n, int py, int px, float (&v)[CT], OplTap& t, Px& s, float& term) const {
        const size_t i = ((size_t)n * g.H + py) * g.W + px;
        s.lab = labels[i];
        ce_probs<CT, EXACT>(zq, g, invT, n, py, px, v, t);
        s.wgt = mas_opl_mode_weight(mode, mode == MAS_LCE_UNWEIGHTED ? 1.0f : weight[i], th);
        int counted;
        term = mas_opl_term(mode, s.wgt, mas_opl_ce(mas_opl_pick<CT>(v, EXACT ? CT : g.C, s.lab)), &counted);
        return counted != 0;
    }
    __device__ __forceinline__ mas_u64 fix(float term) const { return mas_opl_fix_term(term, sgn); }
    __device__ __forceinline__ mas_u64 count(const Px&) const { return 1; }
    __device__ __forceinline__ float scale(float grad, mas_u64 n) const { return (grad / (float)n) * invT; }
    __device__ __forceinline__ float k(const Px& s, float scale) const { return scale * s.wgt; }
    __device__ __forceinline__ float dir(const Px& s, int c, float pc) const { return pc - ((c == s.lab) ? 1.0f : 0.0f); }
};

__device__ __forceinline__ int load_id_any(const void* spx, int dtype, size_t i) {          // (dtype is uniform)
    if (dtype == MAS_ID_I64) return (int)static_cast<const long long*>(spx)[i];
    if (dtype == MAS_ID_I32) return static_cast<const int*>(spx)[i];
    return (int)static_cast<const unsigned short*>(spx)[i];
}

struct SoftCe {
    const float* zq; const void* spx; const unsigned char* mask; const unsigned* bits; const float* softw; const int* live;
    Geo g; float invT; int spx_dtype; int tiles_x, tiles_y;
    struct Px { unsigned Yc; int multi; const float* sw; float A; };     // candidates, whether they carry soft weights, where those start

    __device__ __forceinline__ bool runs(int n) const { return live[n] != 0; }            // a picture without a valid pixel adds nothing
    __device__ __forceinline__ bool selects(size_t i, int) const {
        if (!mask[i]) return false;
        const int id = load_id_any(spx, spx_dtype, i);
        return id >= 0 && id < g.S;
    }
    template <int CT, bool EXACT>
    __device__ __forceinline__ bool pixel(int n, int py, int px, float (&v)[CT], OplTap& t, Px& s, float& term) const {
        const int C = EXACT ? CT : g.C;
        const size_t HW = (size_t)g.H * g.W, pix = (size_t)py * g.W + px;
        const int id = load_id_any(spx, spx_dtype, (size_t)n * HW + pix);
        s.Yc = mas_opl_cands(bits[(size_t)n * g.S + id], C, &s.multi);
        s.sw = softw + (size_t)n * C * HW + pix;
        ce_probs<CT, EXACT>(zq, g, invT, n, py, px, v, t);
        term = mas_opl_soft_term<CT>(v, C, s.Yc, s.multi, s.sw, HW, &s.A);
        return true;
    }
    __device__ __forceinline__ mas_u64 fix(float term) const { return mas_fix(term, MAS_LOSS_FRAC_BITS); }
    __device__ __forceinline__ mas_u64 count(const Px&) const { return 1; }
    __device__ __forceinline__ float scale(float grad, mas_u64 n) const { return (grad / (float)n) * invT; }
    __device__ __forceinline__ float k(const Px&, float scale) const { return scale; }
    __device__ __forceinline__ float dir(const Px& s, int c, float pc) const {
        const int in_y = (int)((s.Yc >> c) & 1u);
        const float wj = (in_y && s.multi) ? s.sw[(size_t)c * ((size_t)g.H * g.W)] : 1.0f;
        return mas_opl_soft_dir(pc, s.A, in_y, wj);
    }
};

// g.S is the number of FINE superpixels here.  The softmax runs at temperature 1 (hier_group.h).
struct HierCe {
    const float* zq; const void* small; const unsigned char* mask; const unsigned* mult; const unsigned* any;
    Geo g; int small_dtype; int tiles_x, tiles_y;
    struct Px { unsigned Yc; const unsigned* m; float U; unsigned cnt; };

    __device__ __forceinline__ bool runs(int) const { return true; }
    __device__ __forceinline__ bool selects(size_t i, int) const {
        if (!mask[i]) return false;
        const int id = load_id_any(small, small_dtype, i);
        if (id < 0 || id >= g.S) return false;
        return any[(i / ((size_t)g.H * g.W)) * g.S + id] != 0u;
    }
    template <int CT, bool EXACT>
    __device__ __forceinline__ bool pixel(int n, int py, int px, float (&v)[CT], OplTap& t, Px& s, float& term) const {
        const int C = EXACT ? CT : g.C;
        const size_t row = (size_t)n * g.S + load_id_any(small, small_dtype, ((size_t)n * g.H + py) * g.W + px);
        s.Yc = C < 32 ? (any[row] & ((1u << C) - 1u)) : any[row];
        s.m = mult + row * C;
        ce_probs<CT, EXACT>(zq, g, 1.0f, n, py, px, v, t);
        term = mas_hg_term<CT>(v, C, s.Yc, s.m, &s.U, &s.cnt);
        return true;
    }
    __device__ __forceinline__ mas_u64 fix(float term) const { return mas_fix(term, MAS_LOSS_FRAC_BITS); }
    __device__ __forceinline__ mas_u64 count(const Px& s) const { return s.cnt; }
    __device__ __forceinline__ float scale(float grad, mas_u64 n) const { return mas_hg_scale(grad, n); }
    __device__ __forceinline__ float k(const Px&, float scale) const { return scale; }
    __device__ __forceinline__ float dir(const Px& s, int c, float pc) const {
        return mas_hg_dir(pc, s.U, ((s.Yc >> c) & 1u) ? (float)s.m[c] : 0.0f);
    }
};

// HierCe with the teacher's per-pair weight (hier_group.h, the cross-view forms): w_c = mult * wgt, a pair of weight 0 is not counted.
struct WHierCe {
    const float* zq; const void* small; const unsigned char* mask; const unsigned* mult; const unsigned* any; const float* wgt;
    Geo g; int small_dtype; int tiles_x, tiles_y;
    struct Px { unsigned Yc; const unsigned* m; const float* wg; float U; unsigned cnt; };

    __device__ __forceinline__ bool runs(int) const { return true; }
    __device__ __forceinline__ bool selects(size_t i, int) const {
        if (!mask[i]) return false;
        const int id = load_id_any(small, small_dtype, i);
        if (id < 0 || id >= g.S) return false;
        return any[(i / ((size_t)g.H * g.W)) * g.S + id] != 0u;
    }
    template <int CT, bool EXACT>
    __device__ __forceinline__ bool pixel(int n, int py, int px, float (&v)[CT], OplTap& t, Px& s, float& term) const {
        const int C = EXACT ? CT : g.C;
        const size_t row = (size_t)n * g.S + load_id_any(small, small_dtype, ((size_t)n * g.H + py) * g.W + px);
        s.Yc = C < 32 ? (any[row] & ((1u << C) - 1u)) : any[row];
        s.m = mult + row * C;
        s.wg = wgt + row * C;
        ce_probs<CT, EXACT>(zq, g, 1.0f, n, py, px, v, t);
        term = mas_ahg_term<CT>(v, C, s.Yc, s.m, s.wg, &s.U, &s.cnt);
        return true;
    }
    __device__ __forceinline__ mas_u64 fix(float term) const { return mas_fix(term, MAS_LOSS_FRAC_BITS); }
    __device__ __forceinline__ mas_u64 count(const Px& s) const { return s.cnt; }
    __device__ __forceinline__ float scale(float grad, mas_u64 n) const { return mas_hg_scale(grad, n); }
    __device__ __forceinline__ float k(const Px&, float scale) const { return scale; }
    __device__ __forceinline__ float dir(const Px& s, int c, float pc) const {
        return mas_hg_dir(pc, s.U, ((s.Yc >> c) & 1u) ? (float)s.m[c] * s.wg[c] : 0.0f);
    }
};

template <int CT, bool EXACT, typename P>
__device__ __forceinline__ void ce_fwd(const P& a, mas_u64* __restrict__ acc) {
    __shared__ int qcount[2];
    __shared__ unsigned short queue[kTilePx];
    __shared__ mas_u64 s_red[kThreads / MAS_WAVE][2];
    int n, ty, tx;
    const int nq = tile_queue(a, EXACT ? CT : a.g.C, queue, qcount, n, ty, tx);
    if (nq == 0) return;                      // (uniform)
    mas_u64 sum = 0, cnt = 0;
    for (int i = threadIdx.x; i < nq; i += kThreads) {
        const unsigned off = queue[i];
        float v[CT];
        OplTap t;
        typename P::Px s;
        float term;
        if (a.template pixel<CT, EXACT>(n, ty * kTileH + (int)(off >> 8), tx * kTileW + (int)(off & 255u), v, t, s, term)) {
            sum += a.fix(term);
            cnt += a.count(s);
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

// The quarter-resolution footprint of a 4 x 256 tile (<= 4 rows x 72 columns per class for the x4 ratio of the model) is summed in LDS
// first; only its non-zero entries go to memory.  Taps outside that image (other ratios) go to memory directly, and so does every tap
// of the generic class count, which has no image.
// The image is held through a pointer typed as LDS.  Through a generic one the optimiser merges the two adds of a tap into one flat
// atomic on a selected pointer (no DS atomic left, 80 registers more, a wave less: profiles/opl_core/README.md).
typedef __attribute__((address_space(3))) mas_u64 lds_u64;

template <int CT, bool EXACT>
struct QuarterImage {
    static constexpr int kLR = 4, kLC = 72, kPlane = kLR * kLC, kSize = EXACT ? CT * kPlane : 1;
    lds_u64* s_acc;               // [kSize]
    mas_u64* qb;                  // the picture's planes [C, h*w] in memory
    int hw, w, ry0, rx0;

    __device__ __forceinline__ void zero() const {
        if (!EXACT) return;
        for (int i = threadIdx.x; i < kSize; i += kThreads) s_acc[i] = 0;
        __syncthreads();
    }
    // the place of element o of a plane within the image's plane, or -1 when it lies outside (then the add goes to memory)
    __device__ __forceinline__ int place(int o) const {
        const int r = o / w - ry0, x = o % w - rx0;
        return (!EXACT || r >= kLR || x >= kLC) ? -1 : r * kLC + x;
    }
    __device__ __forceinline__ void add(int c, int o, int at, long long val) const {
        if (EXACT && at >= 0) __hip_atomic_fetch_add(&s_acc[c * kPlane + at], (mas_u64)val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else atomicAdd(qb + (size_t)c * hw + o, (mas_u64)val);
    }
    __device__ __forceinline__ void flush() const {
        if (!EXACT) return;
        __syncthreads();
        for (int i = threadIdx.x; i < kSize; i += kThreads) {
            const mas_u64 val = s_acc[i];
            if (val) {
                const int c = i / kPlane, rem = i - c * kPlane;
                const int r = rem / kLC, x = rem - r * kLC;
                atomicAdd(qb + (size_t)c * hw + (size_t)(ry0 + r) * w + (rx0 + x), val);
            }
        }
    }
};

template <int CT, bool EXACT, typename P>
__device__ __forceinline__ void ce_bwd(const P& a, const mas_u64* __restrict__ acc, const float* __restrict__ grad, mas_u64* __restrict__ dq) {
    __shared__ int qcount[2];
    __shared__ unsigned short queue[kTilePx];
    __shared__ mas_u64 s_acc[QuarterImage<CT, EXACT>::kSize];
    const int C = EXACT ? CT : a.g.C;
    int n, ty, tx;
    const int nq = tile_queue(a, C, queue, qcount, n, ty, tx);
    if (nq == 0) return;                      // (uniform)
    const int hw = a.g.h * a.g.w;
    const QuarterImage<CT, EXACT> img{(lds_u64*)s_acc, dq + (size_t)n * C * hw, hw, a.g.w, make_tap(a.g.sh, ty * kTileH, a.g.h).i0,
                                      make_tap(a.g.sw, tx * kTileW, a.g.w).i0};
    img.zero();
    const float scale = a.scale(grad[0], acc[1]);
    for (int i = threadIdx.x; i < nq; i += kThreads) {
        const unsigned off = queue[i];
        float v[CT];
        OplTap t;
        typename P::Px s;
        float term;
        if (!a.template pixel<CT, EXACT>(n, ty * kTileH + (int)(off >> 8), tx * kTileW + (int)(off & 255u), v, t, s, term)) continue;
        const float k = a.k(s, scale);
        const float w00 = t.l0h * t.l0w, w01 = t.l0h * t.l1w, w10 = t.l1h * t.l0w, w11 = t.l1h * t.l1w;
        const int at00 = img.place(t.o00), at01 = img.place(t.o01), at10 = img.place(t.o10), at11 = img.place(t.o11);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (EXACT || c < C) {
                const float d = k * a.dir(s, c, v[c]);
                img.add(c, t.o00, at00, mas_opl_grad_fix(d * w00));
                img.add(c, t.o01, at01, mas_opl_grad_fix(d * w01));
                img.add(c, t.o10, at10, mas_opl_grad_fix(d * w10));
                img.add(c, t.o11, at11, mas_opl_grad_fix(d * w11));
            }
        }
    }
    img.flush();
}

// the entry names of the traces and profiles: thin shells over the core
template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_label_ce_fwd(const LabelCe a, mas_u64* __restrict__ acc) { ce_fwd<CT, EXACT>(a, acc); }
template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_label_ce_bwd(const LabelCe a, const mas_u64* __restrict__ acc, const float* __restrict__ grad,
                                                            mas_u64* __restrict__ dq) { ce_bwd<CT, EXACT>(a, acc, grad, dq); }
template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_soft_ce_fwd(const SoftCe a, mas_u64* __restrict__ acc) { ce_fwd<CT, EXACT>(a, acc); }
template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_soft_ce_bwd(const SoftCe a, const mas_u64* __restrict__ acc, const float* __restrict__ grad,
                                                           mas_u64* __restrict__ dq) { ce_bwd<CT, EXACT>(a, acc, grad, dq); }

template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_hier_fwd(const HierCe a, mas_u64* __restrict__ acc) { ce_fwd<CT, EXACT>(a, acc); }
template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_hier_bwd(const HierCe a, const mas_u64* __restrict__ acc, const float* __restrict__ grad,
                                                        mas_u64* __restrict__ dq) { ce_bwd<CT, EXACT>(a, acc, grad, dq); }

template <int CT, bool EXACT> auto fwd_kernel(const LabelCe&) { return &k_label_ce_fwd<CT, EXACT>; }
template <int CT, bool EXACT> auto bwd_kernel(const LabelCe&) { return &k_label_ce_bwd<CT, EXACT>; }
template <int CT, bool EXACT> auto fwd_kernel(const SoftCe&) { return &k_soft_ce_fwd<CT, EXACT>; }
template <int CT, bool EXACT> auto bwd_kernel(const SoftCe&) { return &k_soft_ce_bwd<CT, EXACT>; }
template <int CT, bool EXACT> auto fwd_kernel(const HierCe&) { return &k_hier_fwd<CT, EXACT>; }
template <int CT, bool EXACT> auto bwd_kernel(const HierCe&) { return &k_hier_bwd<CT, EXACT>; }

template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_whier_fwd(const WHierCe a, mas_u64* __restrict__ acc) { ce_fwd<CT, EXACT>(a, acc); }
template <int CT, bool EXACT>
__global__ __launch_bounds__(kThreads) void k_whier_bwd(const WHierCe a, const mas_u64* __restrict__ acc, const float* __restrict__ grad,
                                                         mas_u64* __restrict__ dq) { ce_bwd<CT, EXACT>(a, acc, grad, dq); }
template <int CT, bool EXACT> auto fwd_kernel(const WHierCe&) { return &k_whier_fwd<CT, EXACT>; }
template <int CT, bool EXACT> auto bwd_kernel(const WHierCe&) { return &k_whier_bwd<CT, EXACT>; }

__global__ void k_label_ce_value(const mas_u64* __restrict__ acc, int flags, float* __restrict__ loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    loss[0] = mas_opl_value(acc[0], acc[1], flags);
}

// ---- the hierarchical group term between the two scans (hier_group.h) -----------------------------------------------------------------
// One lane per word of the group scan's table [N,S,C]: the arg-pixel's fine superpixel s' takes the pair (s', c).
__global__ __launch_bounds__(kThreads) void k_hier_pairs(const mas_u64* __restrict__ gmax, const void* __restrict__ small, int small_dtype,
                                                          long long total, int S, int C, int HW, int Ss, unsigned* __restrict__ mult,
                                                          unsigned* __restrict__ any) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const mas_u64 w64 = gmax[i];
    if ((unsigned)(w64 >> 32) == 0u) return;
    const unsigned pp = mas_opl_word_pixel(w64);
    if (pp >= (unsigned)HW) return;
    const int c = (int)(i % C);
    const size_t n = (size_t)(i / ((long long)S * C));
    const int id = load_id_any(small, small_dtype, n * HW + pp);
    if (id < 0 || id >= Ss) return;
    atomicAdd(&mult[(n * Ss + id) * C + c], 1u);
    atomicOr(&any[n * Ss + id], 1u << c);
}

// One lane per pixel of the outermost rows and columns (2W + 2H per picture, the corners twice): its superpixel's row of out = 0.
// Every writer writes the same value.
__global__ __launch_bounds__(kThreads) void k_clear_boundary_bits(const void* __restrict__ spx, int spx_dtype, int N, int H, int W, int S,
                                                                   unsigned* __restrict__ out) {
    const int per = 2 * W + 2 * H;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)N * per) return;
    const int n = (int)(i / per), k = (int)(i % per);
    int y, x;
    if (k < W) { y = 0; x = k; }
    else if (k < 2 * W) { y = H - 1; x = k - W; }
    else if (k < 2 * W + H) { y = k - 2 * W; x = 0; }
    else { y = k - 2 * W - H; x = W - 1; }
    const int id = load_id_any(spx, spx_dtype, ((size_t)n * H + y) * W + x);
    if (id >= 0 && id < S) out[(size_t)n * S + id] = 0u;
}

__global__ void k_hier_value(const mas_u64* __restrict__ acc, float* __restrict__ loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    loss[0] = mas_hg_value(acc[0], acc[1]);
}

// ---- the teacher's per-pair weight over the weak view (hier_group.h, the cross-view forms) --------------------------------------------
// One lane per pixel of the weak view; g.S is the number of FINE superpixels.  Only a selected pixel whose fine superpixel holds a pair
// computes a softmax, and only the classes of existing pairs are touched: the traffic is as sparse as the pair table.  Integer atomics
// only -- an unsigned maximum of the bit patterns (p_c >= 0), or a u64 fixed-point sum beside a u32 pixel count per fine superpixel.
template <int CT, bool EXACT, bool MEAN>
__global__ __launch_bounds__(kThreads) void k_hier_weights(const float* __restrict__ zq, const void* __restrict__ small, int small_dtype,
                                                            const unsigned char* __restrict__ mask, const unsigned* __restrict__ any,
                                                            const Geo g, long long total, unsigned* __restrict__ wgt_bits,
                                                            mas_u64* __restrict__ wsum, unsigned* __restrict__ wcnt) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    if (!mask[i]) return;
    const int id = load_id_any(small, small_dtype, (size_t)i);
    if (id < 0 || id >= g.S) return;
    const int C = EXACT ? CT : g.C;
    const int HW = g.H * g.W;
    const int n = (int)(i / HW);
    const int pix = (int)(i - (long long)n * HW);
    const size_t row = (size_t)n * g.S + id;
    const unsigned Yc = C < 32 ? (any[row] & ((1u << C) - 1u)) : any[row];
    if (!Yc) return;
    float v[CT];
    OplTap t;
    ce_probs<CT, EXACT>(zq, g, 1.0f, n, pix / g.W, pix % g.W, v, t);
    if (MEAN) atomicAdd(&wcnt[row], 1u);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        if (c < C && ((Yc >> c) & 1u)) {
            if (MEAN) atomicAdd(&wsum[row * C + c], (mas_u64)mas_ahg_fix(v[c]));
            else atomicMax(&wgt_bits[row * C + c], mas_f2u(v[c]));
        }
    }
}

// One lane per word of the table [N,Ss,C]: the mean weight of an existing pair whose fine superpixel has selected weak pixels.
__global__ __launch_bounds__(kThreads) void k_hier_weights_mean(const mas_u64* __restrict__ wsum, const unsigned* __restrict__ wcnt,
                                                                 const unsigned* __restrict__ any, long long total, int C,
                                                                 float* __restrict__ wgt) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const long long row = i / C;
    const int c = (int)(i - row * C);
    const unsigned cnt = wcnt[row];
    if (cnt != 0u && ((any[row] >> c) & 1u)) wgt[i] = mas_ahg_mean(wsum[i], cnt);
}

// ---- dispatch -----------------------------------------------------------------------------------------------------------------------
// f(class extent, exact) for the class counts with a build of their own, else for the generic one
template <typename F>
int for_class_count(int C, F f) {
    switch (C) {
        case 19: return f(std::integral_constant<int, 19>{}, std::true_type{});
        case 20: return f(std::integral_constant<int, 20>{}, std::true_type{});
        case 21: return f(std::integral_constant<int, 21>{}, std::true_type{});
        default: return f(std::integral_constant<int, MAS_MAX_CLASSES>{}, std::false_type{});
    }
}

bool id_dtype_ok(int spx_dtype) { return spx_dtype == MAS_ID_I64 || spx_dtype == MAS_ID_I32 || spx_dtype == MAS_ID_U16; }

// f(typed id pointer); the entry points have refused every other dtype (id_dtype_ok)
template <typename F>
int for_id_type(const void* spx, int spx_dtype, F f) {
    switch (spx_dtype) {
        case MAS_ID_I64: return f(static_cast<const long long*>(spx));
        case MAS_ID_I32: return f(static_cast<const int*>(spx));
        case MAS_ID_U16: return f(static_cast<const unsigned short*>(spx));
        default: return MAS_ERR_DTYPE;
    }
}

// one workgroup per tile of every picture: the forward into out = acc when grad is null, else the backward into out = dq
template <typename P>
int launch_ce(P a, int N, const mas_u64* acc_in, const float* grad, mas_u64* out, hipStream_t st) {
    a.tiles_x = (a.g.W + kTileW - 1) / kTileW;
    a.tiles_y = (a.g.H + kTileH - 1) / kTileH;
    const long long nblk = (long long)N * a.tiles_x * a.tiles_y;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return MAS_ERR_SHAPE;
    return for_class_count(a.g.C, [&](auto ct, auto exact) {
        constexpr int CT = decltype(ct)::value;
        constexpr bool EXACT = decltype(exact)::value;
        if (!grad) hipLaunchKernelGGL((fwd_kernel<CT, EXACT>(a)), dim3((unsigned)nblk), dim3(kThreads), 0, st, a, out);
        else hipLaunchKernelGGL((bwd_kernel<CT, EXACT>(a)), dim3((unsigned)nblk), dim3(kThreads), 0, st, a, acc_in, grad, out);
        return mas_launch_status();
    });
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

int check_soft(const float* zq, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits, const float* softw, const int* live,
               int N, int C, int h, int w, int H, int W, int S) {
    if (!zq || !spx || !mask || !bits || !softw || !live) return MAS_ERR_NULL;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
    return 0;
}

// MAS_OPL_WEIGHT_SIM never reads the prototype flag: both at once is a caller's mistake
bool weight_flags_ok(int flags) {
    if (flags & ~(MAS_OPL_WEIGHT_WO_PROTO | MAS_OPL_WEIGHT_SIM)) return false;
    return (flags & (MAS_OPL_WEIGHT_WO_PROTO | MAS_OPL_WEIGHT_SIM)) != (MAS_OPL_WEIGHT_WO_PROTO | MAS_OPL_WEIGHT_SIM);
}

// The prologue of the two per-pixel entry points.  `given`: every pointer is there; `range_ok`: the entry's own scalar is in range;
// `live`, when the entry has one, is zeroed with the work buffer.  Leaves in *gmax the per-(superpixel, class) arg-pixel table: the
// existing group scan and its key encoding.
int scan_prototypes(bool given, const float* zq_p, int Ch, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
                    const uint32_t* bits, int N, int C, int H, int W, int S, float invT, bool range_ok, void* work, size_t work_bytes,
                    int32_t* live, void* stream, const mas_u64** gmax) {
    if (!given) return MAS_ERR_NULL;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    if (Ch < 1 || Ch > MAS_OPL_MAX_FEAT || !range_ok) return MAS_ERR_RANGE;
    if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
    const size_t need = mas_online_plbl_work_bytes(N, S, C);
    if (work_bytes < need) return MAS_ERR_WORKSPACE;
    if ((uintptr_t)work % 8 != 0 || (uintptr_t)live % 4 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t me = hipMemsetAsync(work, 0, need, st);
    if (me == hipSuccess && live) me = hipMemsetAsync(live, 0, (size_t)N * sizeof(int32_t), st);
    if (me != hipSuccess) return (int)me;
    uint64_t* acc = static_cast<uint64_t*>(work);
    *gmax = reinterpret_cast<const mas_u64*>(acc + 8);
    return mas_partial_loss_fwd_lowres(zq_p, h, w, spx, spx_dtype, mask, bits, N, C, H, W, S, invT, MAS_LOSS_GROUP | MAS_LOSS_GROUP_ONLY_MULTI,
                                       acc + 8, acc, stream);
}

// the tail of the forward entry points: acc is zeroed, filled, and turned into the value when the caller wants it
template <typename P>
int ce_forward(const P& a, int N, uint64_t* acc, int value_flags, float* loss, void* stream) {
    if ((uintptr_t)acc % 8 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t me = hipMemsetAsync(acc, 0, 2 * sizeof(uint64_t), st);
    if (me != hipSuccess) return (int)me;
    if (int e = launch_ce(a, N, nullptr, nullptr, reinterpret_cast<mas_u64*>(acc), st)) return e;
    return loss ? mas_label_ce_value(acc, value_flags, loss, stream) : 0;
}

// the tail of the backward entry points: dzq_fix [N,C,h,w] is zeroed, filled, and converted when the caller wants floats
template <typename P>
int ce_backward(const P& a, int N, const uint64_t* acc, const float* grad, int64_t* dzq_fix, float* dzq, void* stream) {
    if ((uintptr_t)dzq_fix % 8 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nq = (size_t)N * a.g.C * a.g.h * a.g.w;
    const hipError_t me = hipMemsetAsync(dzq_fix, 0, nq * sizeof(int64_t), st);
    if (me != hipSuccess) return (int)me;
    if (int e = launch_ce(a, N, reinterpret_cast<const mas_u64*>(acc), grad, reinterpret_cast<mas_u64*>(dzq_fix), st)) return e;
    return dzq ? mas_fix_to_float(dzq_fix, (int64_t)nq, MAS_GRAD_FRAC_BITS, dzq, stream) : 0;
}

LabelCe label_ce(const float* zq, int h, int w, const uint8_t* labels, const float* weight, int C, int H, int W, float invT, int flags,
                 float th) {
    return LabelCe{zq, labels, weight, make_geo(C, 0, h, w, H, W, 0), invT, flags & 3, th, 0, 0, (flags & MAS_LCE_SIGNED) ? 1 : 0};
}
}  // namespace

extern "C" size_t mas_online_plbl_work_bytes(int N, int S, int C) {
    if (N <= 0 || S <= 0 || C <= 0) return 0;
    return (8 + (size_t)N * S * C) * sizeof(mas_u64);
}

extern "C" int mas_online_plbl_labels(const float* zq_p, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype,
                                      const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, float invT, int flags,
                                      void* work, size_t work_bytes, uint8_t* labels, float* weight, void* stream) {
    const mas_u64* gmax;
    if (int e = scan_prototypes(zq_p && featq && spx && mask && bits && work && labels && weight, zq_p, Ch, h, w, spx, spx_dtype, mask, bits, N,
                                C, H, W, S, invT, weight_flags_ok(flags), work, work_bytes, nullptr, stream, &gmax))
        return e;
    const Geo g = make_geo(C, Ch, h, w, H, W, S);
    const long long total = (long long)N * H * W;
    const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
    return for_class_count(C, [&](auto ct, auto exact) {
        return for_id_type(spx, spx_dtype, [&](auto ids) {
            hipLaunchKernelGGL((k_online_assign<decltype(ct)::value, decltype(exact)::value>), grid, dim3(kThreads), 0,
                               static_cast<hipStream_t>(stream), zq_p, featq, ids, mask, bits, gmax, g, total, invT, flags, labels, weight);
            return mas_launch_status();
        });
    });
}

extern "C" int mas_online_soft_weights(const float* zq_p, const float* featq, int Ch, int h, int w, const void* spx, int spx_dtype,
                                       const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, float invT, float invtau,
                                       void* work, size_t work_bytes, float* softw, int32_t* live, void* stream) {
    const mas_u64* gmax;
    if (int e = scan_prototypes(zq_p && featq && spx && mask && bits && work && softw && live, zq_p, Ch, h, w, spx, spx_dtype, mask, bits, N, C,
                                H, W, S, invT, invtau > 0.0f, work, work_bytes, live, stream, &gmax))
        return e;
    const Geo g = make_geo(C, Ch, h, w, H, W, S);
    const long long total = (long long)N * H * W;
    const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
    return for_id_type(spx, spx_dtype, [&](auto ids) {
        hipLaunchKernelGGL(k_online_soft, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), featq, ids, mask, bits, gmax, g, total,
                           invtau, softw, live);
        return mas_launch_status();
    });
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
    return ce_forward(label_ce(zq, h, w, labels, weight, C, H, W, invT, flags, th), N, acc, flags, loss, stream);
}

extern "C" int mas_label_ce_bwd_lowres(const float* zq, int h, int w, const uint8_t* labels, const float* weight, const uint64_t* acc,
                                       const float* grad, int N, int C, int H, int W, float invT, int flags, float th, int64_t* dzq_fix,
                                       float* dzq, void* stream) {
    if (!acc || !grad || !dzq_fix) return MAS_ERR_NULL;
    if (int e = check_ce(zq, labels, weight, N, C, h, w, H, W, flags)) return e;
    return ce_backward(label_ce(zq, h, w, labels, weight, C, H, W, invT, flags, th), N, acc, grad, dzq_fix, dzq, stream);
}

extern "C" int mas_soft_ce_fwd_lowres(const float* zq, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits,
                                      const float* softw, const int32_t* live, int N, int C, int H, int W, int S, float invT, uint64_t* acc,
                                      float* loss, void* stream) {
    if (!acc) return MAS_ERR_NULL;
    if (int e = check_soft(zq, spx, spx_dtype, mask, bits, softw, live, N, C, h, w, H, W, S)) return e;
    return ce_forward(SoftCe{zq, spx, mask, bits, softw, live, make_geo(C, 0, h, w, H, W, S), invT, spx_dtype, 0, 0}, N, acc, 0, loss, stream);
}

extern "C" int mas_soft_ce_bwd_lowres(const float* zq, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits,
                                      const float* softw, const int32_t* live, const uint64_t* acc, const float* grad, int N, int C, int H,
                                      int W, int S, float invT, int64_t* dzq_fix, float* dzq, void* stream) {
    if (!acc || !grad || !dzq_fix) return MAS_ERR_NULL;
    if (int e = check_soft(zq, spx, spx_dtype, mask, bits, softw, live, N, C, h, w, H, W, S)) return e;
    return ce_backward(SoftCe{zq, spx, mask, bits, softw, live, make_geo(C, 0, h, w, H, W, S), invT, spx_dtype, 0, 0}, N, acc, grad, dzq_fix,
                       dzq, stream);
}

// ---- the CPU-side statement: host pointers, plain loops through online_plbl.h.  No device is touched. ---------------------------------
namespace {
long long host_id(const void* spx, int spx_dtype, size_t i) {
    if (spx_dtype == MAS_ID_I64) return static_cast<const long long*>(spx)[i];
    if (spx_dtype == MAS_ID_I32) return static_cast<const int*>(spx)[i];
    return static_cast<const unsigned short*>(spx)[i];
}

// bits[n, id] of a valid pixel (mask set, id in range, at least min_bits bits: more than one for the prototypes), 0 otherwise
uint32_t host_valid_bits(const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits, int n, int S, size_t g, long long* id,
                         int min_bits = 2) {
    if (!mask[g]) return 0;
    *id = (int)host_id(spx, spx_dtype, g);         // (the kernels' mas_load_id)
    if (*id < 0 || *id >= S) return 0;
    const uint32_t Y = bits[(size_t)n * S + (size_t)*id];
    return __builtin_popcount(Y) >= min_bits ? Y : 0;
}

// the arg-pixel table [N,S,C] of the valid pixels (what the group scan leaves)
void host_table(const float* zq_p, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits, int N, int C, int H,
                int W, int S, float invT, uint64_t* table, int min_bits = 2) {
    const size_t HW = (size_t)H * W, hw = (size_t)h * w;
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    for (size_t i = 0; i < (size_t)N * S * C; ++i) table[i] = 0;
    for (int n = 0; n < N; ++n) {
        for (size_t pix = 0; pix < HW; ++pix) {
            const size_t gi = (size_t)n * HW + pix;
            long long id = 0;
            const uint32_t Y = host_valid_bits(spx, spx_dtype, mask, bits, n, S, gi, &id, min_bits);
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

// The host's policies: what LabelCe and SoftCe say, said again on host pointers.  takes(n, i): pixel i of [N,H,W], in picture n, is one
// the loss looks at; pixel(n, i, p, s, term): its state and term from its probabilities p, true when it is counted.
struct HostLabelCe {
    const uint8_t* labels; const float* weight; int C, mode; float th; int sgn;
    struct Px { int lab; float wgt; };

    bool takes(int, size_t i) const { return labels[i] < C; }
    bool pixel(int, size_t i, const float (&p)[MAS_MAX_CLASSES], Px& s, float& term) const {
        s.lab = labels[i];
        s.wgt = mas_opl_mode_weight(mode, mode == MAS_LCE_UNWEIGHTED ? 1.0f : weight[i], th);
        int counted;
        term = mas_opl_term(mode, s.wgt, mas_opl_ce(p[s.lab]), &counted);
        return counted != 0;
    }
    uint64_t fix(float term) const { return mas_opl_fix_term(term, sgn); }
    uint64_t count(const Px&) const { return 1; }
    float scale(float grad, uint64_t n, float invT) const { return (grad / (float)n) * invT; }
    float value(uint64_t sum, uint64_t n, int flags) const { return mas_opl_value(sum, n, flags); }
    float k(const Px& s, float scale) const { return scale * s.wgt; }
    float dir(const Px& s, int c, float pc) const { return pc - ((c == s.lab) ? 1.0f : 0.0f); }
};

struct HostSoftCe {
    const void* spx; int spx_dtype; const uint8_t* mask; const uint32_t* bits; const float* softw; const int32_t* live;
    int C, S; size_t HW;
    struct Px { uint32_t Yc; int multi; const float* sw; float A; };

    bool takes(int n, size_t i) const {
        if (!live[n] || !mask[i]) return false;
        const long long id = (int)host_id(spx, spx_dtype, i);
        return id >= 0 && id < S;
    }
    bool pixel(int n, size_t i, const float (&p)[MAS_MAX_CLASSES], Px& s, float& term) const {
        s.Yc = mas_opl_cands(bits[(size_t)n * S + (size_t)(int)host_id(spx, spx_dtype, i)], C, &s.multi);
        s.sw = softw + (size_t)n * C * HW + (i - (size_t)n * HW);
        term = mas_opl_soft_term<MAS_MAX_CLASSES>(p, C, s.Yc, s.multi, s.sw, HW, &s.A);
        return true;
    }
    uint64_t fix(float term) const { return mas_fix(term, MAS_LOSS_FRAC_BITS); }
    uint64_t count(const Px&) const { return 1; }
    float scale(float grad, uint64_t n, float invT) const { return (grad / (float)n) * invT; }
    float value(uint64_t sum, uint64_t n, int flags) const { return mas_opl_value(sum, n, flags); }
    float k(const Px&, float scale) const { return scale; }
    float dir(const Px& s, int c, float pc) const {
        const int in_y = (int)((s.Yc >> c) & 1u);
        return mas_opl_soft_dir(pc, s.A, in_y, (in_y && s.multi) ? s.sw[(size_t)c * HW] : 1.0f);
    }
};

struct HostHierCe {
    const void* small; int small_dtype; const uint8_t* mask; const uint32_t* mult; const uint32_t* any; int C, Ss;
    struct Px { uint32_t Yc; const uint32_t* m; float U; uint32_t cnt; };

    bool takes(int n, size_t i) const {
        if (!mask[i]) return false;
        const long long id = (int)host_id(small, small_dtype, i);
        return id >= 0 && id < Ss && any[(size_t)n * Ss + (size_t)id] != 0u;
    }
    bool pixel(int n, size_t i, const float (&p)[MAS_MAX_CLASSES], Px& s, float& term) const {
        const size_t row = (size_t)n * Ss + (size_t)(int)host_id(small, small_dtype, i);
        s.Yc = C < 32 ? (any[row] & ((1u << C) - 1u)) : any[row];
        s.m = mult + row * C;
        term = mas_hg_term<MAS_MAX_CLASSES>(p, C, s.Yc, s.m, &s.U, &s.cnt);
        return true;
    }
    uint64_t fix(float term) const { return mas_fix(term, MAS_LOSS_FRAC_BITS); }
    uint64_t count(const Px& s) const { return s.cnt; }
    float scale(float grad, uint64_t n, float) const { return mas_hg_scale(grad, n); }
    float value(uint64_t sum, uint64_t n, int) const { return mas_hg_value(sum, n); }
    float k(const Px&, float scale) const { return scale; }
    float dir(const Px& s, int c, float pc) const { return mas_hg_dir(pc, s.U, ((s.Yc >> c) & 1u) ? (float)s.m[c] : 0.0f); }
};

// pass 0 counts and sums the terms of the counted pixels; pass 1, with dzq_fix, scatters their gradient through the four taps
template <typename P>
void host_ce(const P& a, const float* zq, const Geo& g, int N, float invT, int value_flags, const float* grad, uint64_t* acc, float* loss,
             int64_t* dzq_fix) {
    const size_t HW = (size_t)g.H * g.W, hw = (size_t)g.h * g.w;
    acc[0] = acc[1] = 0;
    for (int pass = 0; pass < (dzq_fix ? 2 : 1); ++pass) {
        float scale = 0.0f;
        if (pass == 1) {
            scale = a.scale(grad[0], acc[1], invT);
            for (size_t i = 0; i < (size_t)N * g.C * hw; ++i) dzq_fix[i] = 0;
        }
        for (int n = 0; n < N; ++n) {
            for (size_t pix = 0; pix < HW; ++pix) {
                const size_t gi = (size_t)n * HW + pix;
                if (!a.takes(n, gi)) continue;
                const OplTap t = mas_opl_tap(g.sh, g.sw, (int)(pix / g.W), (int)(pix % g.W), g.h, g.w);
                float p[MAS_MAX_CLASSES];
                mas_opl_logits<MAS_MAX_CLASSES>(zq + (size_t)n * g.C * hw, hw, t, g.C, p);
                mas_opl_softmax<MAS_MAX_CLASSES>(p, g.C, invT);
                typename P::Px s;
                float term;
                if (!a.pixel(n, gi, p, s, term)) continue;
                if (pass == 0) {
                    acc[0] += a.fix(term);
                    acc[1] += a.count(s);
                    continue;
                }
                const float k = a.k(s, scale);
                const float w00 = t.l0h * t.l0w, w01 = t.l0h * t.l1w, w10 = t.l1h * t.l0w, w11 = t.l1h * t.l1w;
                for (int c = 0; c < g.C; ++c) {
                    int64_t* q = dzq_fix + ((size_t)n * g.C + c) * hw;
                    const float d = k * a.dir(s, c, p[c]);
                    q[t.o00] += mas_opl_grad_fix(d * w00);
                    q[t.o01] += mas_opl_grad_fix(d * w01);
                    q[t.o10] += mas_opl_grad_fix(d * w10);
                    q[t.o11] += mas_opl_grad_fix(d * w11);
                }
            }
        }
        if (pass == 0 && loss) loss[0] = a.value(acc[0], acc[1], value_flags);
    }
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
    host_ce(HostLabelCe{labels, weight, C, ce_flags & 3, th, (ce_flags & MAS_LCE_SIGNED) ? 1 : 0}, zq, g, N, invT_ce, ce_flags, grad, acc, loss,
            dzq_fix);
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
    host_ce(HostSoftCe{spx, spx_dtype, mask, bits, softw, live, C, S, HW}, zq, g, N, invT_ce, 0, grad, acc, loss, dzq_fix);
    return 0;
}

// ---- the hierarchical group term (hier_group.h) ---------------------------------------------------------------------------------------
namespace {
int check_hier(const float* zq, const void* small, int small_dtype, const uint8_t* mask, const uint32_t* mult, const uint32_t* any,
               const uint64_t* acc, int N, int C, int h, int w, int H, int W, int Ss) {
    if (!zq || !small || !mask || !mult || !any || !acc) return MAS_ERR_NULL;
    if (Ss <= 0) return MAS_ERR_SHAPE;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    if (!id_dtype_ok(small_dtype)) return MAS_ERR_DTYPE;
    if ((uintptr_t)mult % 4 != 0 || (uintptr_t)any % 4 != 0 || (uintptr_t)acc % 8 != 0) return MAS_ERR_ALIGN;
    return 0;
}

HierCe hier_ce(const float* zq, int h, int w, const void* small, int small_dtype, const uint8_t* mask, const uint32_t* mult,
               const uint32_t* any, int C, int H, int W, int Ss) {
    return HierCe{zq, small, mask, mult, any, make_geo(C, 0, h, w, H, W, Ss), small_dtype, 0, 0};
}
}  // namespace

extern "C" int mas_hier_group_value(const uint64_t* acc, float* loss, void* stream) {
    if (!acc || !loss) return MAS_ERR_NULL;
    hipLaunchKernelGGL(k_hier_value, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const mas_u64*>(acc), loss);
    return mas_launch_status();
}

extern "C" int mas_hier_group_fwd(const float* zq, int h, int w, const void* spx, int spx_dtype, const void* small, int small_dtype,
                                  const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, int Ss, int flags, void* work,
                                  size_t work_bytes, uint32_t* bits_eff, uint32_t* mult, uint32_t* any, uint64_t* acc, float* loss,
                                  void* stream) {
    if (!spx || !bits || !work) return MAS_ERR_NULL;
    if (int e = check_hier(zq, small, small_dtype, mask, mult, any, acc, N, C, h, w, H, W, Ss)) return e;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (flags & ~(MAS_HIER_ONLY_MULTI | MAS_HIER_NOCROPSP)) return MAS_ERR_RANGE;
    if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
    const bool clear = (flags & MAS_HIER_NOCROPSP) != 0;
    if (clear && !bits_eff) return MAS_ERR_NULL;
    if (clear && (uintptr_t)bits_eff % 4 != 0) return MAS_ERR_ALIGN;
    const size_t need = mas_online_plbl_work_bytes(N, S, C);
    if (work_bytes < need) return MAS_ERR_WORKSPACE;
    if ((uintptr_t)work % 8 != 0) return MAS_ERR_ALIGN;
    const long long words = (long long)N * S * C;
    if (words > 0x7fffffffLL * kThreads || (long long)N * Ss * C > 0x7fffffffLL) return MAS_ERR_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t me = hipMemsetAsync(work, 0, need, st);
    if (me == hipSuccess) me = hipMemsetAsync(mult, 0, (size_t)N * Ss * C * sizeof(uint32_t), st);
    if (me == hipSuccess) me = hipMemsetAsync(any, 0, (size_t)N * Ss * sizeof(uint32_t), st);
    if (me == hipSuccess) me = hipMemsetAsync(acc, 0, 2 * sizeof(uint64_t), st);
    if (me == hipSuccess && clear) me = hipMemcpyAsync(bits_eff, bits, (size_t)N * S * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (me != hipSuccess) return (int)me;
    if (clear) {
        const long long lanes = (long long)N * (2 * W + 2 * H);
        hipLaunchKernelGGL(k_clear_boundary_bits, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, spx, spx_dtype, N,
                           H, W, S, bits_eff);
        if (int e = mas_launch_status()) return e;
    }
    uint64_t* scan_acc = static_cast<uint64_t*>(work);
    if (int e = mas_partial_loss_fwd_lowres(zq, h, w, spx, spx_dtype, mask, clear ? bits_eff : bits, N, C, H, W, S, 1.0f,
                                            MAS_LOSS_GROUP | ((flags & MAS_HIER_ONLY_MULTI) ? MAS_LOSS_GROUP_ONLY_MULTI : 0), scan_acc + 8,
                                            scan_acc, stream))
        return e;
    hipLaunchKernelGGL(k_hier_pairs, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       reinterpret_cast<const mas_u64*>(scan_acc + 8), small, small_dtype, words, S, C, H * W, Ss, mult, any);
    if (int e = mas_launch_status()) return e;
    if (int e = launch_ce(hier_ce(zq, h, w, small, small_dtype, mask, mult, any, C, H, W, Ss), N, nullptr, nullptr,
                          reinterpret_cast<mas_u64*>(acc), st))
        return e;
    return loss ? mas_hier_group_value(acc, loss, stream) : 0;
}

extern "C" int mas_hier_group_bwd(const float* zq, int h, int w, const void* small, int small_dtype, const uint8_t* mask,
                                  const uint32_t* mult, const uint32_t* any, const uint64_t* acc, const float* grad, int N, int C, int H,
                                  int W, int Ss, int64_t* dzq_fix, float* dzq, void* stream) {
    if (!grad || !dzq_fix) return MAS_ERR_NULL;
    if (int e = check_hier(zq, small, small_dtype, mask, mult, any, acc, N, C, h, w, H, W, Ss)) return e;
    return ce_backward(hier_ce(zq, h, w, small, small_dtype, mask, mult, any, C, H, W, Ss), N, acc, grad, dzq_fix, dzq, stream);
}

extern "C" int mas_hier_group_reference(const float* zq, int h, int w, const void* spx, int spx_dtype, const void* small, int small_dtype,
                                        const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, int Ss, int flags,
                                        const float* grad, uint64_t* gmax, uint32_t* bits_eff, uint32_t* mult, uint32_t* any, uint64_t* acc,
                                        float* loss, int64_t* dzq_fix) {
    if (!spx || !bits) return MAS_ERR_NULL;
    if (int e = check_hier(zq, small, small_dtype, mask, mult, any, acc, N, C, h, w, H, W, Ss)) return e;
    if (S <= 0) return MAS_ERR_SHAPE;
    if (flags & ~(MAS_HIER_ONLY_MULTI | MAS_HIER_NOCROPSP)) return MAS_ERR_RANGE;
    if (!id_dtype_ok(spx_dtype)) return MAS_ERR_DTYPE;
    const bool clear = (flags & MAS_HIER_NOCROPSP) != 0;
    if (clear && !bits_eff) return MAS_ERR_NULL;
    if (dzq_fix && !grad) return MAS_ERR_NULL;
    const size_t HW = (size_t)H * W;
    if (clear) {
        for (size_t i = 0; i < (size_t)N * S; ++i) bits_eff[i] = bits[i];
        for (int n = 0; n < N; ++n) {
            for (size_t pix = 0; pix < HW; ++pix) {
                const int y = (int)(pix / W), x = (int)(pix % W);
                if (y != 0 && y != H - 1 && x != 0 && x != W - 1) continue;
                const long long id = (int)host_id(spx, spx_dtype, (size_t)n * HW + pix);
                if (id >= 0 && id < S) bits_eff[(size_t)n * S + (size_t)id] = 0u;
            }
        }
        bits = bits_eff;
    }
    uint64_t* table = gmax ? gmax : new uint64_t[(size_t)N * S * C];
    host_table(zq, h, w, spx, spx_dtype, mask, bits, N, C, H, W, S, 1.0f, table, (flags & MAS_HIER_ONLY_MULTI) ? 2 : 1);
    for (size_t i = 0; i < (size_t)N * Ss * C; ++i) mult[i] = 0;
    for (size_t i = 0; i < (size_t)N * Ss; ++i) any[i] = 0;
    for (size_t i = 0; i < (size_t)N * S * C; ++i) {
        if ((table[i] >> 32) == 0) continue;
        const uint32_t pp = mas_opl_word_pixel(table[i]);
        if (pp >= (uint32_t)HW) continue;
        const size_t n = i / ((size_t)S * C);
        const int c = (int)(i % C);
        const long long id = (int)host_id(small, small_dtype, n * HW + pp);
        if (id < 0 || id >= Ss) continue;
        mult[(n * Ss + (size_t)id) * C + c] += 1;
        any[n * Ss + (size_t)id] |= 1u << c;
    }
    if (!gmax) delete[] table;
    host_ce(HostHierCe{small, small_dtype, mask, mult, any, C, Ss}, zq, make_geo(C, 0, h, w, H, W, Ss), N, 1.0f, 0, grad, acc, loss, dzq_fix);
    return 0;
}

// ---- the cross-view forms (hier_group.h): tables from the weak view, the sum over the strong view ---------------------------------------
namespace {
struct HostWHierCe {
    const void* small; int small_dtype; const uint8_t* mask; const uint32_t* mult; const uint32_t* any; const float* wgt; int C, Ss;
    struct Px { uint32_t Yc; const uint32_t* m; const float* wg; float U; uint32_t cnt; };

    bool takes(int n, size_t i) const {
        if (!mask[i]) return false;
        const long long id = (int)host_id(small, small_dtype, i);
        return id >= 0 && id < Ss && any[(size_t)n * Ss + (size_t)id] != 0u;
    }
    bool pixel(int n, size_t i, const float (&p)[MAS_MAX_CLASSES], Px& s, float& term) const {
        const size_t row = (size_t)n * Ss + (size_t)(int)host_id(small, small_dtype, i);
        s.Yc = C < 32 ? (any[row] & ((1u << C) - 1u)) : any[row];
        s.m = mult + row * C;
        s.wg = wgt + row * C;
        term = mas_ahg_term<MAS_MAX_CLASSES>(p, C, s.Yc, s.m, s.wg, &s.U, &s.cnt);
        return true;
    }
    uint64_t fix(float term) const { return mas_fix(term, MAS_LOSS_FRAC_BITS); }
    uint64_t count(const Px& s) const { return s.cnt; }
    float scale(float grad, uint64_t n, float) const { return mas_hg_scale(grad, n); }
    float value(uint64_t sum, uint64_t n, int) const { return mas_hg_value(sum, n); }
    float k(const Px&, float scale) const { return scale; }
    float dir(const Px& s, int c, float pc) const { return mas_hg_dir(pc, s.U, ((s.Yc >> c) & 1u) ? (float)s.m[c] * s.wg[c] : 0.0f); }
};

bool weight_mode_ok(int mode) { return mode == MAS_AHG_WEIGHT_NONE || mode == MAS_AHG_WEIGHT_MAX || mode == MAS_AHG_WEIGHT_MEAN; }

int check_weight(const float* wgt) { return (wgt && (uintptr_t)wgt % 4 != 0) ? MAS_ERR_ALIGN : 0; }
}  // namespace

extern "C" size_t mas_async_hier_work_bytes(int N, int S, int Ss, int C, int mode) {
    if (N <= 0 || S <= 0 || Ss <= 0 || C <= 0) return 0;
    size_t words = 8 + (size_t)N * S * C;                                           // the scan's eight words and its table
    if (mode == MAS_AHG_WEIGHT_MEAN) words += (size_t)N * Ss * C + ((size_t)N * Ss + 1) / 2;      // u64 sums, then u32 pixel counts
    return words * sizeof(mas_u64);
}

extern "C" int mas_async_hier_tables(const float* zq, int h, int w, const void* spx, int spx_dtype, const void* small, int small_dtype,
                                     const uint8_t* mask, const uint32_t* bits, int N, int C, int H, int W, int S, int Ss, int mode, void* work,
                                     size_t work_bytes, uint32_t* mult, uint32_t* any, float* wgt, void* stream) {
    if (!zq || !spx || !small || !mask || !bits || !work || !mult || !any) return MAS_ERR_NULL;
    if (S <= 0 || Ss <= 0) return MAS_ERR_SHAPE;
    if (int e = check_geometry(N, C, h, w, H, W)) return e;
    if (!weight_mode_ok(mode)) return MAS_ERR_RANGE;
    if (!id_dtype_ok(spx_dtype) || !id_dtype_ok(small_dtype)) return MAS_ERR_DTYPE;
    if (mode != MAS_AHG_WEIGHT_NONE && !wgt) return MAS_ERR_NULL;
    const size_t need = mas_async_hier_work_bytes(N, S, Ss, C, mode);
    if (work_bytes < need) return MAS_ERR_WORKSPACE;
    if ((uintptr_t)work % 8 != 0 || (uintptr_t)mult % 4 != 0 || (uintptr_t)any % 4 != 0) return MAS_ERR_ALIGN;
    if (int e = check_weight(wgt)) return e;
    const long long words = (long long)N * S * C, pairs = (long long)N * Ss * C;
    if (words > 0x7fffffffLL * kThreads || pairs > 0x7fffffffLL) return MAS_ERR_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t me = hipMemsetAsync(work, 0, need, st);
    if (me == hipSuccess) me = hipMemsetAsync(mult, 0, (size_t)pairs * sizeof(uint32_t), st);
    if (me == hipSuccess) me = hipMemsetAsync(any, 0, (size_t)N * Ss * sizeof(uint32_t), st);
    if (me == hipSuccess && mode != MAS_AHG_WEIGHT_NONE) me = hipMemsetAsync(wgt, 0, (size_t)pairs * sizeof(float), st);
    if (me != hipSuccess) return (int)me;
    uint64_t* scan_acc = static_cast<uint64_t*>(work);
    if (int e = mas_partial_loss_fwd_lowres(zq, h, w, spx, spx_dtype, mask, bits, N, C, H, W, S, 1.0f, MAS_LOSS_GROUP, scan_acc + 8, scan_acc,
                                            stream))
        return e;
    hipLaunchKernelGGL(k_hier_pairs, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       reinterpret_cast<const mas_u64*>(scan_acc + 8), small, small_dtype, words, S, C, H * W, Ss, mult, any);
    if (int e = mas_launch_status()) return e;
    if (mode == MAS_AHG_WEIGHT_NONE) return 0;
    const bool mean = mode == MAS_AHG_WEIGHT_MEAN;
    mas_u64* wsum = reinterpret_cast<mas_u64*>(scan_acc + 8 + words);
    unsigned* wcnt = reinterpret_cast<unsigned*>(wsum + pairs);
    const Geo g = make_geo(C, 0, h, w, H, W, Ss);
    const long long total = (long long)N * H * W;
    const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
    if (int e = for_class_count(C, [&](auto ct, auto exact) {
            constexpr int CT = decltype(ct)::value;
            constexpr bool EXACT = decltype(exact)::value;
            if (mean)
                hipLaunchKernelGGL((k_hier_weights<CT, EXACT, true>), grid, dim3(kThreads), 0, st, zq, small, small_dtype, mask, any, g, total,
                                   (unsigned*)nullptr, wsum, wcnt);
            else
                hipLaunchKernelGGL((k_hier_weights<CT, EXACT, false>), grid, dim3(kThreads), 0, st, zq, small, small_dtype, mask, any, g, total,
                                   reinterpret_cast<unsigned*>(wgt), (mas_u64*)nullptr, (unsigned*)nullptr);
            return mas_launch_status();
        }))
        return e;
    if (!mean) return 0;
    hipLaunchKernelGGL(k_hier_weights_mean, dim3((unsigned)((pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, wsum, wcnt, any, pairs, C,
                       wgt);
    return mas_launch_status();
}

extern "C" int mas_async_hier_value(const uint64_t* acc, float* loss, void* stream) { return mas_hier_group_value(acc, loss, stream); }

extern "C" int mas_async_hier_fwd(const float* zq, int h, int w, const void* small, int small_dtype, const uint8_t* mask, const uint32_t* mult,
                                  const uint32_t* any, const float* wgt, int N, int C, int H, int W, int Ss, uint64_t* acc, float* loss,
                                  void* stream) {
    if (int e = check_hier(zq, small, small_dtype, mask, mult, any, acc, N, C, h, w, H, W, Ss)) return e;
    if (int e = check_weight(wgt)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t me = hipMemsetAsync(acc, 0, 2 * sizeof(uint64_t), st);
    if (me != hipSuccess) return (int)me;
    const int e = wgt ? launch_ce(WHierCe{zq, small, mask, mult, any, wgt, make_geo(C, 0, h, w, H, W, Ss), small_dtype, 0, 0}, N, nullptr, nullptr,
                                  reinterpret_cast<mas_u64*>(acc), st)
                      : launch_ce(hier_ce(zq, h, w, small, small_dtype, mask, mult, any, C, H, W, Ss), N, nullptr, nullptr,
                                  reinterpret_cast<mas_u64*>(acc), st);
    if (e) return e;
    return loss ? mas_hier_group_value(acc, loss, stream) : 0;
}

extern "C" int mas_async_hier_bwd(const float* zq, int h, int w, const void* small, int small_dtype, const uint8_t* mask, const uint32_t* mult,
                                  const uint32_t* any, const float* wgt, const uint64_t* acc, const float* grad, int N, int C, int H, int W,
                                  int Ss, int64_t* dzq_fix, float* dzq, void* stream) {
    if (!grad || !dzq_fix) return MAS_ERR_NULL;
    if (int e = check_hier(zq, small, small_dtype, mask, mult, any, acc, N, C, h, w, H, W, Ss)) return e;
    if (int e = check_weight(wgt)) return e;
    if (wgt)
        return ce_backward(WHierCe{zq, small, mask, mult, any, wgt, make_geo(C, 0, h, w, H, W, Ss), small_dtype, 0, 0}, N, acc, grad, dzq_fix,
                           dzq, stream);
    return ce_backward(hier_ce(zq, h, w, small, small_dtype, mask, mult, any, C, H, W, Ss), N, acc, grad, dzq_fix, dzq, stream);
}

extern "C" int mas_async_hier_reference(const float* zq_weak, int h_o, int w_o, const void* spx_weak, int spx_dtype, const void* small_weak,
                                        int small_weak_dtype, const uint8_t* mask_weak, const uint32_t* bits, int H_o, int W_o, int S, int mode,
                                        const float* zq, int h, int w, const void* small, int small_dtype, const uint8_t* mask, int N, int C,
                                        int H, int W, int Ss, const float* grad, uint64_t* gmax, uint32_t* mult, uint32_t* any, float* wgt,
                                        uint64_t* acc, float* loss, int64_t* dzq_fix) {
    const bool given = (mode & MAS_AHG_TABLES_GIVEN) != 0;
    const int wmode = mode & ~MAS_AHG_TABLES_GIVEN;
    if (!weight_mode_ok(wmode)) return MAS_ERR_RANGE;
    if (int e = check_hier(zq, small, small_dtype, mask, mult, any, acc, N, C, h, w, H, W, Ss)) return e;
    if (wmode != MAS_AHG_WEIGHT_NONE && !wgt) return MAS_ERR_NULL;
    if (int e = check_weight(wgt)) return e;
    if (dzq_fix && !grad) return MAS_ERR_NULL;
    if (!given) {
        if (!zq_weak || !spx_weak || !small_weak || !mask_weak || !bits) return MAS_ERR_NULL;
        if (S <= 0) return MAS_ERR_SHAPE;
        if (int e = check_geometry(N, C, h_o, w_o, H_o, W_o)) return e;
        if (!id_dtype_ok(spx_dtype) || !id_dtype_ok(small_weak_dtype)) return MAS_ERR_DTYPE;
        const size_t HWo = (size_t)H_o * W_o, hwo = (size_t)h_o * w_o, pairs = (size_t)N * Ss * C;
        uint64_t* table = gmax ? gmax : new uint64_t[(size_t)N * S * C];
        host_table(zq_weak, h_o, w_o, spx_weak, spx_dtype, mask_weak, bits, N, C, H_o, W_o, S, 1.0f, table, 1);
        for (size_t i = 0; i < pairs; ++i) mult[i] = 0;
        for (size_t i = 0; i < (size_t)N * Ss; ++i) any[i] = 0;
        for (size_t i = 0; i < (size_t)N * S * C; ++i) {
            if ((table[i] >> 32) == 0) continue;
            const uint32_t pp = mas_opl_word_pixel(table[i]);
            if (pp >= (uint32_t)HWo) continue;
            const size_t n = i / ((size_t)S * C);
            const int c = (int)(i % C);
            const long long id = (int)host_id(small_weak, small_weak_dtype, n * HWo + pp);
            if (id < 0 || id >= Ss) continue;
            mult[(n * Ss + (size_t)id) * C + c] += 1;
            any[n * Ss + (size_t)id] |= 1u << c;
        }
        if (!gmax) delete[] table;
        if (wmode != MAS_AHG_WEIGHT_NONE) {
            const bool mean = wmode == MAS_AHG_WEIGHT_MEAN;
            uint64_t* wsum = new uint64_t[pairs]();
            uint32_t* wcnt = new uint32_t[(size_t)N * Ss]();
            uint32_t* wbits = reinterpret_cast<uint32_t*>(wgt);
            for (size_t i = 0; i < pairs; ++i) wbits[i] = 0u;
            const float sh = (float)h_o / (float)H_o, sw = (float)w_o / (float)W_o;
            for (int n = 0; n < N; ++n) {
                for (size_t pix = 0; pix < HWo; ++pix) {
                    const size_t gi = (size_t)n * HWo + pix;
                    if (!mask_weak[gi]) continue;
                    const long long id = (int)host_id(small_weak, small_weak_dtype, gi);
                    if (id < 0 || id >= Ss) continue;
                    const size_t row = (size_t)n * Ss + (size_t)id;
                    const uint32_t Yc = C < 32 ? (any[row] & ((1u << C) - 1u)) : any[row];
                    if (!Yc) continue;
                    const OplTap t = mas_opl_tap(sh, sw, (int)(pix / W_o), (int)(pix % W_o), h_o, w_o);
                    float p[MAS_MAX_CLASSES];
                    mas_opl_logits<MAS_MAX_CLASSES>(zq_weak + (size_t)n * C * hwo, hwo, t, C, p);
                    mas_opl_softmax<MAS_MAX_CLASSES>(p, C, 1.0f);
                    if (mean) wcnt[row] += 1;
                    for (int c = 0; c < C; ++c) {
                        if (!((Yc >> c) & 1u)) continue;
                        if (mean) wsum[row * C + c] += mas_ahg_fix(p[c]);
                        else if (mas_f2u(p[c]) > wbits[row * C + c]) wbits[row * C + c] = mas_f2u(p[c]);
                    }
                }
            }
            if (mean) {
                for (size_t i = 0; i < pairs; ++i) {
                    const size_t row = i / C;
                    if (wcnt[row] != 0u && ((any[row] >> (i % C)) & 1u)) wgt[i] = mas_ahg_mean(wsum[i], wcnt[row]);
                }
            }
            delete[] wsum;
            delete[] wcnt;
        }
    }
    const Geo g = make_geo(C, 0, h, w, H, W, Ss);
    if (wmode != MAS_AHG_WEIGHT_NONE) host_ce(HostWHierCe{small, small_dtype, mask, mult, any, wgt, C, Ss}, zq, g, N, 1.0f, 0, grad, acc, loss, dzq_fix);
    else host_ce(HostHierCe{small, small_dtype, mask, mult, any, C, Ss}, zq, g, N, 1.0f, 0, grad, acc, loss, dzq_fix);
    return 0;
}
