// losses.hip -- stage-1 partial-label losses (K5 merged-positive CE, K6 group/MIL max-pool CE) for gfx950.
//
//   k_target_bits        multi-hot target rows u8[rows, cols] -> one u32 bit mask per superpixel.
//   k_partial_loss_fwd   ONE streaming pass over mask + ids (+ logits of the selected pixels only):
//                        per-pixel softmax in registers, fixed-point CE sums, and the segmented
//                        per-(superpixel, class) max with arg-pixel through a per-workgroup LDS table
//                        of packed (prob bits << 32 | ~pixel) words combined with 64-bit atomic max.
//   k_group_finalize     -log(max + eps) over the (superpixel, class) table.
//   k_loss_values_weighted   fixed-point sums -> the reference's mean-normalised f32 losses (with weights: and their weighted sum).
//   k_loss_scales_weighted   upstream gradients / (1 + n) -> per-loss scale factors (no host sync).
//   k_partial_loss_bwd   one pass writing dz[N,C,H,W] completely (zeros off-mask), softmax recomputed,
//                        group-loss gradient gathered from the arg-pixel table (no atomics).
//   PLX instantiations of both scans: the multi-hot pixel term is the risk-consistent (MAS_LOSS_RC) or the top-1 candidate
//                        (MAS_LOSS_TOPONE) formula of partial_label.h instead of the merged positive; chosen at launch, so the
//                        merged-positive kernels carry nothing of it.
//   mas_partial_loss_reference   the CE-family sums and dz on HOST pointers, a plain loop through partial_label.h.
//   the TT instantiations of both scans    the same two scan bodies with a fourth loss slot: the teacher-gated top-1 term (a second logit plane,
//                        the eval-mode teacher's, read with the same taps / at the same address) or the candidate entropy of
//                        teacher_terms.h, beside the merged-positive and group terms.  Kernels of their own, so every
//                        k_partial_loss_* instantiation compiles to what it was.
//   mas_teacher_loss_reference   all four terms (the group table included) and dz on HOST pointers.
//   the MAS_TT_WGROUP instantiations       the same two scan bodies with the TEACHER-WEIGHTED group term (teacher_terms.h, wgroup): a pixel
//                        that contributes to the group table also soft-maxes the teacher's row and raises a second, u32 table `tmax`
//                        [N,S,C] of the teacher's per-(superpixel, class) maximum (LDS table beside the student's, same slot keys, same
//                        overflow path); k_group_finalize<true> weights every entry's -log by it, the backward's arg-pixel gather
//                        reads it.  No fourth slot, eight accumulator words.
//   mas_wgroup_loss_reference    the same on HOST pointers, both tables included.
//
// Reference semantics: trainer/active_joint_multi_predignore_lossdecomp.py:21-72 (OnehotCEMultihotChoice),
// trainer/active_joint_multi_predignore_mclossablation2.py:22-79 (GroupMultiLabelCE_onlymulti),
// trainer/active_joint_multi_predignore.py:21-128, utils/loss.py:91-141,543-588 (base classes).
#include "common.h"
#include "partial_label.h"
#include "teacher_terms.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 256;
constexpr int kTileH = 4;
constexpr int kLogSlots = 6;
constexpr int kSlots = 1 << kLogSlots;

// accumulator slots of the u64 `acc` array
enum { ACC_SUM_CE = 0, ACC_SUM_MC = 1, ACC_N_CE = 2, ACC_N_MC = 3, ACC_N_EMPTY = 4, ACC_SUM_GROUP = 5, ACC_N_GROUP = 6 };
// the teacher-term scans use a 16-word accumulator: word 7 stays the fused forward's arrival counter, 8 / 9 are the fourth loss slot
enum { ACC_SUM_X = 8, ACC_N_X = 9 };

// what the teacher-term kernels take beside the arguments of the plain scans (teacher_terms.h); TT == MAS_TT_NONE bodies never read it
struct TeacherIn {
    const float* zt;        // teacher logits, laid out as z (top1, wgroup; NULL for ent)
    float invT;             // the term's own inverse temperature
    float th;               // plbl_th
    int within;             // within_filtering
    unsigned* tmax;         // wgroup: the teacher's table [N,S,C] of probability bits (written by the forward, read by the backward)
};

__device__ __forceinline__ mas_u64 pack_max(float p, unsigned pix) {
    return ((mas_u64)mas_f2u(p) << 32) | (mas_u64)(0xffffffffu - pix);
}

__device__ __forceinline__ int table_slot(int* keys, int id) {
    unsigned h = ((unsigned)id * 2654435769u) >> (32 - kLogSlots);
    for (int probe = 0; probe < kSlots; ++probe) {
        int k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == id) return (int)h;
        if (k == -1) {
            int old = atomicCAS(&keys[h], -1, id);
            if (old == -1 || old == id) return (int)h;
        }
        h = (h + 1) & (kSlots - 1);
    }
    return -1;
}

__global__ __launch_bounds__(kThreads) void k_target_bits(const unsigned char* __restrict__ tgt, long long n_rows,
                                                           int cols_stored, int cols_used, unsigned* __restrict__ bits) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_rows) return;
    const unsigned char* t = tgt + r * cols_stored;
    unsigned b = 0;
    for (int c = 0; c < cols_used; ++c) b |= (t[c] ? 1u : 0u) << c;
    bits[r] = b;
}


// ---- logits of one pixel -------------------------------------------------------------------------------------------
// LOWRES: the kernels read the model's quarter-resolution logits zq [C,h,w] and evaluate the final
// F.interpolate(bilinear, align_corners=False) of models/segmentation/utils.py:25 for the pixel in registers -- the
// arithmetic of csrc/upsample.hip (ATen's area_pixel_compute_source_index), so the values equal those of the materialised
// full-resolution tensor bit for bit; that tensor (189 MB per training batch) is then never written or read.
struct LTap { int i0, i1; float l0, l1; };

__device__ __forceinline__ LTap loss_tap(float scale, int o, int n_in) {
    float s = scale * ((float)o + 0.5f) - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    LTap t;
    t.i0 = (int)s;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

struct LowRes { int h, w; float sh, sw; };

template <int CT, bool EXACT, bool LOWRES>
__device__ __forceinline__ void load_logits(const float* __restrict__ zb, int C, int HW, size_t pix, int y, int x, const LowRes& lr,
                                            float (&v)[CT], LTap& ty, LTap& tx) {
    if (LOWRES) {
        ty = loss_tap(lr.sh, y, lr.h);
        tx = loss_tap(lr.sw, x, lr.w);
        const int hw = lr.h * lr.w;
        const int o00 = ty.i0 * lr.w + tx.i0, o01 = ty.i0 * lr.w + tx.i1, o10 = ty.i1 * lr.w + tx.i0, o11 = ty.i1 * lr.w + tx.i1;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (EXACT || c < C) {
                const float* q = zb + (size_t)c * hw;
                v[c] = ty.l0 * (tx.l0 * q[o00] + tx.l1 * q[o01]) + ty.l1 * (tx.l0 * q[o10] + tx.l1 * q[o11]);
            } else {
                v[c] = 0.f;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < CT; ++c) v[c] = (EXACT || c < C) ? zb[(size_t)c * HW + pix] : 0.f;
    }
}

// signed fixed point (44 fractional bits) of one gradient contribution, round to nearest even; mirrored by oracle/exact.c
#define MAS_GRAD_FRAC 44
__device__ __forceinline__ long long grad_fix(float t) {
    union { double d; mas_u64 u; } s;
    s.u = (mas_u64)(1023 + MAS_GRAD_FRAC) << 52;
    return __double2ll_rn((double)t * s.d);
}

// Selected pixels are sparse (a few % of a crop, whole superpixels at a time).  Both scans therefore run in two phases
// per 16x256 tile: (1) every lane looks at the mask bytes of its pixels and the selected ones are COMPACTED into an LDS
// queue (wave ballot + one LDS counter add per wave); (2) the queue is processed densely, one selected pixel per lane, so
// the softmax / log arithmetic runs with all 64 lanes busy instead of whole waves executing it for a handful of lanes.
// Only the logits of selected pixels are ever loaded.  Sums are integers and the group table is a max, so the
// (non-deterministic) queue order cannot change any result.
constexpr int kTilePx = kTileW * kTileH;

__device__ __forceinline__ void queue_push(bool sel, unsigned short off, unsigned short* queue, int* qcount) {
    const unsigned long long bal = __ballot(sel);
    if (bal == 0) return;
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    int base = 0;
    if (lane == 0) base = atomicAdd(qcount, (int)__popcll(bal));
    base = __shfl(base, 0, MAS_WAVE);
    if (sel) queue[base + (int)__popcll(bal & ((1ull << lane) - 1ull))] = off;
}

// phase 1 of both scans: compact the selected pixels of this tile; BWD additionally zero-fills dz for the whole tile
template <int CT, bool EXACT, bool VEC, bool BWD>
__device__ __forceinline__ void tile_compact(const unsigned char* __restrict__ mb, int C, int H, int W, int HW, int tx, int ty,
                                             unsigned short* queue, int* qcount, float* __restrict__ db) {
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    const int wave = threadIdx.x / MAS_WAVE;
    for (int it = 0; it < kTileH / 4; ++it) {
        const int ry = it * 4 + wave;
        const int y = ty * kTileH + ry;
        if (y >= H) break;
        const size_t row = (size_t)y * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int rx = VEC ? (lane * 4 + k) : (k * MAS_WAVE + lane);
            const int x = tx * kTileW + rx;
            const bool sel = (x < W) && (mb[row + (x < W ? x : 0)] != 0);
            queue_push(sel, (unsigned short)((ry << 8) | rx), queue, qcount);
        }
        if (BWD) {
            if (VEC) {
                const int x = tx * kTileW + lane * 4;
                if (x < W) {
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        if (EXACT || c < C) *reinterpret_cast<float4*>(db + (size_t)c * HW + row + x) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = tx * kTileW + k * MAS_WAVE + lane;
                    if (x < W) {
#pragma unroll
                        for (int c = 0; c < CT; ++c)
                            if (EXACT || c < C) db[(size_t)c * HW + row + x] = 0.0f;
                    }
                }
            }
        }
    }
}

// The fourth loss slot of a selected multi-hot pixel (teacher_terms.h).  `v` holds the student's logits.  top1: the teacher's row is
// loaded into `u` (same taps / same address as the student's), reduced to the gate, and only then overwritten with the student's
// softmax at the term's temperature -- the teacher row is never live beside a third array.  ent: `u` = the softmax restricted to
// M = the candidates with a non-zero logit.  Returns whether the pixel counts.
template <int CT, bool EXACT, bool LOWRES, int TT>
__device__ __forceinline__ bool teacher_term_probs(const float* __restrict__ ztb, const float (&v)[CT], int C, int HW, size_t pix, int py,
                                                   int px, const LowRes& lr, unsigned Y, const TeacherIn& te, float (&u)[CT], unsigned& M) {
    const int Cn = EXACT ? CT : C;
    if (TT == MAS_TT_TOP1) {
        LTap t_y, t_x;
        load_logits<CT, EXACT, LOWRES>(ztb, C, HW, pix, py, px, lr, u, t_y, t_x);
        M = mas_tt_all(Cn);
        mas_tt_softmax(u, CT, Cn, M, te.invT);
        if (!mas_tt_gate(u, CT, Cn, Y, te.within, te.th)) return false;
    } else {
        M = mas_tt_ent_set(v, CT, Cn, Y);
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) u[c] = v[c];
    mas_tt_softmax(u, CT, Cn, M, te.invT);
    return true;
}

// TT (MAS_TT_*): the fourth loss slot (teacher_terms.h).  MAS_TT_NONE instantiations are the scans as they were: `te` is a trailing
// kernel argument they never read, and nothing of the slot is compiled into them.
template <int CT, bool EXACT, typename IdT, bool VEC, bool LOWRES, bool PLX, int TT>
__global__ __launch_bounds__(kThreads) void k_partial_loss_fwd(const float* __restrict__ z, const IdT* __restrict__ spx,
                                                                const unsigned char* __restrict__ mask,
                                                                const unsigned* __restrict__ bits, int C, int H, int W, int S,
                                                                float invT, int flags, int tiles_x, int tiles_y,
                                                                mas_u64* __restrict__ gmax, mas_u64* __restrict__ acc, const LowRes lr,
                                                                const TeacherIn te) {
    constexpr bool XS = TT == MAS_TT_TOP1 || TT == MAS_TT_ENT;     // a fourth loss slot
    constexpr bool WG = TT == MAS_TT_WGROUP;                        // the teacher's table beside the student's
    constexpr int NR = XS ? 7 : 5;              // scalar accumulators of a workgroup
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    mas_u64* t_max = reinterpret_cast<mas_u64*>(smem);                       // [kSlots * C]
    int* t_keys = reinterpret_cast<int*>(smem + sizeof(mas_u64) * kSlots * C);  // [kSlots]
    mas_u64* s_red = reinterpret_cast<mas_u64*>(smem + sizeof(mas_u64) * kSlots * C + sizeof(int) * kSlots);  // [4][NR]
    int* qcount = reinterpret_cast<int*>(s_red + 4 * NR);
    unsigned short* queue = reinterpret_cast<unsigned short*>(qcount + 2);     // [kTilePx]
    unsigned* t_tmax = reinterpret_cast<unsigned*>(queue + kTilePx);           // [kSlots * C] (WG only: fwd_smem_bytes)

    const bool do_ce = flags & MAS_LOSS_CE;
    const bool do_group = flags & MAS_LOSS_GROUP;
    const bool only_multi = flags & MAS_LOSS_GROUP_ONLY_MULTI;
    const bool tce = flags & MAS_LOSS_TCE;          // `spx` holds class labels, the target of a pixel is its label, no epsilon
    const int pl_mode = PLX ? mas_pl_mode(flags) : MAS_PL_CHOICE;      // (PLX: rc or topone, never combined with tce)
    if (threadIdx.x == 0) *qcount = 0;
    if (do_group) {
        for (int i = threadIdx.x; i < kSlots; i += kThreads) t_keys[i] = -1;
        for (int i = threadIdx.x; i < kSlots * C; i += kThreads) t_max[i] = 0;
        if (WG)
            for (int i = threadIdx.x; i < kSlots * C; i += kThreads) t_tmax[i] = 0;
    }
    __syncthreads();

    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int n = bid / tiles_y;
    const int HW = H * W;
    const float* zb = z + (size_t)n * C * (LOWRES ? lr.h * lr.w : HW);
    const float* ztb = (TT == MAS_TT_TOP1 || WG) ? te.zt + (size_t)n * C * (LOWRES ? lr.h * lr.w : HW) : nullptr;
    const IdT* sb = spx + (size_t)n * HW;
    const unsigned char* mb = mask + (size_t)n * HW;
    const unsigned* bb = bits + (size_t)n * S;
    mas_u64* gm = gmax + (size_t)n * S * C;
    unsigned* tm = WG ? te.tmax + (size_t)n * S * C : nullptr;
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    const int wave = threadIdx.x / MAS_WAVE;

    tile_compact<CT, EXACT, VEC, false>(mb, C, H, W, HW, tx, ty, queue, qcount, nullptr);
    __syncthreads();
    const int nq = *qcount;

    mas_u64 sum_ce = 0, sum_mc = 0, sum_x = 0;
    unsigned n_ce = 0, n_mc = 0, n_empty = 0, n_x = 0;
    for (int i = threadIdx.x; i < nq; i += kThreads) {
        const unsigned off = queue[i];
        const int py = ty * kTileH + (int)(off >> 8), px = tx * kTileW + (int)(off & 255u);
        const size_t pix = (size_t)py * W + px;
        const int id = mas_load_id(sb, pix);
        if (id < 0 || id >= S) continue;
        float v[CT];
        LTap t_y, t_x;
        load_logits<CT, EXACT, LOWRES>(zb, C, HW, pix, py, px, lr, v, t_y, t_x);
        const unsigned Y = tce ? (1u << id) : bb[id];
        const int nb = __popc(Y);
        if (nb == 0) { n_empty += 1; continue; }
        if (XS && nb > 1) {
            float u[CT];
            unsigned M;
            if (teacher_term_probs<CT, EXACT, LOWRES, TT>(ztb, v, C, HW, pix, py, px, lr, Y, te, u, M)) {
                const int Cn = EXACT ? CT : C;
                const float l = (TT == MAS_TT_TOP1) ? mas_pl_loss(u, CT, Cn, Y, MAS_PL_TOPONE) : mas_tt_ent_loss(u, CT, Cn, M);
                sum_x += mas_fix(l, MAS_LOSS_FRAC);
                n_x += 1;
            }
        }
        {
            const float rinv = mas_softmax_regs<CT, EXACT>(v, C, invT);
#pragma unroll
            for (int c = 0; c < CT; ++c) v[c] = v[c] * rinv;
        }
        if (PLX && do_ce && nb > 1) {
            sum_mc += mas_fix(mas_pl_loss(v, CT, EXACT ? CT : C, Y, pl_mode), MAS_LOSS_FRAC);
            n_mc += 1;
        } else if (do_ce) {
            float pos = 0.0f;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (EXACT || c < C) pos = ((Y >> c) & 1u) ? (pos + v[c]) : pos;
            // (temperature CE: no epsilon; a target probability below the smallest normal float -- a logit gap beyond 86 / T, outside the
            //  cosine head's range -- is held there, so neither the logarithm nor the backward's 1 / pos leaves the finite floats)
            const float l = -mas_logf(tce ? (pos < 1.17549435e-38f ? 1.17549435e-38f : pos) : pos + 1e-8f);
            const mas_u64 q = mas_fix(l, MAS_LOSS_FRAC);
            if (nb == 1) { sum_ce += q; n_ce += 1; } else { sum_mc += q; n_mc += 1; }
        }
        if (do_group && (!only_multi || nb > 1)) {
            const int s = table_slot(t_keys, id);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if ((EXACT || c < C) && ((Y >> c) & 1u)) {
                    const mas_u64 w = pack_max(v[c], (unsigned)pix);
                    if (s >= 0) atomicMax(&t_max[s * C + c], w);
                    else atomicMax(&gm[(size_t)id * C + c], w);
                }
            }
            if (WG) {
                // the teacher's row of the same pixel (same taps / same address) replaces the student's probabilities, which are done
                load_logits<CT, EXACT, LOWRES>(ztb, C, HW, pix, py, px, lr, v, t_y, t_x);
                const float rinv = mas_softmax_regs<CT, EXACT>(v, C, invT);
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    if ((EXACT || c < C) && ((Y >> c) & 1u)) {
                        const unsigned w = mas_f2u(v[c] * rinv);
                        if (s >= 0) atomicMax(&t_tmax[s * C + c], w);
                        else atomicMax(&tm[(size_t)id * C + c], w);
                    }
                }
            }
        }
    }

    // block reduction of the five (teacher terms: seven) scalar accumulators
    mas_u64 r[7] = {sum_ce, sum_mc, (mas_u64)n_ce, (mas_u64)n_mc, (mas_u64)n_empty, sum_x, (mas_u64)n_x};
#pragma unroll
    for (int i = 0; i < NR; ++i) {
#pragma unroll
        for (int off = MAS_WAVE / 2; off > 0; off >>= 1) r[i] += __shfl_down(r[i], off, MAS_WAVE);
        if (lane == 0) s_red[wave * NR + i] = r[i];
    }
    __syncthreads();
    if (threadIdx.x < NR) {
        mas_u64 a = 0;
        for (int w = 0; w < kThreads / MAS_WAVE; ++w) a += s_red[w * NR + threadIdx.x];
        if (a) atomicAdd(&acc[threadIdx.x < 5 ? threadIdx.x : ACC_SUM_X + (threadIdx.x - 5)], a);
    }
    if (do_group) {
        for (int i = threadIdx.x; i < kSlots * C; i += kThreads) {
            const mas_u64 w = t_max[i];
            if (w) {
                const int s = i / C;
                atomicMax(&gm[(size_t)t_keys[s] * C + (i - s * C)], w);
            }
        }
        if (WG) {
            for (int i = threadIdx.x; i < kSlots * C; i += kThreads) {
                const unsigned w = t_tmax[i];
                if (w) {
                    const int s = i / C;
                    atomicMax(&tm[(size_t)t_keys[s] * C + (i - s * C)], w);
                }
            }
        }
    }
}

// acc[ACC_DONE]: workgroups of k_group_finalize that have added their sums (the fused entry point: the LAST one turns the sums into
// the loss values -- no k_loss_values launch)
constexpr int ACC_DONE = 7;
__host__ __device__ __forceinline__ void loss_values_of(const mas_u64* acc, int flags, const float* w, float* out);

// WG: the weighted form (teacher_terms.h, wgroup) -- every counted entry's -log is multiplied by the teacher's maximum tmax[i]
template <bool WG>
__global__ __launch_bounds__(kThreads) void k_group_finalize(const mas_u64* __restrict__ gmax, const unsigned* __restrict__ tmax,
                                                              long long n_entries, mas_u64* __restrict__ acc, int flags,
                                                              const float* __restrict__ w, float* __restrict__ values) {
    __shared__ mas_u64 s_red[kThreads / MAS_WAVE][2];
    __shared__ int s_last;
    mas_u64 sum = 0, cnt = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_entries; i += (long long)gridDim.x * kThreads) {
        const mas_u64 w64 = gmax[i];
        const unsigned pb = (unsigned)(w64 >> 32);
        if (pb) {            // a (superpixel, class) with target bit set whose max prob is non-zero
            const float l = WG ? mas_tt_wg_loss(mas_u2f(tmax[i]), mas_u2f(pb)) : -mas_logf(mas_u2f(pb) + 1e-8f);
            sum += mas_fix(l, MAS_LOSS_FRAC);
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
        mas_u64 a = 0;
        for (int wv = 0; wv < kThreads / MAS_WAVE; ++wv) a += s_red[wv][threadIdx.x];
        if (a) atomicAdd(&acc[threadIdx.x == 0 ? ACC_SUM_GROUP : ACC_N_GROUP], a);
    }
    if (!values) return;
    // the last workgroup to arrive sees every other workgroup's sums: device-scope release (fence + counter add) / acquire
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const mas_u64 done = atomicAdd(&acc[ACC_DONE], (mas_u64)1);
        s_last = done == (mas_u64)(gridDim.x - 1);
    }
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        __threadfence();
        mas_u64 a[8];
        for (int i = 0; i < 7; ++i) a[i] = __hip_atomic_load(&acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        loss_values_of(a, flags, w, values);
    }
}

// the fused forward's first launch: zero the accumulators and the (superpixel, class) table, and (targets != NULL) turn the
// multi-hot target rows into bit masks -- one launch instead of a memset and k_target_bits
__global__ __launch_bounds__(kThreads) void k_loss_prep(mas_u64* __restrict__ zero64, long long n_zero, const unsigned char* __restrict__ tgt,
                                                         long long n_rows, int cols_stored, int cols_used, unsigned* __restrict__ bits) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_zero) zero64[i] = 0;
    if (tgt && i < n_rows) {
        const unsigned char* t = tgt + i * cols_stored;
        unsigned b = 0;
        for (int c = 0; c < cols_used; ++c) b |= (t[c] ? 1u : 0u) << c;
        bits[i] = b;
    }
}

// loss = (sum * 2^-32) / (1 + n) in f64, rounded once to f32; MAS_LOSS_TCE: the plain mean, / n (0 / 0 = NaN as torch's
// CrossEntropyLoss over no valid pixel)
__host__ __device__ __forceinline__ float loss_value(mas_u64 sum, mas_u64 n, int one = 1) {
    union { double d; mas_u64 u; } s;
    s.u = (mas_u64)(1023 - MAS_LOSS_FRAC) << 52;
    return (float)(((double)sum * s.d) / (double)(n + one));
}

// losses[0..2] = (ce, mc, group); with weights also losses[3] = (w_ce * ce + w_mc * mc) + w_group * group, every product and sum
// rounded once in f32 -- the operation order of `coeff * ce_loss + coeff_mc * mc_loss + coeff_gm * group_loss`
// (trainer/active_joint_multi_predignore_lossdecomp.py:104), so the value equals the torch expression bit for bit.
__host__ __device__ __forceinline__ void loss_values_of(const mas_u64* acc, int flags, const float* w, float* out) {
    if (flags & MAS_LOSS_TCE) {
        out[0] = loss_value(acc[ACC_SUM_CE], acc[ACC_N_CE], 0);
        out[1] = 0.0f;
        out[2] = 0.0f;
        if (w) out[3] = (w[0] * out[0] + w[1] * 0.0f) + w[2] * 0.0f;
        return;
    }
    float ce, mc;
    if (flags & MAS_LOSS_DECOMP) {
        ce = loss_value(acc[ACC_SUM_CE], acc[ACC_N_CE]);
        mc = loss_value(acc[ACC_SUM_MC], acc[ACC_N_MC]);
    } else {
        ce = loss_value(acc[ACC_SUM_CE] + acc[ACC_SUM_MC], acc[ACC_N_CE] + acc[ACC_N_MC]);
        mc = 0.0f;
    }
    const float gr = loss_value(acc[ACC_SUM_GROUP], acc[ACC_N_GROUP]);
    out[0] = ce;
    out[1] = mc;
    out[2] = gr;
    if (w) out[3] = (w[0] * ce + w[1] * mc) + w[2] * gr;
}

// (w == NULL: the three losses alone)
__global__ void k_loss_values_weighted(const mas_u64* __restrict__ acc, int flags, const float* __restrict__ w, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    loss_values_of(acc, flags, w, out);
}

// scale_k = upstream_k / (1 + n_k) (f32 division, correctly rounded); with weights: grad[0] is dL/dtotal and
// scale_k = (dL/dtotal * w_k) / (1 + n_k) -- the chain rule through the weighted sum, in the order autograd applies it
__host__ __device__ __forceinline__ void loss_scales_of(const mas_u64* acc, const float* grad, const float* w, int flags, float* scale) {
    if (flags & MAS_LOSS_TCE) {
        scale[0] = (w ? grad[0] * w[0] : grad[0]) / (float)acc[ACC_N_CE];
        scale[1] = 0.0f;
        scale[2] = 0.0f;
        return;
    }
    const float g0 = w ? grad[0] * w[0] : grad[0], g1 = w ? grad[0] * w[1] : grad[1], g2 = w ? grad[0] * w[2] : grad[2];
    if (flags & MAS_LOSS_DECOMP) {
        scale[0] = g0 / (float)(acc[ACC_N_CE] + 1);
        scale[1] = g1 / (float)(acc[ACC_N_MC] + 1);
    } else {
        const float sc = g0 / (float)(acc[ACC_N_CE] + acc[ACC_N_MC] + 1);
        scale[0] = sc;
        scale[1] = sc;
    }
    scale[2] = g2 / (float)(acc[ACC_N_GROUP] + 1);
}

// (w == NULL: `grad_total` holds the three upstream gradients)
__global__ void k_loss_scales_weighted(const mas_u64* __restrict__ acc, const float* __restrict__ grad_total, const float* __restrict__ w,
                                       int flags, float* __restrict__ scale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    loss_scales_of(acc, grad_total, w, flags, scale);
}

// LOWRES: `dz` is the caller-zeroed int64 fixed-point accumulator dzq_fix [N,C,h,w] (MAS_GRAD_FRAC fractional bits): every
// selected pixel adds (gradient of its class-c logit) * (bilinear weight) into the four quarter-resolution elements its
// logits were interpolated from -- integer atomics, so the sums do not depend on the order; nothing is written at full
// resolution.
// TT != MAS_TT_NONE: scale[3] is the factor of the fourth loss slot; the gradient of its term is added to the pixel's d in f32 before
// the one store (full resolution) or the four fixed-point adds (LOWRES), so there is still one write per logit.
template <int CT, bool EXACT, typename IdT, bool VEC, bool LOWRES, bool PLX, int TT>
__global__ __launch_bounds__(kThreads) void k_partial_loss_bwd(const float* __restrict__ z, const IdT* __restrict__ spx,
                                                                const unsigned char* __restrict__ mask,
                                                                const unsigned* __restrict__ bits,
                                                                const mas_u64* __restrict__ gmax,
                                                                const float* __restrict__ scale, int C, int H, int W, int S,
                                                                float invT, int flags, int tiles_x, int tiles_y,
                                                                float* __restrict__ dz, const LowRes lr, const mas_u64* __restrict__ acc,
                                                                const float* __restrict__ grad, const float* __restrict__ gw,
                                                                const TeacherIn te) {
    __shared__ int qcount[2];
    __shared__ unsigned short queue[kTilePx];
    // LOWRES: the quarter-resolution footprint of a 4 x 256 tile (<= 4 rows x 72 columns per class for the x4 ratios of the
    // model) is accumulated in LDS first; only its non-zero entries go to memory (16-60x fewer global atomics)
    constexpr bool LACC = LOWRES && EXACT;
    constexpr int kLR = 4, kLC = 72;
    __shared__ mas_u64 s_acc[LACC ? CT * kLR * kLC : 1];
    const bool do_ce = flags & MAS_LOSS_CE;
    const bool do_group = flags & MAS_LOSS_GROUP;
    const bool only_multi = flags & MAS_LOSS_GROUP_ONLY_MULTI;
    const int pl_mode = PLX ? mas_pl_mode(flags) : MAS_PL_CHOICE;
    if (threadIdx.x == 0) qcount[0] = 0;
    __syncthreads();
    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int n = bid / tiles_y;
    const int HW = H * W;
    const int hw_in = LOWRES ? lr.h * lr.w : HW;
    const float* zb = z + (size_t)n * C * hw_in;
    constexpr bool XS = TT == MAS_TT_TOP1 || TT == MAS_TT_ENT;     // a fourth loss slot
    constexpr bool WG = TT == MAS_TT_WGROUP;                        // arg-pixel entries weighted by the teacher's table
    const float* ztb = (TT == MAS_TT_TOP1) ? te.zt + (size_t)n * C * hw_in : nullptr;
    const unsigned* tm = WG ? te.tmax + (size_t)n * S * C : nullptr;
    float* db = LOWRES ? nullptr : dz + (size_t)n * C * HW;
    mas_u64* qb = LOWRES ? reinterpret_cast<mas_u64*>(dz) + (size_t)n * C * hw_in : nullptr;
    const IdT* sb = spx + (size_t)n * HW;
    const unsigned char* mb = mask + (size_t)n * HW;
    const unsigned* bb = bits + (size_t)n * S;
    const mas_u64* gm = gmax + (size_t)n * S * C;
    // scale == NULL (the fused entry points): every workgroup forms the three scale factors itself from the accumulators of the
    // forward scan and the upstream gradient (three divisions on uniform values) -- the k_loss_scales launch is gone
    float sc3[3];
    if (scale) { sc3[0] = scale[0]; sc3[1] = scale[1]; sc3[2] = scale[2]; }
    else loss_scales_of(acc, grad, gw, flags, sc3);
    const float a_ce = sc3[0] * invT, a_mc = sc3[1] * invT, g6 = sc3[2] * invT;
    const float a_x = XS ? scale[3] * te.invT : 0.0f;

    // phase 1: dz = 0 over the whole tile (streaming 16-B stores) while the selected pixels are compacted
    tile_compact<CT, EXACT, VEC, !LOWRES>(mb, C, H, W, HW, tx, ty, queue, qcount, db);
    __syncthreads();        // (waits for this workgroup's zero stores: the gradients below overwrite some of them)
    const int nq = qcount[0];
    int ry0 = 0, rx0 = 0;
    if (LACC) {
        if (nq == 0) return;                              // (uniform) nothing selected in this tile
        ry0 = loss_tap(lr.sh, ty * kTileH, lr.h).i0;
        rx0 = loss_tap(lr.sw, tx * kTileW, lr.w).i0;
        for (int i = threadIdx.x; i < CT * kLR * kLC; i += kThreads) s_acc[i] = 0;
        __syncthreads();
    }
    auto add_q = [&](mas_u64* q, int c, int iy, int ix, long long val) {
        const int r = iy - ry0, x = ix - rx0;
        if (LACC && r < kLR && x < kLC) atomicAdd(&s_acc[(c * kLR + r) * kLC + x], (mas_u64)val);
        else atomicAdd(q + (iy * lr.w + ix), (mas_u64)val);
    };

    // phase 2: gradients of the selected pixels, one pixel per lane
    for (int i = threadIdx.x; i < nq; i += kThreads) {
        const unsigned off = queue[i];
        const int py = ty * kTileH + (int)(off >> 8), px = tx * kTileW + (int)(off & 255u);
        const size_t pix = (size_t)py * W + px;
        const int id = mas_load_id(sb, pix);
        if (id < 0 || id >= S) continue;
        const unsigned Y = (flags & MAS_LOSS_TCE) ? (1u << id) : bb[id];
        const int nb = __popc(Y);
        if (nb == 0) continue;
        float v[CT];
        LTap t_y, t_x;
        load_logits<CT, EXACT, LOWRES>(zb, C, HW, pix, py, px, lr, v, t_y, t_x);
        // the fourth slot: u = the term's own probabilities of this pixel, (gx, ux) the per-pixel constants of its gradient
        float u[XS ? CT : 1];
        unsigned M = 0;
        bool xon = false;
        mas_pl_grad_ctx gx = {};
        float ux = 0.0f;
        if constexpr (XS) {
            if (nb > 1) xon = teacher_term_probs<CT, EXACT, LOWRES, TT>(ztb, v, C, HW, pix, py, px, lr, Y, te, u, M);
            if (xon) {
                if (TT == MAS_TT_TOP1) gx = mas_pl_grad_prepare(u, CT, EXACT ? CT : C, Y, MAS_PL_TOPONE, a_x);
                else ux = mas_tt_ent_u(u, CT, EXACT ? CT : C, M);
            }
        }
        {
            const float rinv = mas_softmax_regs<CT, EXACT>(v, C, invT);
#pragma unroll
            for (int c = 0; c < CT; ++c) v[c] = v[c] * rinv;
        }
        float coef = 0.0f, pos = 0.0f;
        // PLX: the multi-hot pixel's CE coefficients come from partial_label.h (rc / topone); one-hot pixels keep the arithmetic below
        const bool plx = PLX && do_ce && nb > 1;
        mas_pl_grad_ctx gk = {};
        if (plx) {
            gk = mas_pl_grad_prepare(v, CT, EXACT ? CT : C, Y, pl_mode, a_mc);
        } else if (do_ce) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (EXACT || c < C) pos = ((Y >> c) & 1u) ? (pos + v[c]) : pos;
            coef = ((nb == 1) ? a_ce : a_mc) * (1.0f / ((flags & MAS_LOSS_TCE) ? (pos < 1.17549435e-38f ? 1.17549435e-38f : pos) : pos + 1e-8f));
        }
        // group loss: classes of Y whose arg-max pixel is this pixel
        unsigned A = 0;
        float ug = 0.0f;
        float t[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) t[c] = 0.0f;
        if (do_group && (!only_multi || nb > 1)) {
            const unsigned key = 0xffffffffu - (unsigned)pix;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if ((EXACT || c < C) && ((Y >> c) & 1u)) {
                    const mas_u64 w = gm[(size_t)id * C + c];
                    if ((unsigned)w == key && (unsigned)(w >> 32) != 0u) {
                        A |= 1u << c;
                        t[c] = WG ? mas_tt_wg_coef(g6, mas_u2f(tm[(size_t)id * C + c]), v[c]) : -(g6 / (v[c] + 1e-8f));
                        ug = ug + t[c] * v[c];
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (EXACT || c < C) {
                const float p = v[c];
                const float yj = ((Y >> c) & 1u) ? 1.0f : 0.0f;
                float d = coef * (p * (pos - yj));
                if (plx) d = mas_pl_grad(gk, pl_mode, p, (int)((Y >> c) & 1u), c);
                if (A) {
                    if ((A >> c) & 1u) d = d + t[c] * p;
                    d = d - p * ug;
                }
                if constexpr (XS) {
                    if (xon) d = d + ((TT == MAS_TT_TOP1) ? mas_pl_grad(gx, MAS_PL_TOPONE, u[c], (int)((Y >> c) & 1u), c)
                                                          : mas_tt_ent_grad(a_x, ux, u[c], (int)((M >> c) & 1u)));
                }
                if (LOWRES) {
                    mas_u64* q = qb + (size_t)c * hw_in;
                    add_q(q, c, t_y.i0, t_x.i0, grad_fix(d * (t_y.l0 * t_x.l0)));
                    add_q(q, c, t_y.i0, t_x.i1, grad_fix(d * (t_y.l0 * t_x.l1)));
                    add_q(q, c, t_y.i1, t_x.i0, grad_fix(d * (t_y.l1 * t_x.l0)));
                    add_q(q, c, t_y.i1, t_x.i1, grad_fix(d * (t_y.l1 * t_x.l1)));
                } else {
                    db[(size_t)c * HW + pix] = d;
                }
            }
        }
    }
    if (LACC) {
        __syncthreads();
        for (int i = threadIdx.x; i < CT * kLR * kLC; i += kThreads) {
            const mas_u64 val = s_acc[i];
            if (val) {
                const int c = i / (kLR * kLC), rem = i - c * (kLR * kLC);
                const int r = rem / kLC, x = rem - r * kLC;
                atomicAdd(qb + (size_t)c * hw_in + (size_t)(ry0 + r) * lr.w + (rx0 + x), val);
            }
        }
    }
}

// tt: the MAS_TT_* value of the instantiation -- a fourth slot reduces seven scalars, wgroup appends the teacher's u32 table
inline size_t fwd_smem_bytes(int C, int tt = MAS_TT_NONE) {
    const bool xs = tt == MAS_TT_TOP1 || tt == MAS_TT_ENT;
    return sizeof(mas_u64) * kSlots * (size_t)C + sizeof(int) * kSlots + sizeof(mas_u64) * 4 * (xs ? 7 : 5) + sizeof(int) * 2 +
           sizeof(unsigned short) * kTilePx + (tt == MAS_TT_WGROUP ? sizeof(unsigned) * kSlots * (size_t)C : 0);
}

// which entry points a call came through: it decides the flag rule (the *_flags_ok predicates below)
enum LossFamily {
    FAMILY_PLAIN,               // mas_partial_loss_*: `acc` has 8 words, `te` is unused
    FAMILY_TEACHER,             // mas_teacher_loss_*: `acc` has 16 words, `te` holds the fourth slot's inputs, `scale` four factors
    FAMILY_WGROUP               // mas_wgroup_loss_*: `acc` has 8 words, `te.zt` and `te.tmax` are filled in
};

struct LossArgs {
    LossFamily family;
    const float* z; const void* spx; const unsigned char* mask; const unsigned* bits;
    int N, C, H, W, S; float invT; int flags;
    int h, w;                   // > 0: `z` is the quarter-resolution tensor [N,C,h,w] (LOWRES kernels)
    mas_u64* gmax; mas_u64* acc; const float* scale; float* dz;
    const float* grad = nullptr; const float* gw = nullptr;     // backward with scale == NULL: upstream gradient(s) and optional weights
    TeacherIn te = {nullptr, 0.f, 0.f, 0, nullptr};
};

// The one place a scan's arguments are put together: the head every entry point shares, the quarter-resolution extents (h <= 0: full
// resolution), then what the direction reads and writes -- forward: the table and the accumulators; backward: the table, the scale
// factors (NULL in the fused backward, which passes `acc` and fills in grad / gw), dz, and the fixed-point sums that take dz's place
// at quarter resolution.  The tables and sums are the caller's uint64_t / int64_t; the kernels' own types have the same layout.
inline LossArgs loss_args(LossFamily family, const float* z, int h, int w, const void* spx, const uint8_t* mask, const uint32_t* bits, int N,
                          int C, int H, int W, int S, float invT, int flags, const void* gmax, const void* acc,
                          const float* scale = nullptr, float* dz = nullptr, int64_t* dzq_fix = nullptr) {
    const bool low = h > 0;
    return LossArgs{family, z, spx, mask, bits, N, C, H, W, S, invT, flags, low ? h : 0, low ? w : 0,
                    const_cast<mas_u64*>(static_cast<const mas_u64*>(gmax)), const_cast<mas_u64*>(static_cast<const mas_u64*>(acc)), scale,
                    low ? reinterpret_cast<float*>(dzq_fix) : dz};
}

template <int CT, bool EXACT, typename IdT, bool PLX, int TT = MAS_TT_NONE>
int launch_loss(const LossArgs& a, bool backward, hipStream_t st) {
    const int tiles_x = (a.W + kTileW - 1) / kTileW;
    const int tiles_y = (a.H + kTileH - 1) / kTileH;
    const long long nblk = (long long)a.N * tiles_x * tiles_y;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return MAS_ERR_SHAPE;
    const IdT* ids = static_cast<const IdT*>(a.spx);
    const bool low = a.h > 0;
    const bool vec = (a.W % 4 == 0) && (low || ((((uintptr_t)a.z & 15) == 0) && (!backward || (((uintptr_t)a.dz & 15) == 0))));
    const dim3 grid((unsigned)nblk), block(kThreads);
    const LowRes lr{a.h, a.w, low ? (float)a.h / (float)a.H : 0.f, low ? (float)a.w / (float)a.W : 0.f};
#define MAS_LAUNCH_LOSS(VECV, LOWV)                                                                                                     \
    do {                                                                                                                                \
        if (!backward)                                                                                                                  \
            hipLaunchKernelGGL((k_partial_loss_fwd<CT, EXACT, IdT, VECV, LOWV, PLX, TT>), grid, block, fwd_smem_bytes(a.C, TT), st, a.z, ids, \
                               a.mask, a.bits, a.C, a.H, a.W, a.S, a.invT, a.flags, tiles_x, tiles_y, a.gmax, a.acc, lr, a.te);           \
        else                                                                                                                            \
            hipLaunchKernelGGL((k_partial_loss_bwd<CT, EXACT, IdT, VECV, LOWV, PLX, TT>), grid, block, 0, st, a.z, ids, a.mask, a.bits, a.gmax, \
                               a.scale, a.C, a.H, a.W, a.S, a.invT, a.flags, tiles_x, tiles_y, a.dz, lr, a.acc, a.grad, a.gw, a.te);     \
    } while (0)
    if (low) { if (vec) MAS_LAUNCH_LOSS(true, true); else MAS_LAUNCH_LOSS(false, true); }
    else { if (vec) MAS_LAUNCH_LOSS(true, false); else MAS_LAUNCH_LOSS(false, false); }
#undef MAS_LAUNCH_LOSS
    return mas_launch_status();
}

template <int CT, bool EXACT>
int dispatch_loss_ids(const LossArgs& a, int spx_dtype, bool backward, hipStream_t st) {
    if (const int tt = mas_tt_mode(a.flags)) {
#define MAS_TEACHER_BY_TERM(IDT) (tt == MAS_TT_TOP1 ? launch_loss<CT, EXACT, IDT, false, MAS_TT_TOP1>(a, backward, st) \
                                  : (tt == MAS_TT_ENT ? launch_loss<CT, EXACT, IDT, false, MAS_TT_ENT>(a, backward, st)     \
                                                      : launch_loss<CT, EXACT, IDT, false, MAS_TT_WGROUP>(a, backward, st)))
        switch (spx_dtype) {
            case MAS_ID_I64: return MAS_TEACHER_BY_TERM(long long);
            case MAS_ID_I32: return MAS_TEACHER_BY_TERM(int);
            case MAS_ID_U16: return MAS_TEACHER_BY_TERM(unsigned short);
            default: return MAS_ERR_DTYPE;
        }
#undef MAS_TEACHER_BY_TERM
    }
    // the rc / topone multi-hot term is compiled into instantiations of its own (PLX): the merged-positive kernels stay as they were
    const bool plx = (a.flags & (MAS_LOSS_RC | MAS_LOSS_TOPONE)) != 0;
#define MAS_LOSS_BY_MODE(IDT) (plx ? launch_loss<CT, EXACT, IDT, true>(a, backward, st) : launch_loss<CT, EXACT, IDT, false>(a, backward, st))
    switch (spx_dtype) {
        case MAS_ID_I64: return MAS_LOSS_BY_MODE(long long);
        case MAS_ID_I32: return MAS_LOSS_BY_MODE(int);
        case MAS_ID_U16: return MAS_LOSS_BY_MODE(unsigned short);
        default: return MAS_ERR_DTYPE;
    }
#undef MAS_LOSS_BY_MODE
}

// MAS_LOSS_RC / MAS_LOSS_TOPONE name the multi-hot term of the CE sums: one of them at most, with MAS_LOSS_CE, never with MAS_LOSS_TCE
inline bool loss_flags_ok(int flags) {
    if (flags & (MAS_LOSS_TOP1 | MAS_LOSS_ENT | MAS_LOSS_WITHIN)) return false;     // (the mas_teacher_loss_* entry points only)
    if (flags & MAS_LOSS_WGROUP) return false;                                      // (the mas_wgroup_loss_* entry points only)
    const int m = flags & (MAS_LOSS_RC | MAS_LOSS_TOPONE);
    if (!m) return true;
    return m != (MAS_LOSS_RC | MAS_LOSS_TOPONE) && (flags & MAS_LOSS_CE) && !(flags & MAS_LOSS_TCE);
}

// MAS_LOSS_TOP1 / MAS_LOSS_ENT: one of them, beside the merged-positive (MAS_LOSS_CE, optionally MAS_LOSS_DECOMP) and group flags only;
// MAS_LOSS_WITHIN qualifies MAS_LOSS_TOP1
inline bool teacher_flags_ok(int flags) {
    const int t = flags & (MAS_LOSS_TOP1 | MAS_LOSS_ENT);
    if (!t || t == (MAS_LOSS_TOP1 | MAS_LOSS_ENT)) return false;
    if ((flags & MAS_LOSS_WITHIN) && !(flags & MAS_LOSS_TOP1)) return false;
    return !(flags & ~(MAS_LOSS_CE | MAS_LOSS_DECOMP | MAS_LOSS_GROUP | MAS_LOSS_GROUP_ONLY_MULTI | MAS_LOSS_TOP1 | MAS_LOSS_ENT | MAS_LOSS_WITHIN));
}

// MAS_LOSS_WGROUP: with MAS_LOSS_GROUP, beside MAS_LOSS_CE, MAS_LOSS_DECOMP and MAS_LOSS_GROUP_ONLY_MULTI only
inline bool wgroup_flags_ok(int flags) {
    if (!(flags & MAS_LOSS_WGROUP) || !(flags & MAS_LOSS_GROUP)) return false;
    return !(flags & ~(MAS_LOSS_CE | MAS_LOSS_DECOMP | MAS_LOSS_GROUP | MAS_LOSS_GROUP_ONLY_MULTI | MAS_LOSS_WGROUP));
}

inline bool family_flags_ok(LossFamily family, int flags) {
    return family == FAMILY_WGROUP ? wgroup_flags_ok(flags) : (family == FAMILY_TEACHER ? teacher_flags_ok(flags) : loss_flags_ok(flags));
}

// the extents and the class count of a scan; `plane_limit`: with the scans' bound on H * W.  (The fused entry points ask without it
// before their first launch; dispatch_loss then asks with it.)
inline int loss_dims_status(int N, int C, int H, int W, int S, bool plane_limit) {
    if (N <= 0 || H <= 0 || W <= 0 || S <= 0 || (plane_limit && (long long)H * W > 0x7fffffffLL / 2)) return MAS_ERR_SHAPE;
    if (C < 2 || C > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    return 0;
}

int dispatch_loss(const LossArgs& a, int spx_dtype, bool backward, hipStream_t st) {
    if (!family_flags_ok(a.family, a.flags)) return MAS_ERR_RANGE;
    if (int e = loss_dims_status(a.N, a.C, a.H, a.W, a.S, true)) return e;
    switch (a.C) {              // (an unknown spx_dtype is MAS_ERR_DTYPE from dispatch_loss_ids, for every entry point)
        case 19: return dispatch_loss_ids<19, true>(a, spx_dtype, backward, st);
        case 20: return dispatch_loss_ids<20, true>(a, spx_dtype, backward, st);
        case 21: return dispatch_loss_ids<21, true>(a, spx_dtype, backward, st);
        default: return dispatch_loss_ids<MAS_MAX_CLASSES, false>(a, spx_dtype, backward, st);
    }
}

// k_group_finalize behind a scan, in few workgroups: every one of them ends in atomics on the same accumulator words -- with 640 of
// them those serialised at the L2 for 40 us, measured; 64 x 256 threads x 10 entries each is 4 us.  So 8 x 256 entries per workgroup,
// 64 workgroups at the most.  (mas_group_finalize, the entry point of its own, has its own grid.)
template <bool WG>
int launch_group_finalize(const mas_u64* gmax, const unsigned* tmax, long long n_entries, mas_u64* acc, int flags, const float* w, float* values,
                          hipStream_t st) {
    long long nblk = (n_entries + 8 * kThreads - 1) / (8 * kThreads);
    if (nblk > 64) nblk = 64;
    hipLaunchKernelGGL(k_group_finalize<WG>, dim3((unsigned)nblk), dim3(kThreads), 0, st, gmax, tmax, n_entries, acc, flags, w, values);
    return mas_launch_status();
}

// w == NULL: losses [3]; else losses [4] with the weighted objective
int launch_loss_values(const mas_u64* acc, int flags, const float* w, float* losses, hipStream_t st) {
    hipLaunchKernelGGL(k_loss_values_weighted, dim3(1), dim3(64), 0, st, acc, flags, w, losses);
    return mas_launch_status();
}

// w == NULL: grad [3], the upstream gradient of every loss; else grad [1], the upstream gradient of the weighted objective
int launch_loss_scales(const mas_u64* acc, const float* grad, const float* w, int flags, float* scale, hipStream_t st) {
    hipLaunchKernelGGL(k_loss_scales_weighted, dim3(1), dim3(64), 0, st, acc, grad, w, flags, scale);
    return mas_launch_status();
}

}  // namespace

extern "C" int mas_target_bits(const uint8_t* targets, int64_t n_rows, int cols_stored, int cols_used, uint32_t* bits,
                               void* stream) {
    if (!targets || !bits) return MAS_ERR_NULL;
    if (n_rows <= 0 || cols_stored <= 0) return MAS_ERR_SHAPE;
    if (cols_used < 1 || cols_used > cols_stored || cols_used > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    const long long nblk = (n_rows + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_target_bits, dim3((unsigned)nblk), dim3(kThreads), 0, static_cast<hipStream_t>(stream), targets,
                       (long long)n_rows, cols_stored, cols_used, bits);
    return mas_launch_status();
}

extern "C" int mas_partial_loss_fwd(const float* z, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits,
                                    int N, int C, int H, int W, int S, float invT, int flags, uint64_t* gmax, uint64_t* acc,
                                    void* stream) {
    if (!z || !spx || !mask || !bits || !acc) return MAS_ERR_NULL;
    if ((flags & MAS_LOSS_GROUP) && !gmax) return MAS_ERR_NULL;
    return dispatch_loss(loss_args(FAMILY_PLAIN, z, 0, 0, spx, mask, bits, N, C, H, W, S, invT, flags, gmax, acc), spx_dtype, false,
                         static_cast<hipStream_t>(stream));
}

extern "C" int mas_group_finalize(const uint64_t* gmax, int64_t n_entries, uint64_t* acc, void* stream) {
    if (!gmax || !acc) return MAS_ERR_NULL;
    if (n_entries <= 0) return MAS_ERR_SHAPE;
    long long nblk = (n_entries + kThreads - 1) / kThreads;
    if (nblk > 1024) nblk = 1024;
    hipLaunchKernelGGL(k_group_finalize<false>, dim3((unsigned)nblk), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const mas_u64*>(gmax), static_cast<const unsigned*>(nullptr), (long long)n_entries, reinterpret_cast<mas_u64*>(acc), 0,
                       static_cast<const float*>(nullptr), static_cast<float*>(nullptr));
    return mas_launch_status();
}

extern "C" int mas_loss_values(const uint64_t* acc, int flags, float* losses, void* stream) {
    if (!acc || !losses) return MAS_ERR_NULL;
    return launch_loss_values(reinterpret_cast<const mas_u64*>(acc), flags, nullptr, losses, static_cast<hipStream_t>(stream));
}

extern "C" int mas_loss_values_weighted(const uint64_t* acc, int flags, const float* weights, float* losses4, void* stream) {
    if (!acc || !weights || !losses4) return MAS_ERR_NULL;
    return launch_loss_values(reinterpret_cast<const mas_u64*>(acc), flags, weights, losses4, static_cast<hipStream_t>(stream));
}

extern "C" int mas_loss_scales_weighted(const uint64_t* acc, const float* grad_total, const float* weights, int flags, float* scale,
                                        void* stream) {
    if (!acc || !grad_total || !weights || !scale) return MAS_ERR_NULL;
    return launch_loss_scales(reinterpret_cast<const mas_u64*>(acc), grad_total, weights, flags, scale, static_cast<hipStream_t>(stream));
}

extern "C" int mas_loss_scales(const uint64_t* acc, const float* grad_out, int flags, float* scale, void* stream) {
    if (!acc || !grad_out || !scale) return MAS_ERR_NULL;
    return launch_loss_scales(reinterpret_cast<const mas_u64*>(acc), grad_out, nullptr, flags, scale, static_cast<hipStream_t>(stream));
}

extern "C" int mas_partial_loss_bwd(const float* z, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits,
                                    const uint64_t* gmax, const float* scale, int N, int C, int H, int W, int S, float invT,
                                    int flags, float* dz, void* stream) {
    if (!z || !spx || !mask || !bits || !scale || !dz) return MAS_ERR_NULL;
    if ((flags & MAS_LOSS_GROUP) && !gmax) return MAS_ERR_NULL;
    return dispatch_loss(loss_args(FAMILY_PLAIN, z, 0, 0, spx, mask, bits, N, C, H, W, S, invT, flags, gmax, nullptr, scale, dz), spx_dtype,
                         true, static_cast<hipStream_t>(stream));
}

// ---- quarter-resolution forms: the x4 bilinear upsampling of the logits (models/segmentation/utils.py:25) is evaluated per
// selected pixel inside the scans; forward results are bit-identical to mas_partial_loss_fwd on the materialised tensor.
extern "C" int mas_partial_loss_fwd_lowres(const float* zq, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
                                           const uint32_t* bits, int N, int C, int H, int W, int S, float invT, int flags,
                                           uint64_t* gmax, uint64_t* acc, void* stream) {
    if (!zq || !spx || !mask || !bits || !acc) return MAS_ERR_NULL;
    if ((flags & MAS_LOSS_GROUP) && !gmax) return MAS_ERR_NULL;
    if (h <= 0 || w <= 0 || h > H || w > W) return MAS_ERR_SHAPE;
    return dispatch_loss(loss_args(FAMILY_PLAIN, zq, h, w, spx, mask, bits, N, C, H, W, S, invT, flags, gmax, acc), spx_dtype, false,
                         static_cast<hipStream_t>(stream));
}

extern "C" int mas_partial_loss_bwd_lowres(const float* zq, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
                                           const uint32_t* bits, const uint64_t* gmax, const float* scale, int N, int C, int H, int W,
                                           int S, float invT, int flags, int64_t* dzq_fix, void* stream) {
    if (!zq || !spx || !mask || !bits || !scale || !dzq_fix) return MAS_ERR_NULL;
    if ((flags & MAS_LOSS_GROUP) && !gmax) return MAS_ERR_NULL;
    if (h <= 0 || w <= 0 || h > H || w > W) return MAS_ERR_SHAPE;
    return dispatch_loss(loss_args(FAMILY_PLAIN, zq, h, w, spx, mask, bits, N, C, H, W, S, invT, flags, gmax, nullptr, scale, nullptr, dzq_fix),
                         spx_dtype, true, static_cast<hipStream_t>(stream));
}

namespace {
__global__ __launch_bounds__(kThreads) void k_fix_to_float(const long long* __restrict__ fix, long long n, int frac, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    union { double d; mas_u64 u; } s;
    s.u = (mas_u64)(1023 - frac) << 52;
    out[i] = (float)((double)fix[i] * s.d);
}
}  // namespace

extern "C" int mas_fix_to_float(const int64_t* fix, int64_t n, int frac_bits, float* out, void* stream) {
    if (!fix || !out) return MAS_ERR_NULL;
    if (n <= 0 || frac_bits < 0 || frac_bits > 62) return MAS_ERR_SHAPE;
    hipLaunchKernelGGL(k_fix_to_float, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(fix), (long long)n, frac_bits, out);
    return mas_launch_status();
}

// ---- fused forms: one call = every launch of a direction ---------------------------------------------------------------------------
// forward : k_loss_prep (zero acc + table, target rows -> bit masks)  ->  forward scan  ->  k_group_finalize whose last workgroup
//           writes the loss values (3 launches; were: memset, k_target_bits, scan, k_group_finalize, k_loss_values[_weighted])
// backward: (LOWRES: memset of the fixed-point accumulator)  ->  backward scan that forms its scale factors itself  ->  (LOWRES:
//           k_fix_to_float)   (1 / 3 launches; were: k_loss_scales[_weighted], scan / memset, k_loss_scales, scan, k_fix_to_float)
// Same kernels, same arithmetic, same bits as the step-by-step entry points above (tests/test_losses_gpu.py compares both with
// oracle/exact.c).  Reference: trainer/active_joint_multi_predignore_lossdecomp.py:21-72, ..._mclossablation2.py:22-79.
namespace {
struct WorkLayout { size_t gmax_off, bits_off, bytes; };
inline WorkLayout work_layout(int N, int S, int C, int flags) {
    WorkLayout L;
    L.gmax_off = 8 * sizeof(mas_u64);
    const size_t g = (flags & MAS_LOSS_GROUP) ? (size_t)N * S * C * sizeof(mas_u64) : 0;
    L.bits_off = L.gmax_off + g;
    L.bytes = L.bits_off + (size_t)N * S * sizeof(unsigned);
    return L;
}
}  // namespace

extern "C" size_t mas_partial_loss_work_bytes(int N, int S, int C, int flags) {
    if (N <= 0 || S <= 0 || C <= 0) return 0;
    return work_layout(N, S, C, flags).bytes;
}

extern "C" int mas_partial_loss_fwd_fused(const float* z, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
                                          const uint8_t* targets, int cols_stored, int cols_used, const uint32_t* bits, int N, int C, int H,
                                          int W, int S, float invT, int flags, const float* weights, void* work, size_t work_bytes,
                                          float* losses, void* stream) {
    if (!z || !spx || !mask || !work || (!targets && !bits)) return MAS_ERR_NULL;
    if (!loss_flags_ok(flags)) return MAS_ERR_RANGE;
    if (int e = loss_dims_status(N, C, H, W, S, false)) return e;
    if ((h > 0) != (w > 0) || h > H || w > W) return MAS_ERR_SHAPE;
    if (targets && (cols_stored <= 0 || cols_used < 1 || cols_used > cols_stored || cols_used > MAS_MAX_CLASSES)) return MAS_ERR_CLASSES;
    const WorkLayout L = work_layout(N, S, C, flags);
    if (work_bytes < L.bytes) return MAS_ERR_WORKSPACE;
    if ((uintptr_t)work % 8 != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char* wb = static_cast<unsigned char*>(work);
    mas_u64* acc = reinterpret_cast<mas_u64*>(wb);
    mas_u64* gmax = (flags & MAS_LOSS_GROUP) ? reinterpret_cast<mas_u64*>(wb + L.gmax_off) : nullptr;
    unsigned* wbits = reinterpret_cast<unsigned*>(wb + L.bits_off);
    const long long n_zero = (long long)(L.bits_off / sizeof(mas_u64)), n_rows = (long long)N * S;
    const long long n_prep = n_zero > n_rows ? n_zero : n_rows;
    hipLaunchKernelGGL(k_loss_prep, dim3((unsigned)((n_prep + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, acc, n_zero, targets, n_rows,
                       cols_stored, cols_used, wbits);
    if (int e = mas_launch_status()) return e;
    const LossArgs a = loss_args(FAMILY_PLAIN, z, h, w, spx, mask, targets ? wbits : bits, N, C, H, W, S, invT, flags, gmax, acc);
    if (int e = dispatch_loss(a, spx_dtype, false, st)) return e;
    if (gmax) return launch_group_finalize<false>(gmax, nullptr, (long long)N * S * C, acc, flags, weights, losses, st);
    if (losses) return launch_loss_values(acc, flags, weights, losses, st);
    return mas_launch_status();
}

extern "C" int mas_partial_loss_bwd_fused(const float* z, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits,
                                          const void* work, const float* grad, const float* weights, int N, int C, int H, int W, int S,
                                          float invT, int flags, float* dz, int64_t* dzq_fix, void* stream) {
    if (!z || !spx || !mask || !work || !grad || !dz) return MAS_ERR_NULL;
    if (!loss_flags_ok(flags)) return MAS_ERR_RANGE;
    if (int e = loss_dims_status(N, C, H, W, S, false)) return e;
    const bool low = h > 0;
    if ((h > 0) != (w > 0) || h > H || w > W) return MAS_ERR_SHAPE;
    if (low && !dzq_fix) return MAS_ERR_NULL;
    const WorkLayout L = work_layout(N, S, C, flags);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char* wb = static_cast<const unsigned char*>(work);
    const void* gmax = (flags & MAS_LOSS_GROUP) ? wb + L.gmax_off : nullptr;
    const unsigned* wbits = bits ? bits : reinterpret_cast<const unsigned*>(wb + L.bits_off);
    const size_t nq = low ? (size_t)N * C * h * w : 0;
    if (low) {
        const hipError_t e = hipMemsetAsync(dzq_fix, 0, nq * sizeof(int64_t), st);
        if (e != hipSuccess) return (int)e;
    }
    LossArgs a = loss_args(FAMILY_PLAIN, z, h, w, spx, mask, wbits, N, C, H, W, S, invT, flags, gmax, work, nullptr, dz, dzq_fix);
    a.grad = grad;              // (no scale factors: the scan forms them from the accumulators, the upstream gradient(s) and the weights)
    a.gw = weights;
    if (int e = dispatch_loss(a, spx_dtype, true, st)) return e;
    if (low) {
        hipLaunchKernelGGL(k_fix_to_float, dim3((unsigned)((nq + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           reinterpret_cast<const long long*>(dzq_fix), (long long)nq, MAS_GRAD_FRAC, dz);
        return mas_launch_status();
    }
    return 0;
}

// ---- the CPU-side statement of the spec: host pointers, a plain loop over the pixels through partial_label.h.  No device is touched.
// CE-family flags only (MAS_LOSS_CE with MAS_LOSS_DECOMP / MAS_LOSS_RC / MAS_LOSS_TOPONE); softmax in the operation order of
// mas_softmax_regs (common.h).  acc[0..4] are added to; losses (optional) = mas_loss_values(acc); dz (optional, with grad_out) = what
// mas_loss_scales + mas_partial_loss_bwd write.
extern "C" int mas_partial_loss_reference(const float* z, const void* spx, int spx_dtype, const uint8_t* mask, const uint32_t* bits, int N,
                                          int C, int H, int W, int S, float invT, int flags, const float* grad_out, uint64_t* acc,
                                          float* losses, float* dz) {
    if (!z || !spx || !mask || !bits || !acc || (dz && !grad_out)) return MAS_ERR_NULL;
    if (N <= 0 || H <= 0 || W <= 0 || S <= 0 || (long long)H * W > 0x7fffffffLL / 2) return MAS_ERR_SHAPE;
    if (C < 2 || C > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    if (spx_dtype != MAS_ID_I64 && spx_dtype != MAS_ID_I32 && spx_dtype != MAS_ID_U16) return MAS_ERR_DTYPE;
    if (!(flags & MAS_LOSS_CE) || (flags & ~(MAS_LOSS_CE | MAS_LOSS_DECOMP | MAS_LOSS_RC | MAS_LOSS_TOPONE)) || !loss_flags_ok(flags))
        return MAS_ERR_RANGE;
    const int mode = mas_pl_mode(flags);
    const size_t HW = (size_t)H * W;
    mas_u64* a64 = reinterpret_cast<mas_u64*>(acc);
    for (int pass = 0; pass < (dz ? 2 : 1); ++pass) {
        float sc3[3] = {0.f, 0.f, 0.f};
        if (pass == 1) {
            loss_scales_of(a64, grad_out, nullptr, flags, sc3);
            for (size_t i = 0; i < (size_t)N * C * HW; ++i) dz[i] = 0.0f;
        }
        const float a_ce = sc3[0] * invT, a_mc = sc3[1] * invT;
        for (int n = 0; n < N; ++n) {
            for (size_t i = 0; i < HW; ++i) {
                const size_t g = (size_t)n * HW + i;
                if (!mask[g]) continue;
                long long id;
                if (spx_dtype == MAS_ID_I64) id = static_cast<const long long*>(spx)[g];
                else if (spx_dtype == MAS_ID_I32) id = static_cast<const int*>(spx)[g];
                else id = static_cast<const unsigned short*>(spx)[g];
                if (id < 0 || id >= S) continue;
                const uint32_t Y = bits[(size_t)n * S + (size_t)id];
                const int nb = mas_pl_popcount(Y);
                if (nb == 0) { if (pass == 0) a64[ACC_N_EMPTY] += 1; continue; }
                float p[MAS_MAX_CLASSES];
                const float* zp = z + (size_t)n * C * HW + i;
                float m = zp[0];
                for (int c = 1; c < C; ++c) m = (zp[c * HW] > m) ? zp[c * HW] : m;
                const float negM = -(m * invT);
                float sum = 0.0f;
                for (int c = 0; c < C; ++c) {
                    p[c] = mas_expf_np(mas_fmaf(zp[c * HW], invT, negM));
                    sum = (c == 0) ? p[c] : (sum + p[c]);
                }
                const float rinv = 1.0f / sum;
                for (int c = 0; c < C; ++c) p[c] = p[c] * rinv;
                const int pm = nb == 1 ? MAS_PL_CHOICE : mode;
                if (pass == 0) {
                    const mas_u64 q = mas_fix(mas_pl_loss(p, C, C, Y, pm), MAS_LOSS_FRAC);
                    if (nb == 1) { a64[ACC_SUM_CE] += q; a64[ACC_N_CE] += 1; } else { a64[ACC_SUM_MC] += q; a64[ACC_N_MC] += 1; }
                } else {
                    const mas_pl_grad_ctx gk = mas_pl_grad_prepare(p, C, C, Y, pm, nb == 1 ? a_ce : a_mc);
                    for (int c = 0; c < C; ++c)
                        dz[((size_t)n * C + c) * HW + i] = mas_pl_grad(gk, pm, p[c], (int)((Y >> c) & 1u), c);
                }
            }
        }
        if (pass == 0 && losses) loss_values_of(a64, flags, nullptr, losses);
    }
    return 0;
}

// ---- teacher-gated candidate terms (teacher_terms.h): step-by-step entry points over the teacher-term kernels --------------------------
// Reference: trainer/active_joint_multi_predignore_top1plbl.py:19-82 (TopOnePlbl), ..._multient.py:16-70 (MultiChoiceEnt_).
namespace {
inline int teacher_args_ok(const float* z, const float* zt, int h, int w, const void* spx, const uint8_t* mask, const uint32_t* bits, int H, int W,
                           float invT_x, int flags) {
    if (!z || !spx || !mask || !bits) return MAS_ERR_NULL;
    if (!teacher_flags_ok(flags)) return MAS_ERR_RANGE;
    if ((flags & MAS_LOSS_TOP1) && !zt) return MAS_ERR_NULL;
    if (!(invT_x > 0.0f)) return MAS_ERR_RANGE;
    if ((h > 0) != (w > 0) || h < 0 || h > H || w > W) return MAS_ERR_SHAPE;
    return 0;
}
}  // namespace

extern "C" int mas_teacher_loss_fwd(const float* z, const float* zt, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
                                    const uint32_t* bits, int N, int C, int H, int W, int S, float invT, float invT_x, float plbl_th, int flags,
                                    uint64_t* gmax, uint64_t* acc, void* stream) {
    if (int e = teacher_args_ok(z, zt, h, w, spx, mask, bits, H, W, invT_x, flags)) return e;
    if (!acc || ((flags & MAS_LOSS_GROUP) && !gmax)) return MAS_ERR_NULL;
    LossArgs a = loss_args(FAMILY_TEACHER, z, h, w, spx, mask, bits, N, C, H, W, S, invT, flags, gmax, acc);
    a.te = TeacherIn{zt, invT_x, plbl_th, (flags & MAS_LOSS_WITHIN) ? 1 : 0};
    return dispatch_loss(a, spx_dtype, false, static_cast<hipStream_t>(stream));
}

extern "C" int mas_teacher_loss_bwd(const float* z, const float* zt, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
                                    const uint32_t* bits, const uint64_t* gmax, const float* scale, int N, int C, int H, int W, int S,
                                    float invT, float invT_x, float plbl_th, int flags, float* dz, int64_t* dzq_fix, void* stream) {
    if (int e = teacher_args_ok(z, zt, h, w, spx, mask, bits, H, W, invT_x, flags)) return e;
    if (!scale || (h > 0 ? !dzq_fix : !dz) || ((flags & MAS_LOSS_GROUP) && !gmax)) return MAS_ERR_NULL;
    LossArgs a = loss_args(FAMILY_TEACHER, z, h, w, spx, mask, bits, N, C, H, W, S, invT, flags, gmax, nullptr, scale, dz, dzq_fix);
    a.te = TeacherIn{zt, invT_x, plbl_th, (flags & MAS_LOSS_WITHIN) ? 1 : 0};
    return dispatch_loss(a, spx_dtype, true, static_cast<hipStream_t>(stream));
}

namespace {
// losses4 = (ce, mc, group, x): the first three as mas_loss_values, x = the fourth slot's sum / (1 + n)
__host__ __device__ __forceinline__ void teacher_values_of(const mas_u64* acc, int flags, float* out) {
    loss_values_of(acc, flags & ~(MAS_LOSS_TOP1 | MAS_LOSS_ENT | MAS_LOSS_WITHIN), nullptr, out);
    out[3] = loss_value(acc[ACC_SUM_X], acc[ACC_N_X]);
}
__host__ __device__ __forceinline__ void teacher_scales_of(const mas_u64* acc, const float* grad, int flags, float* scale) {
    loss_scales_of(acc, grad, nullptr, flags & ~(MAS_LOSS_TOP1 | MAS_LOSS_ENT | MAS_LOSS_WITHIN), scale);
    scale[3] = grad[3] / (float)(acc[ACC_N_X] + 1);
}
__global__ void k_teacher_loss_values(const mas_u64* __restrict__ acc, int flags, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    teacher_values_of(acc, flags, out);
}
__global__ void k_teacher_loss_scales(const mas_u64* __restrict__ acc, const float* __restrict__ grad, int flags, float* __restrict__ scale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    teacher_scales_of(acc, grad, flags, scale);
}
}  // namespace

extern "C" int mas_teacher_loss_values(const uint64_t* acc, int flags, float* losses4, void* stream) {
    if (!acc || !losses4) return MAS_ERR_NULL;
    if (!teacher_flags_ok(flags)) return MAS_ERR_RANGE;
    hipLaunchKernelGGL(k_teacher_loss_values, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const mas_u64*>(acc), flags,
                       losses4);
    return mas_launch_status();
}

extern "C" int mas_teacher_loss_scales(const uint64_t* acc, const float* grad_out4, int flags, float* scale4, void* stream) {
    if (!acc || !grad_out4 || !scale4) return MAS_ERR_NULL;
    if (!teacher_flags_ok(flags)) return MAS_ERR_RANGE;
    hipLaunchKernelGGL(k_teacher_loss_scales, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const mas_u64*>(acc),
                       grad_out4, flags, scale4);
    return mas_launch_status();
}

// ---- the CPU-side statement: host pointers, a plain loop over the pixels through partial_label.h and teacher_terms.h, every term the
// teacher-term kernels compute -- the merged-positive sums, the group table with its finalize, the fourth slot -- and dz in the
// operation order of the TT instantiations of k_partial_loss_bwd.  No device is touched.
extern "C" int mas_teacher_loss_reference(const float* z, const float* zt, const void* spx, int spx_dtype, const uint8_t* mask,
                                          const uint32_t* bits, int N, int C, int H, int W, int S, float invT, float invT_x, float plbl_th,
                                          int flags, const float* grad_out4, uint64_t* acc, uint64_t* gmax, float* losses4, float* dz) {
    if (int e = teacher_args_ok(z, zt, 0, 0, spx, mask, bits, H, W, invT_x, flags)) return e;
    if (!acc || (dz && !grad_out4) || ((flags & MAS_LOSS_GROUP) && !gmax)) return MAS_ERR_NULL;
    if (N <= 0 || H <= 0 || W <= 0 || S <= 0 || (long long)H * W > 0x7fffffffLL / 2) return MAS_ERR_SHAPE;
    if (C < 2 || C > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    if (spx_dtype != MAS_ID_I64 && spx_dtype != MAS_ID_I32 && spx_dtype != MAS_ID_U16) return MAS_ERR_DTYPE;
    const int tt = mas_tt_mode(flags), within = (flags & MAS_LOSS_WITHIN) ? 1 : 0;
    const bool do_ce = flags & MAS_LOSS_CE, do_group = flags & MAS_LOSS_GROUP, only_multi = flags & MAS_LOSS_GROUP_ONLY_MULTI;
    const size_t HW = (size_t)H * W;
    mas_u64* a64 = reinterpret_cast<mas_u64*>(acc);
    mas_u64* g64 = reinterpret_cast<mas_u64*>(gmax);
    for (int pass = 0; pass < (dz ? 2 : 1); ++pass) {
        float sc4[4] = {0.f, 0.f, 0.f, 0.f};
        if (pass == 1) {
            teacher_scales_of(a64, grad_out4, flags, sc4);
            for (size_t i = 0; i < (size_t)N * C * HW; ++i) dz[i] = 0.0f;
        }
        const float a_ce = sc4[0] * invT, a_mc = sc4[1] * invT, g6 = sc4[2] * invT, a_x = sc4[3] * invT_x;
        for (int n = 0; n < N; ++n) {
            for (size_t i = 0; i < HW; ++i) {
                const size_t g = (size_t)n * HW + i;
                if (!mask[g]) continue;
                long long id;
                if (spx_dtype == MAS_ID_I64) id = static_cast<const long long*>(spx)[g];
                else if (spx_dtype == MAS_ID_I32) id = static_cast<const int*>(spx)[g];
                else id = static_cast<const unsigned short*>(spx)[g];
                if (id < 0 || id >= S) continue;
                const uint32_t Y = bits[(size_t)n * S + (size_t)id];
                const int nb = mas_pl_popcount(Y);
                if (nb == 0) { if (pass == 0) a64[ACC_N_EMPTY] += 1; continue; }
                float v[MAS_MAX_CLASSES], u[MAS_MAX_CLASSES];
                for (int c = 0; c < C; ++c) v[c] = z[((size_t)n * C + c) * HW + i];
                // the fourth slot
                bool xon = false;
                uint32_t M = 0;
                if (nb > 1) {
                    xon = true;
                    if (tt == MAS_TT_TOP1) {
                        for (int c = 0; c < C; ++c) u[c] = zt[((size_t)n * C + c) * HW + i];
                        M = mas_tt_all(C);
                        mas_tt_softmax(u, C, C, M, invT_x);
                        xon = mas_tt_gate(u, C, C, Y, within, plbl_th) != 0;
                    } else {
                        M = mas_tt_ent_set(v, C, C, Y);
                    }
                    if (xon) {
                        for (int c = 0; c < C; ++c) u[c] = v[c];
                        mas_tt_softmax(u, C, C, M, invT_x);
                    }
                }
                mas_pl_grad_ctx gx = {};
                float ux = 0.0f;
                if (xon && pass == 0) {
                    const float l = (tt == MAS_TT_TOP1) ? mas_pl_loss(u, C, C, Y, MAS_PL_TOPONE) : mas_tt_ent_loss(u, C, C, M);
                    a64[ACC_SUM_X] += mas_fix(l, MAS_LOSS_FRAC);
                    a64[ACC_N_X] += 1;
                } else if (xon) {
                    if (tt == MAS_TT_TOP1) gx = mas_pl_grad_prepare(u, C, C, Y, MAS_PL_TOPONE, a_x);
                    else ux = mas_tt_ent_u(u, C, C, M);
                }
                // the scan's softmax (mas_softmax_regs)
                {
                    float m = v[0];
                    for (int c = 1; c < C; ++c) m = (v[c] > m) ? v[c] : m;
                    const float negM = -(m * invT);
                    float sum = 0.0f;
                    for (int c = 0; c < C; ++c) {
                        v[c] = mas_expf_np(mas_fmaf(v[c], invT, negM));
                        sum = (c == 0) ? v[c] : (sum + v[c]);
                    }
                    const float rinv = 1.0f / sum;
                    for (int c = 0; c < C; ++c) v[c] = v[c] * rinv;
                }
                const bool grp = do_group && (!only_multi || nb > 1);
                mas_u64* gm = g64 ? g64 + (size_t)n * S * C + (size_t)id * C : nullptr;
                if (pass == 0) {
                    if (do_ce) {
                        const mas_u64 q = mas_fix(mas_pl_loss(v, C, C, Y, MAS_PL_CHOICE), MAS_LOSS_FRAC);
                        if (nb == 1) { a64[ACC_SUM_CE] += q; a64[ACC_N_CE] += 1; } else { a64[ACC_SUM_MC] += q; a64[ACC_N_MC] += 1; }
                    }
                    if (grp) {
                        for (int c = 0; c < C; ++c) {
                            if ((Y >> c) & 1u) {
                                const mas_u64 w64 = ((mas_u64)mas_f2u(v[c]) << 32) | (mas_u64)(0xffffffffu - (unsigned)i);
                                if (w64 > gm[c]) gm[c] = w64;
                            }
                        }
                    }
                    continue;
                }
                float coef = 0.0f, pos = 0.0f;
                if (do_ce) {
                    pos = mas_pl_pos(v, C, C, Y);
                    coef = ((nb == 1) ? a_ce : a_mc) * (1.0f / (pos + 1e-8f));
                }
                unsigned A = 0;
                float ug = 0.0f;
                float t[MAS_MAX_CLASSES];
                for (int c = 0; c < C; ++c) t[c] = 0.0f;
                if (grp) {
                    const unsigned key = 0xffffffffu - (unsigned)i;
                    for (int c = 0; c < C; ++c) {
                        if ((Y >> c) & 1u) {
                            const mas_u64 w64 = gm[c];
                            if ((unsigned)w64 == key && (unsigned)(w64 >> 32) != 0u) {
                                A |= 1u << c;
                                t[c] = -(g6 / (v[c] + 1e-8f));
                                ug = ug + t[c] * v[c];
                            }
                        }
                    }
                }
                for (int c = 0; c < C; ++c) {
                    const float p = v[c];
                    const float yj = ((Y >> c) & 1u) ? 1.0f : 0.0f;
                    float d = coef * (p * (pos - yj));
                    if (A) {
                        if ((A >> c) & 1u) d = d + t[c] * p;
                        d = d - p * ug;
                    }
                    if (xon) d = d + ((tt == MAS_TT_TOP1) ? mas_pl_grad(gx, MAS_PL_TOPONE, u[c], (int)((Y >> c) & 1u), c)
                                                          : mas_tt_ent_grad(a_x, ux, u[c], (int)((M >> c) & 1u)));
                    dz[((size_t)n * C + c) * HW + i] = d;
                }
            }
        }
        if (pass == 0) {
            if (do_group) {             // k_group_finalize
                for (size_t e = 0; e < (size_t)N * S * C; ++e) {
                    const unsigned pb = (unsigned)(g64[e] >> 32);
                    if (pb) { a64[ACC_SUM_GROUP] += mas_fix(-mas_logf(mas_u2f(pb) + 1e-8f), MAS_LOSS_FRAC); a64[ACC_N_GROUP] += 1; }
                }
            }
            if (losses4) teacher_values_of(a64, flags, losses4);
        }
    }
    return 0;
}

// ---- teacher-weighted group term (teacher_terms.h, wgroup): the MAS_TT_WGROUP scans and the weighted finalize ------------------------------
// Reference: trainer/active_joint_multi_predignore_wgroup.py:12-82 (WeightedGroupMultiLabelCE).
namespace {
inline int wgroup_args_ok(const float* z, const float* zt, int h, int w, const void* spx, const uint8_t* mask, const uint32_t* bits,
                          const uint64_t* gmax, const uint32_t* tmax, int H, int W, int flags) {
    if (!wgroup_flags_ok(flags)) return MAS_ERR_RANGE;
    if (!zt) return MAS_ERR_RANGE;              // (the flag without a teacher: a combination, not a missing buffer)
    if (!z || !spx || !mask || !bits || !gmax || !tmax) return MAS_ERR_NULL;
    if ((h > 0) != (w > 0) || h < 0 || h > H || w > W) return MAS_ERR_SHAPE;
    return 0;
}
}  // namespace

extern "C" int mas_wgroup_loss_fwd(const float* z, const float* zt, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
                                   const uint32_t* bits, int N, int C, int H, int W, int S, float invT, int flags, uint64_t* gmax,
                                   uint32_t* tmax, uint64_t* acc, float* losses, void* stream) {
    if (int e = wgroup_args_ok(z, zt, h, w, spx, mask, bits, gmax, tmax, H, W, flags)) return e;
    if (!acc) return MAS_ERR_NULL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LossArgs a = loss_args(FAMILY_WGROUP, z, h, w, spx, mask, bits, N, C, H, W, S, invT, flags, gmax, acc);
    a.te = TeacherIn{zt, invT, 0.f, 0, tmax};
    if (int e = dispatch_loss(a, spx_dtype, false, st)) return e;
    return launch_group_finalize<true>(a.gmax, tmax, (long long)N * S * C, a.acc, flags & ~MAS_LOSS_WGROUP, nullptr, losses, st);
}

extern "C" int mas_wgroup_loss_bwd(const float* z, const float* zt, int h, int w, const void* spx, int spx_dtype, const uint8_t* mask,
                                   const uint32_t* bits, const uint64_t* gmax, const uint32_t* tmax, const float* scale, int N, int C, int H,
                                   int W, int S, float invT, int flags, float* dz, int64_t* dzq_fix, void* stream) {
    if (int e = wgroup_args_ok(z, zt, h, w, spx, mask, bits, gmax, tmax, H, W, flags)) return e;
    if (!scale || (h > 0 ? !dzq_fix : !dz)) return MAS_ERR_NULL;
    LossArgs a = loss_args(FAMILY_WGROUP, z, h, w, spx, mask, bits, N, C, H, W, S, invT, flags, gmax, nullptr, scale, dz, dzq_fix);
    a.te = TeacherIn{zt, invT, 0.f, 0, const_cast<unsigned*>(static_cast<const unsigned*>(tmax))};
    return dispatch_loss(a, spx_dtype, true, static_cast<hipStream_t>(stream));
}

// ---- the CPU-side statement: host pointers, a plain loop through partial_label.h and teacher_terms.h -- the merged-positive sums, both
// tables, the weighted finalize and dz in the operation order of the MAS_TT_WGROUP instantiations.  No device is touched.
extern "C" int mas_wgroup_loss_reference(const float* z, const float* zt, const void* spx, int spx_dtype, const uint8_t* mask,
                                         const uint32_t* bits, int N, int C, int H, int W, int S, float invT, int flags, const float* grad_out,
                                         uint64_t* acc, uint64_t* gmax, uint32_t* tmax, float* losses, float* dz) {
    if (int e = wgroup_args_ok(z, zt, 0, 0, spx, mask, bits, gmax, tmax, H, W, flags)) return e;
    if (!acc || (dz && !grad_out)) return MAS_ERR_NULL;
    if (N <= 0 || H <= 0 || W <= 0 || S <= 0 || (long long)H * W > 0x7fffffffLL / 2) return MAS_ERR_SHAPE;
    if (C < 2 || C > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    if (spx_dtype != MAS_ID_I64 && spx_dtype != MAS_ID_I32 && spx_dtype != MAS_ID_U16) return MAS_ERR_DTYPE;
    const bool do_ce = flags & MAS_LOSS_CE, only_multi = flags & MAS_LOSS_GROUP_ONLY_MULTI;
    const int vflags = flags & ~MAS_LOSS_WGROUP;
    const size_t HW = (size_t)H * W;
    mas_u64* a64 = reinterpret_cast<mas_u64*>(acc);
    mas_u64* g64 = reinterpret_cast<mas_u64*>(gmax);
    for (int pass = 0; pass < (dz ? 2 : 1); ++pass) {
        float sc3[3] = {0.f, 0.f, 0.f};
        if (pass == 1) {
            loss_scales_of(a64, grad_out, nullptr, vflags, sc3);
            for (size_t i = 0; i < (size_t)N * C * HW; ++i) dz[i] = 0.0f;
        }
        const float a_ce = sc3[0] * invT, a_mc = sc3[1] * invT, g6 = sc3[2] * invT;
        for (int n = 0; n < N; ++n) {
            for (size_t i = 0; i < HW; ++i) {
                const size_t g = (size_t)n * HW + i;
                if (!mask[g]) continue;
                long long id;
                if (spx_dtype == MAS_ID_I64) id = static_cast<const long long*>(spx)[g];
                else if (spx_dtype == MAS_ID_I32) id = static_cast<const int*>(spx)[g];
                else id = static_cast<const unsigned short*>(spx)[g];
                if (id < 0 || id >= S) continue;
                const uint32_t Y = bits[(size_t)n * S + (size_t)id];
                const int nb = mas_pl_popcount(Y);
                if (nb == 0) { if (pass == 0) a64[ACC_N_EMPTY] += 1; continue; }
                float v[MAS_MAX_CLASSES], u[MAS_MAX_CLASSES];
                for (int c = 0; c < C; ++c) v[c] = z[((size_t)n * C + c) * HW + i];
                mas_tt_wg_probs(v, C, invT);
                const bool grp = !only_multi || nb > 1;
                mas_u64* gm = g64 + ((size_t)n * S + (size_t)id) * C;
                uint32_t* tm = tmax + ((size_t)n * S + (size_t)id) * C;
                if (pass == 0) {
                    if (do_ce) {
                        const mas_u64 q = mas_fix(mas_pl_loss(v, C, C, Y, MAS_PL_CHOICE), MAS_LOSS_FRAC);
                        if (nb == 1) { a64[ACC_SUM_CE] += q; a64[ACC_N_CE] += 1; } else { a64[ACC_SUM_MC] += q; a64[ACC_N_MC] += 1; }
                    }
                    if (grp) {
                        for (int c = 0; c < C; ++c) u[c] = zt[((size_t)n * C + c) * HW + i];
                        mas_tt_wg_probs(u, C, invT);
                        for (int c = 0; c < C; ++c) {
                            if ((Y >> c) & 1u) {
                                const mas_u64 w64 = ((mas_u64)mas_f2u(v[c]) << 32) | (mas_u64)(0xffffffffu - (unsigned)i);
                                if (w64 > gm[c]) gm[c] = w64;
                                const uint32_t tb = mas_f2u(u[c]);
                                if (tb > tm[c]) tm[c] = tb;
                            }
                        }
                    }
                    continue;
                }
                float coef = 0.0f, pos = 0.0f;
                if (do_ce) {
                    pos = mas_pl_pos(v, C, C, Y);
                    coef = ((nb == 1) ? a_ce : a_mc) * (1.0f / (pos + 1e-8f));
                }
                unsigned A = 0;
                float ug = 0.0f;
                float t[MAS_MAX_CLASSES];
                for (int c = 0; c < C; ++c) t[c] = 0.0f;
                if (grp) {
                    const unsigned key = 0xffffffffu - (unsigned)i;
                    for (int c = 0; c < C; ++c) {
                        if ((Y >> c) & 1u) {
                            const mas_u64 w64 = gm[c];
                            if ((unsigned)w64 == key && (unsigned)(w64 >> 32) != 0u) {
                                A |= 1u << c;
                                t[c] = mas_tt_wg_coef(g6, mas_u2f(tm[c]), v[c]);
                                ug = ug + t[c] * v[c];
                            }
                        }
                    }
                }
                for (int c = 0; c < C; ++c) {
                    const float p = v[c];
                    const float yj = ((Y >> c) & 1u) ? 1.0f : 0.0f;
                    float d = coef * (p * (pos - yj));
                    if (A) {
                        if ((A >> c) & 1u) d = d + t[c] * p;
                        d = d - p * ug;
                    }
                    dz[((size_t)n * C + c) * HW + i] = d;
                }
            }
        }
        if (pass == 0) {
            for (size_t e = 0; e < (size_t)N * S * C; ++e) {             // k_group_finalize<true>
                const unsigned pb = (unsigned)(g64[e] >> 32);
                if (pb) { a64[ACC_SUM_GROUP] += mas_fix(mas_tt_wg_loss(mas_u2f(tmax[e]), mas_u2f(pb)), MAS_LOSS_FRAC); a64[ACC_N_GROUP] += 1; }
            }
            if (losses) loss_values_of(a64, vflags, nullptr, losses);
        }
    }
    return 0;
}
