// candidate_plbl.hip -- one label per pixel for the stage-2 generators that do not expand: the arg-max within the superpixel's candidate
// set (or a label map decided elsewhere) under the mask, a confidence-thresholded top-1 outside it, straight from quarter-resolution
// logits, with the MeanIoU counters of the result.
//
// Reference: trainer/eval_save_candidateplbl.py:53 (top_pseudo_label_generation, eval_within_multihot.py:93-146),
// trainer/eval_save_candidateplbl_prop.py:46-59 and trainer/eval_save_cosplbl_naiveprop.py:54-67 (the same fallback over the labels of
// eval_save_cosplbl.pseudo_label_generation), each followed by MeanIoU._after_step (utils/miou.py:23-38).  feat_forward's logits are
// upsampled x4 to the picture first; materialised they are 168 MB per 1024 x 2048 picture, and top_pseudo_label_generation gathers an
// HW x C copy of the multi-hot rows next to them.  Here each pixel's C values exist in registers only, one at a time.
//
// Arithmetic (normative; tests/candidate_plbl_restated.py restates it in numpy):
//   1. interpolation: step 1 of naive_plbl.hip -- the tap and the expression of k_upsample_fwd (upsample_tap.h), scale =
//      (float)h / (float)H on the host, so y_c equals mas_upsample_bilinear_fwd's output bit for bit.  Identity geometry: the logit.
//   2. under the mask, candidate mode: s = spx[p]; v_c = y_c * (float)((bits[n,s] >> c) & 1), the multiplication done literally (an
//      excluded channel gives +-0, a NaN stays NaN, +-inf * 0 is NaN); label = the first maximum of v_c in channel order by
//      arg_update's rule (strict '>', the first NaN wins) -- (valid_output * trg_pixel).max(dim=1)[1], including the reference's quirk
//      that a superpixel whose candidate logits are all negative gets the first excluded channel.  An id outside [0, S) reads no row
//      and gives 255.
//   3. under the mask, map mode: label = inner[p] narrowed to u8.
//   4. outside the mask, fallback off: 255.
//   5. outside the mask, fallback on: p_max = 1 / sum_c expf((y_c - y_max) * inv_T), channel order, the sum starts from 0; label =
//      the first arg-max of y if p_max > th, else 255 (a NaN logit gives p_max NaN, i.e. 255).  The reference takes the arg-max of the
//      probabilities, which differs only when the two largest round to the same float; the softmax is not bit-equal to torch.softmax
//      (naive_plbl.hip lives with both).
//   6. counters (optional): tally() of iou_tally.h with K = num_classes, no "undefined" triple, into per-workgroup LDS u32 counters;
//      one 64-bit global atomic per non-zero counter: integer sums, the same on every run.
//
// Shape: that of k_naive_plbl.  A workgroup owns a 16 x 64 output tile, a thread 4 consecutive pixels of one row; the tile's
// quarter-resolution footprint (nrq x ncq, exact maxima over tiles from the host) is staged in LDS for `cb` channels at a time.  Pass 0
// takes the arg-max each pixel needs (candidate under the mask, global outside it; see Pixels); a second walk over the channel blocks
// for the exp sum runs only with the fallback.  A pixel's bits row is one 4-byte load (neighbouring pixels mostly share it: the rows
// are not staged).
#include "common.h"
#include "iou_tally.h"
#include "upsample_tap.h"

namespace {
constexpr int kTH = 16, kTW = 64;          // output tile
constexpr int kThreads = 256;              // 16 lanes x 4 pixels per row, 16 rows
constexpr int kPix = 4;
constexpr size_t kLdsBudget = 32 * 1024;   // staged logits
constexpr int kMaxCnt = 3 * (MAS_MAX_CLASSES + 1);

struct CandArgs {
    const float* z;               // [N,C,h,w]
    const unsigned char* mask;    // [N,H,W]
    const long long* spx;         // [N,H,W]  (candidate mode)
    const int* bits;              // [N,S]    (candidate mode)
    const long long* inner;       // [N,H,W]  (map mode)
    const long long* tgt;         // [N,H,W] or NULL
    mas_u64* counts;              // [3K+3] or NULL
    unsigned char* out;           // [N,H,W]
    long long ignore_label;
    int C, h, w, H, W, S, K;
    float sh, sw, th, inv_T;
    int fallback;
    int nrq, ncq, cb;             // LDS extents (quarter rows, quarter columns of one tile) and channels per staged block
    int vec_ok;                   // mask and labels are 4-byte aligned and W % 4 == 0: 32-bit mask loads and label stores
};

// What a thread knows of its four pixels before the channel walk.  A pixel needs ONE arg-max: under the mask that of the products
// (candidate mode) or none (map mode), outside it that of the logits.  So the walk keeps one (best, idx) per pixel and multiplies by the
// row bit everywhere in candidate mode, with a row of ones where the pixel is not under the mask or its id reads no row: y * 1.0f is y.
struct Pixels {
    unsigned flags;               // bit k: the mask byte of pixel k is non-zero; bit 4 + k: ... and its id lies in [0, S) (candidate mode)
    unsigned row[kPix];           // candidate mode: the bits row, or ones
};

__device__ __forceinline__ void load_pixels(const CandArgs& a, size_t base, int n, bool vec, Pixels& p) {
    p.flags = 0u;
    if (vec) {
        const unsigned m = *reinterpret_cast<const unsigned*>(a.mask + base);
#pragma unroll
        for (int k = 0; k < kPix; ++k) p.flags |= ((m >> (8 * k)) & 0xffu) ? 1u << k : 0u;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) p.flags |= (k < n && a.mask[base + k]) ? 1u << k : 0u;
    }
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        p.row[k] = 0xffffffffu;
        if (a.spx && ((p.flags >> k) & 1u)) {
            const long long s = a.spx[base + k];
            if (s >= 0 && s < a.S) {
                p.flags |= 16u << k;
                p.row[k] = (unsigned)a.bits[(size_t)blockIdx.z * a.S + (size_t)s];
            }
        }
    }
}

// pass 0, channel c of one pixel: the arg-max of the logits, in candidate mode of the products with the row's bits
__device__ __forceinline__ void walk_argmax(bool cand, unsigned row, int c, float v, float& best, int& idx) {
    if (cand) v = v * (float)((row >> c) & 1u);
    if (c == 0) best = v;
    else arg_update(v, c, best, idx);
}

__device__ __forceinline__ void clear_counts(unsigned* s_cnt, int n) {
    for (int i = threadIdx.x; i < n; i += kThreads) s_cnt[i] = 0;
}

// labels of the thread's pixels, their store, and (with counts) the tally and the workgroup's flush; called by every thread
__device__ __forceinline__ void finish(const CandArgs& a, unsigned* s_cnt, size_t base, int n, bool vec, unsigned flags,
                                       const int (&idx)[kPix], const float (&sum)[kPix]) {
    unsigned char v[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        unsigned char lab = 255;
        if ((flags >> k) & 1u) {                      // (only pixels of the picture: k < n)
            if (a.spx) lab = ((flags >> (4 + k)) & 1u) ? (unsigned char)idx[k] : (unsigned char)255;
            else lab = (unsigned char)a.inner[base + k];
        } else if (a.fallback && (1.0f / sum[k]) > a.th) {
            lab = (unsigned char)idx[k];
        }
        v[k] = lab;
    }
    if (vec) {
        *reinterpret_cast<unsigned*>(a.out + base) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
    } else {
        for (int k = 0; k < n; ++k) a.out[base + k] = v[k];
    }
    if (!a.counts) return;                            // (uniform over the grid)
    for (int k = 0; k < n; ++k) tally(s_cnt, a.K, a.tgt[base + k], v[k], v[k], a.ignore_label, false);
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * a.K + 3; i += kThreads)
        if (s_cnt[i]) atomicAdd(&a.counts[i], (mas_u64)s_cnt[i]);
}

// grid: (ceil(W / kTW), ceil(H / kTH), N); dynamic LDS: cb * nrq * ncq floats
__global__ __launch_bounds__(kThreads) void k_candidate_plbl(const CandArgs a) {
    extern __shared__ float lds[];
    __shared__ unsigned s_cnt[kMaxCnt];
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, C = a.C, h = a.h, w = a.w;
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    const int y1 = min(y0 + kTH, H) - 1, x1 = min(x0 + kTW, W) - 1;
    const int py = y0 + tid / (kTW / kPix), px0 = x0 + (tid % (kTW / kPix)) * kPix;
    const bool live = py < H && px0 < W;
    const int n = live ? min(kPix, W - px0) : 0;
    const int cy = min(py, y1);
    const int q_lo = make_tap(a.sh, y0, h).i0, q_hi = make_tap(a.sh, y1, h).i1;
    const int c_lo = make_tap(a.sw, x0, w).i0, c_hi = make_tap(a.sw, x1, w).i1;
    const int nq = q_hi - q_lo + 1, nc = c_hi - c_lo + 1;
    const size_t plane = (size_t)H * W, base = (size_t)blockIdx.z * plane + (size_t)cy * W + (live ? px0 : 0);
    const bool vec = n == kPix && a.vec_ok;
    if (nq > a.nrq || nc > a.ncq) {                   // (uniform over the workgroup; the host sized the extents -- never taken)
        for (int k = 0; k < n; ++k) a.out[base + k] = 255;
        return;
    }
    Pixels p;
    load_pixels(a, base, n, vec, p);
    if (a.counts) clear_counts(s_cnt, 3 * a.K + 3);   // (the first staging barrier orders it before any tally)
    const Tap ty = make_tap(a.sh, cy, h);
    const int r0 = (ty.i0 - q_lo) * a.ncq, r1 = (ty.i1 - q_lo) * a.ncq;
    Tap tx[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) tx[k] = make_tap(a.sw, min(px0 + k, x1), w);
    const size_t qplane = (size_t)h * w;
    const float* zq = a.z + (size_t)blockIdx.z * C * qplane;
    const int tile = a.nrq * a.ncq;
    const bool cand = a.spx != nullptr;
    float best[kPix], sum[kPix];
    int idx[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) best[k] = 0.0f, sum[k] = 0.0f, idx[k] = 0;
    // one walk over the channel blocks; `use(k, c, v)` takes channel c of pixel k
    auto walk = [&](auto use) {
        for (int c0 = 0; c0 < C; c0 += a.cb) {
            const int nb = min(a.cb, C - c0);
            __syncthreads();                          // (the previous block's reads are done)
            // (not vectorised: the vectoriser's copy of the index arithmetic is the kernel's register peak, 84 against 70, and costs
            // two waves per SIMD for some seven elements per thread)
#pragma clang loop vectorize(disable)
            for (int i = tid; i < nb * nq * nc; i += kThreads) {
                const int cc = i / (nq * nc), rem = i - cc * (nq * nc), r = rem / nc, col = rem - r * nc;
                lds[cc * tile + r * a.ncq + col] = zq[(size_t)(c0 + cc) * qplane + (size_t)(q_lo + r) * w + c_lo + col];
            }
            __syncthreads();
            for (int cc = 0; cc < nb; ++cc) {
                const float* q = lds + cc * tile;
#pragma unroll
                for (int k = 0; k < kPix; ++k) {
                    const int i0 = tx[k].i0 - c_lo, i1 = tx[k].i1 - c_lo;
                    use(k, c0 + cc, ty.l0 * (tx[k].l0 * q[r0 + i0] + tx[k].l1 * q[r0 + i1]) +
                                    ty.l1 * (tx[k].l0 * q[r1 + i0] + tx[k].l1 * q[r1 + i1]));
                }
            }
        }
    };
    walk([&](int k, int c, float v) { walk_argmax(cand, p.row[k], c, v, best[k], idx[k]); });
    if (a.fallback) walk([&](int k, int, float v) { sum[k] = sum[k] + expf((v - best[k]) * a.inv_T); });
    finish(a, s_cnt, base, n, vec, p.flags, idx, sum);
}

// identity geometry (h == H, w == W): the logits themselves, read in place
__global__ __launch_bounds__(kThreads) void k_candidate_plbl_identity(const CandArgs a) {
    __shared__ unsigned s_cnt[kMaxCnt];
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, C = a.C;
    const int py = blockIdx.y * kTH + tid / (kTW / kPix), px0 = blockIdx.x * kTW + (tid % (kTW / kPix)) * kPix;
    const bool live = py < H && px0 < W;
    const int n = live ? min(kPix, W - px0) : 0;
    const size_t plane = (size_t)H * W, pix = live ? (size_t)py * W + px0 : 0, base = (size_t)blockIdx.z * plane + pix;
    const bool vec = n == kPix && a.vec_ok;
    Pixels p;
    load_pixels(a, base, n, vec, p);
    if (a.counts) {
        clear_counts(s_cnt, 3 * a.K + 3);
        __syncthreads();
    }
    const float* z = a.z + (size_t)blockIdx.z * C * plane + pix;
    const bool cand = a.spx != nullptr;
    float best[kPix], sum[kPix];
    int idx[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) best[k] = 0.0f, sum[k] = 0.0f, idx[k] = 0;
    if (live) {
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < kPix; ++k) walk_argmax(cand, p.row[k], c, z[(size_t)c * plane + (k < n ? k : 0)], best[k], idx[k]);
        if (a.fallback)
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < kPix; ++k) sum[k] = sum[k] + expf((z[(size_t)c * plane + (k < n ? k : 0)] - best[k]) * a.inv_T);
    }
    finish(a, s_cnt, base, n, vec, p.flags, idx, sum);
}
}  // namespace

extern "C" int mas_candidate_plbl(const float* z_q, int N, int C, int h, int w, int H, int W, const uint8_t* mask, const int64_t* spx,
                                  const int32_t* bits, int S, const int64_t* inner, int fallback, float th, float inv_T,
                                  const int64_t* targets, int num_classes, int64_t ignore_label, uint64_t* counts, uint8_t* labels,
                                  void* stream) {
    if (!z_q || !mask || !labels || (counts && !targets)) return MAS_ERR_NULL;
    const bool cand = spx || bits;
    if (cand ? (!spx || !bits || inner) : !inner) return MAS_ERR_NULL;      // exactly one of (spx, bits) and inner
    if (C < 1 || C > (cand ? 32 : 255)) return MAS_ERR_CLASSES;
    if (counts && (num_classes < 1 || num_classes > MAS_MAX_CLASSES)) return MAS_ERR_CLASSES;
    if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1 || N > 65535 || H > 65535 * kTH || (cand && S < 1)) return MAS_ERR_SHAPE;
    const bool ident = h == H && w == W;
    // what mas_naive_plbl / ops.naive_plbl_supported accept: the identity, or an upsampling at most x6 along the rows
    if (!ident && (h > H || w > W || (long long)W > 6LL * w || H > 65535)) return MAS_ERR_SHAPE;
    if (fallback && !(th >= 0.0f)) return MAS_ERR_RANGE;
    CandArgs a;
    a.z = z_q, a.mask = mask, a.out = labels;
    a.spx = reinterpret_cast<const long long*>(spx), a.bits = bits, a.inner = reinterpret_cast<const long long*>(inner);
    a.tgt = counts ? reinterpret_cast<const long long*>(targets) : nullptr;
    a.counts = reinterpret_cast<mas_u64*>(counts);
    a.ignore_label = (long long)ignore_label;
    a.C = C, a.h = h, a.w = w, a.H = H, a.W = W, a.S = cand ? S : 0, a.K = counts ? num_classes : 0;
    a.sh = (float)h / (float)H, a.sw = (float)w / (float)W, a.th = th, a.inv_T = inv_T;
    a.fallback = fallback ? 1 : 0;
    a.vec_ok = (W & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)mask & 3) == 0;
    const dim3 grid((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH), (unsigned)N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ident) {
        a.nrq = a.ncq = a.cb = 0;
        hipLaunchKernelGGL(k_candidate_plbl_identity, grid, dim3(kThreads), 0, st, a);
        return mas_launch_status();
    }
    // LDS extents: the exact maxima over tiles (same tap arithmetic as the kernel)
    int nrq, ncq;
    tile_footprint(a.sh, a.sw, h, w, H, W, kTH, kTW, &nrq, &ncq);
    int cb = (int)(kLdsBudget / (sizeof(float) * (size_t)nrq * ncq));     // >= 7: nrq <= kTH + 1, ncq <= kTW + 1
    cb = cb > C ? C : cb;
    a.nrq = nrq, a.ncq = ncq, a.cb = cb;
    hipLaunchKernelGGL(k_candidate_plbl, grid, dim3(kThreads), sizeof(float) * (size_t)cb * nrq * ncq, st, a);
    return mas_launch_status();
}
