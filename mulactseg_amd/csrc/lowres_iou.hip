// lowres_iou.hip -- the mIoU counters of the evaluation loop straight from the network's quarter-resolution logits.
//
// Reference: trainer/eval_naive.py:39-80 (= active_joint_multi_predignore.py:175-215): net(images) upsamples the logits x4 to the
// picture, then MeanIoU counts argmax(z[:, :-1]) and IoUIgnore counts argmax(z) against the labels.  mas_logits_iou_counts
// (metrics.hip) already fuses the two arg-maxes and the counters, but it reads the materialised full-resolution logits: 168 MB per
// 1024 x 2048 picture with 20 channels, written by the upsampling and read back.  Here each pixel's CH values exist in registers only.
//
// Arithmetic (normative; tests/lowres_iou_restated.py restates it in numpy).  The counters equal
// mas_logits_iou_counts(mas_upsample_bilinear_fwd(z_q, H, W), targets) in every element:
//   1. interpolation: the tap and the expression of k_upsample_fwd (upsample_tap.h), scale = (float)h / (float)H on the host; the
//      identity geometry (h == H, w == W) takes the logit itself.
//   2. two arg-maxes from one walk over the channels, the rule of k_logits_iou: o_cls starts at channel 0 and moves to channel c < C
//      only when y_c > best (strict: the first maximum wins; a NaN never moves it, a NaN in channel 0 keeps it at 0).  o_all is C
//      when CH = C + 1 and y_C > best, o_cls otherwise.
//   3. tally (iou_tally.h, shared with metrics.hip), with the "undefined" counters only when CH = C + 1.  Per-workgroup LDS u32
//      counters, one 64-bit global atomic per non-zero counter: integer sums, deterministic.
//
// Shape: that of k_naive_plbl (naive_plbl.hip).  A workgroup owns a 16 x 64 output tile, a thread 4 consecutive pixels of one row;
// the tile's quarter-resolution footprint (nrq x ncq, exact maxima over tiles from the host) is staged in LDS for `cb` channels at a
// time.  A thread's four int64 targets are loaded before the channel walk, so their latency hides behind it.
#include "common.h"
#include "iou_tally.h"
#include "upsample_tap.h"

namespace {
constexpr int kTH = 16, kTW = 64;          // output tile
constexpr int kThreads = 256;              // 16 lanes x 4 pixels per row, 16 rows
constexpr int kPix = 4;
constexpr size_t kLdsBudget = 32 * 1024;   // staged logits
constexpr int kMaxCnt = 3 * (MAS_MAX_CLASSES + 1);

struct IouArgs {
    const float* z;               // [B,CH,h,w]
    const long long* t;           // [B,H,W]
    mas_u64* counts;              // [3C+3]
    long long ignore_label;
    int CH, C, h, w, H, W;
    float sh, sw;
    int nrq, ncq, cb;             // LDS extents (quarter rows, quarter columns of one tile) and channels per staged block
    int vec_ok;                   // targets 16-byte aligned and W % 4 == 0: a thread's four targets are two 16-byte loads
};

__device__ __forceinline__ void load_targets(const IouArgs& a, size_t base, int n, bool vec, long long (&t)[kPix]) {
    if (vec) {
        const longlong2* p = reinterpret_cast<const longlong2*>(a.t + base);
        const longlong2 lo = p[0], hi = p[1];
        t[0] = lo.x, t[1] = lo.y, t[2] = hi.x, t[3] = hi.y;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) t[k] = k < n ? a.t[base + k] : 0;
    }
}

// channel c of the walk: c < C updates (best, idx) as k_logits_iou does; c == C (CH = C + 1) decides o_all
__device__ __forceinline__ void walk(float v, int c, int C, float& best, int& idx, bool& all_is_c) {
    if (c == 0) {
        best = v;
    } else if (c < C) {
        if (v > best) {
            best = v;
            idx = c;
        }
    } else {
        all_is_c = v > best;
    }
}

__device__ __forceinline__ void clear_counts(unsigned* s_cnt, int n) {
    for (int i = threadIdx.x; i < n; i += kThreads) s_cnt[i] = 0;
}

__device__ __forceinline__ void finish(const IouArgs& a, unsigned* s_cnt, int n, const long long (&t)[kPix], const int (&idx)[kPix],
                                       const bool (&all_is_c)[kPix]) {
    const bool with_ignore = a.CH > a.C;
    for (int k = 0; k < n; ++k) tally(s_cnt, a.C, t[k], idx[k], all_is_c[k] ? a.C : idx[k], a.ignore_label, with_ignore);
    __syncthreads();
    const int ncnt = 3 * a.C + 3;
    for (int i = threadIdx.x; i < ncnt; i += kThreads)
        if (s_cnt[i]) atomicAdd(&a.counts[i], (mas_u64)s_cnt[i]);
}

// grid: (ceil(W / kTW), ceil(H / kTH), B); dynamic LDS: cb * nrq * ncq floats
__global__ __launch_bounds__(kThreads) void k_lowres_iou(const IouArgs a) {
    extern __shared__ float lds[];
    __shared__ unsigned s_cnt[kMaxCnt];
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, CH = a.CH, C = a.C, h = a.h, w = a.w;
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    const int y1 = min(y0 + kTH, H) - 1, x1 = min(x0 + kTW, W) - 1;
    const int py = y0 + tid / (kTW / kPix), px0 = x0 + (tid % (kTW / kPix)) * kPix;
    const bool live = py < H && px0 < W;
    const int n = live ? min(kPix, W - px0) : 0;
    const int cy = min(py, y1);
    const int q_lo = make_tap(a.sh, y0, h).i0, q_hi = make_tap(a.sh, y1, h).i1;
    const int c_lo = make_tap(a.sw, x0, w).i0, c_hi = make_tap(a.sw, x1, w).i1;
    const int nq = q_hi - q_lo + 1, nc = c_hi - c_lo + 1;
    const size_t base = (size_t)blockIdx.z * ((size_t)H * W) + (size_t)cy * W + (live ? px0 : 0);
    if (nq > a.nrq || nc > a.ncq) return;             // (uniform over the workgroup; the host sized the extents -- never taken)
    long long t[kPix];
    load_targets(a, base, n, n == kPix && a.vec_ok, t);
    clear_counts(s_cnt, 3 * C + 3);                   // (the first staging barrier orders it before any tally)
    const Tap ty = make_tap(a.sh, cy, h);
    const int r0 = (ty.i0 - q_lo) * a.ncq, r1 = (ty.i1 - q_lo) * a.ncq;
    Tap tx[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) tx[k] = make_tap(a.sw, min(px0 + k, x1), w);
    const size_t qplane = (size_t)h * w;
    const float* zq = a.z + (size_t)blockIdx.z * CH * qplane;
    const int tile = a.nrq * a.ncq;
    float best[kPix];
    int idx[kPix];
    bool all_is_c[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) best[k] = 0.0f, idx[k] = 0, all_is_c[k] = false;
    for (int c0 = 0; c0 < CH; c0 += a.cb) {
        const int nb = min(a.cb, CH - c0);
        __syncthreads();                              // (the previous block's reads are done)
        for (int i = tid; i < nb * nq * nc; i += kThreads) {
            const int cc = i / (nq * nc), rem = i - cc * (nq * nc), r = rem / nc, col = rem - r * nc;
            lds[cc * tile + r * a.ncq + col] = zq[(size_t)(c0 + cc) * qplane + (size_t)(q_lo + r) * w + c_lo + col];
        }
        __syncthreads();
        for (int cc = 0; cc < nb; ++cc) {
            const float* q = lds + cc * tile;
            const int c = c0 + cc;
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                const int i0 = tx[k].i0 - c_lo, i1 = tx[k].i1 - c_lo;
                const float v = ty.l0 * (tx[k].l0 * q[r0 + i0] + tx[k].l1 * q[r0 + i1]) +
                                ty.l1 * (tx[k].l0 * q[r1 + i0] + tx[k].l1 * q[r1 + i1]);
                walk(v, c, C, best[k], idx[k], all_is_c[k]);
            }
        }
    }
    finish(a, s_cnt, n, t, idx, all_is_c);
}

// identity geometry (h == H, w == W): the logits themselves, read in place
__global__ __launch_bounds__(kThreads) void k_lowres_iou_identity(const IouArgs a) {
    __shared__ unsigned s_cnt[kMaxCnt];
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, CH = a.CH, C = a.C;
    const int py = blockIdx.y * kTH + tid / (kTW / kPix), px0 = blockIdx.x * kTW + (tid % (kTW / kPix)) * kPix;
    const bool live = py < H && px0 < W;
    const int n = live ? min(kPix, W - px0) : 0;
    const size_t plane = (size_t)H * W, pix = live ? (size_t)py * W + px0 : 0, base = (size_t)blockIdx.z * plane + pix;
    long long t[kPix];
    load_targets(a, base, n, n == kPix && a.vec_ok, t);
    clear_counts(s_cnt, 3 * C + 3);
    __syncthreads();
    const float* z = a.z + (size_t)blockIdx.z * CH * plane + pix;
    float best[kPix];
    int idx[kPix];
    bool all_is_c[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) best[k] = 0.0f, idx[k] = 0, all_is_c[k] = false;
    if (live)
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int k = 0; k < kPix; ++k) walk(z[(size_t)c * plane + (k < n ? k : 0)], c, C, best[k], idx[k], all_is_c[k]);
    finish(a, s_cnt, n, t, idx, all_is_c);
}
}  // namespace

extern "C" int mas_lowres_iou_counts(const float* z_q, const int64_t* targets, int B, int channels, int h, int w, int H, int W,
                                     int num_classes, int64_t ignore_label, uint64_t* counts, void* stream) {
    if (!z_q || !targets || !counts) return MAS_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || (long long)H * W > 0x7fffffffLL / 2) return MAS_ERR_SHAPE;
    if (num_classes < 1 || num_classes > MAS_MAX_CLASSES || (channels != num_classes && channels != num_classes + 1))
        return MAS_ERR_CLASSES;
    if (B > 65535 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    const bool ident = h == H && w == W;
    // what mas_naive_plbl / ops.naive_plbl_supported accept: the identity, or an upsampling at most x6 along the rows
    if (!ident && (h > H || w > W || (long long)W > 6LL * w || H > 65535)) return MAS_ERR_SHAPE;
    IouArgs a;
    a.z = z_q, a.t = reinterpret_cast<const long long*>(targets), a.counts = reinterpret_cast<mas_u64*>(counts);
    a.ignore_label = (long long)ignore_label;
    a.CH = channels, a.C = num_classes, a.h = h, a.w = w, a.H = H, a.W = W;
    a.sh = (float)h / (float)H, a.sw = (float)w / (float)W;
    a.vec_ok = (W & 3) == 0 && ((uintptr_t)targets & 15) == 0;
    const dim3 grid((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH), (unsigned)B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ident) {
        a.nrq = a.ncq = a.cb = 0;
        hipLaunchKernelGGL(k_lowres_iou_identity, grid, dim3(kThreads), 0, st, a);
        return mas_launch_status();
    }
    int nrq, ncq;
    tile_footprint(a.sh, a.sw, h, w, H, W, kTH, kTW, &nrq, &ncq);
    int cb = (int)(kLdsBudget / (sizeof(float) * (size_t)nrq * ncq));     // >= 7: nrq <= kTH + 1, ncq <= kTW + 1
    cb = cb > channels ? channels : cb;
    a.nrq = nrq, a.ncq = ncq, a.cb = cb;
    hipLaunchKernelGGL(k_lowres_iou, grid, dim3(kThreads), sizeof(float) * (size_t)cb * nrq * ncq, st, a);
    return mas_launch_status();
}
