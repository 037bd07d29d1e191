// naive_plbl.hip -- naive top-1 pseudo labels of the stage-2 ablation without prototypes, straight from quarter-resolution logits.
//
// Reference: trainer/eval_save_naiveplbl.py:46-61.  feat_forward's logits are upsampled x4 to the picture (F.interpolate bilinear,
// align_corners=False), then label = argmax over the C channels; pixels outside the mask get 255; with plbl_th > 0 the mask is
// softmax(logits).max(1) > plbl_th over every pixel instead.  Materialised, the full-resolution logits are 168 MB per 1024 x 2048
// picture; here each pixel's C values exist in registers only, one at a time.
//
// Arithmetic (normative; tests/naive_plbl_restated.py restates it in numpy):
//   1. interpolation: the tap and the expression of k_upsample_fwd (upsample.hip), scale = (float)h / (float)H on the host,
//        y = l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11)
//      so every value equals mas_upsample_bilinear_fwd's output bit for bit.  Identity geometry (h == H, w == W): the logit itself.
//   2. argmax: channel order, strict '>' (the first maximum wins, as torch.max); a NaN takes the place and keeps it (the first NaN
//      wins, as torch.max).
//   3. threshold (th > 0): p_max = 1 / sum_c expf(y_c - y_max), channel order, sum starts from 0; label kept iff p_max > th.  Not
//      bit-equal to torch.softmax (another exp and another summation order); a NaN logit gives p_max NaN, i.e. 255.
//
// Shape: a workgroup owns a 16 x 64 output tile, a thread 4 consecutive pixels of one row (one 32-bit mask load and label store).
// The tile's quarter-resolution footprint (nrq x ncq, exact maxima over tiles computed on the host with the same tap arithmetic) is
// staged in LDS for `cb` channels at a time, channel blocks in order; the threshold pass walks the blocks a second time.
#include "common.h"
#include "upsample_tap.h"

namespace {
constexpr int kTH = 16, kTW = 64;          // output tile
constexpr int kThreads = 256;              // 16 lanes x 4 pixels per row, 16 rows
constexpr int kPix = 4;
constexpr size_t kLdsBudget = 32 * 1024;

struct PlblArgs {
    const float* z;               // [N,C,h,w]
    const unsigned char* mask;    // [N,H,W] or NULL (threshold mode)
    unsigned char* out;           // [N,H,W]
    int C, h, w, H, W;
    float sh, sw, th;
    int nrq, ncq, cb;             // LDS extents (quarter rows, quarter columns of one tile) and channels per staged block
    int vec_ok;                   // mask and labels are 4-byte aligned and W % 4 == 0: 32-bit mask loads and label stores
};

__device__ __forceinline__ void store4(unsigned char* dst, const unsigned char (&v)[kPix], int n, bool vec) {
    if (vec) {
        *reinterpret_cast<unsigned*>(dst) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
    } else {
        for (int k = 0; k < n; ++k) dst[k] = v[k];
    }
}

__device__ __forceinline__ void finish(const PlblArgs& a, size_t base, int n, bool vec, const int (&idx)[kPix], const float (&sum)[kPix],
                                       bool thr) {
    unsigned char keep[kPix] = {0, 0, 0, 0};
    if (thr) {
#pragma unroll
        for (int k = 0; k < kPix; ++k) keep[k] = (1.0f / sum[k]) > a.th;
    } else if (vec) {
        const unsigned m = *reinterpret_cast<const unsigned*>(a.mask + base);
#pragma unroll
        for (int k = 0; k < kPix; ++k) keep[k] = (m >> (8 * k)) & 0xff;
    } else {
        for (int k = 0; k < n; ++k) keep[k] = a.mask[base + k];
    }
    unsigned char v[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) v[k] = keep[k] ? (unsigned char)idx[k] : (unsigned char)255;
    store4(a.out + base, v, n, vec);
}

// grid: (ceil(W / kTW), ceil(H / kTH), N); dynamic LDS: cb * nrq * ncq floats
__global__ __launch_bounds__(kThreads) void k_naive_plbl(const PlblArgs a) {
    extern __shared__ float lds[];
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
        if (live) {
            const unsigned char v[kPix] = {255, 255, 255, 255};
            store4(a.out + base, v, n, false);
        }
        return;
    }
    const Tap ty = make_tap(a.sh, cy, h);
    const int r0 = (ty.i0 - q_lo) * a.ncq, r1 = (ty.i1 - q_lo) * a.ncq;
    Tap tx[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) tx[k] = make_tap(a.sw, min(px0 + k, x1), w);
    const size_t qplane = (size_t)h * w;
    const float* zq = a.z + (size_t)blockIdx.z * C * qplane;
    const int tile = a.nrq * a.ncq;
    const bool thr = a.mask == nullptr;
    float best[kPix], sum[kPix];
    int idx[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) best[k] = 0.0f, sum[k] = 0.0f, idx[k] = 0;
    for (int pass = 0; pass < (thr ? 2 : 1); ++pass) {
        for (int c0 = 0; c0 < C; c0 += a.cb) {
            const int nb = min(a.cb, C - c0);
            __syncthreads();                          // (the previous block's reads are done)
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
                    if (pass == 0) {
                        if (c == 0) best[k] = v;
                        else arg_update(v, c, best[k], idx[k]);
                    } else {
                        sum[k] = sum[k] + expf(v - best[k]);
                    }
                }
            }
        }
    }
    if (live) finish(a, base, n, vec, idx, sum, thr);
}

// identity geometry (h == H, w == W): the logits themselves, read in place
__global__ __launch_bounds__(kThreads) void k_naive_plbl_identity(const PlblArgs a) {
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, C = a.C;
    const int py = blockIdx.y * kTH + tid / (kTW / kPix), px0 = blockIdx.x * kTW + (tid % (kTW / kPix)) * kPix;
    if (py >= H || px0 >= W) return;
    const int n = min(kPix, W - px0);
    const size_t plane = (size_t)H * W, pix = (size_t)py * W + px0, base = (size_t)blockIdx.z * plane + pix;
    const bool vec = n == kPix && a.vec_ok;
    const float* z = a.z + (size_t)blockIdx.z * C * plane + pix;
    const bool thr = a.mask == nullptr;
    float best[kPix], sum[kPix];
    int idx[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) best[k] = z[k < n ? k : 0], sum[k] = 0.0f, idx[k] = 0;
    for (int c = 1; c < C; ++c)
#pragma unroll
        for (int k = 0; k < kPix; ++k) arg_update(z[(size_t)c * plane + (k < n ? k : 0)], c, best[k], idx[k]);
    if (thr)
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < kPix; ++k) sum[k] = sum[k] + expf(z[(size_t)c * plane + (k < n ? k : 0)] - best[k]);
    finish(a, base, n, vec, idx, sum, thr);
}
}  // namespace

extern "C" int mas_naive_plbl(const float* logits_q, int N, int C, int h, int w, int H, int W, const uint8_t* mask, float th,
                              uint8_t* labels, void* stream) {
    if (!logits_q || !labels) return MAS_ERR_NULL;
    const bool thr = th > 0.0f;
    if (!thr && !mask) return MAS_ERR_NULL;
    if (C < 1 || C > 255) return MAS_ERR_CLASSES;
    if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1 || N > 65535 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    const bool ident = h == H && w == W;
    // what mas_upsample_bilinear_fwd / ops.upsample_bilinear_supported accept: an upsampling, at most x6 along the rows
    if (!ident && (h > H || w > W || (long long)W > 6LL * w || H > 65535)) return MAS_ERR_SHAPE;
    PlblArgs a;
    a.z = logits_q, a.mask = thr ? nullptr : mask, a.out = labels;
    a.C = C, a.h = h, a.w = w, a.H = H, a.W = W;
    a.sh = (float)h / (float)H, a.sw = (float)w / (float)W, a.th = th;
    a.vec_ok = (W & 3) == 0 && ((uintptr_t)labels & 3) == 0 && (thr || ((uintptr_t)mask & 3) == 0);
    const dim3 grid((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH), (unsigned)N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ident) {
        a.nrq = a.ncq = a.cb = 0;
        hipLaunchKernelGGL(k_naive_plbl_identity, grid, dim3(kThreads), 0, st, a);
        return mas_launch_status();
    }
    // LDS extents: the exact maxima over tiles (same tap arithmetic as the kernel)
    int nrq, ncq;
    tile_footprint(a.sh, a.sw, h, w, H, W, kTH, kTW, &nrq, &ncq);
    int cb = (int)(kLdsBudget / (sizeof(float) * (size_t)nrq * ncq));     // >= 7: nrq <= kTH + 1, ncq <= kTW + 1
    cb = cb > C ? C : cb;
    a.nrq = nrq, a.ncq = ncq, a.cb = cb;
    hipLaunchKernelGGL(k_naive_plbl, grid, dim3(kThreads), sizeof(float) * (size_t)cb * nrq * ncq, st, a);
    return mas_launch_status();
}
