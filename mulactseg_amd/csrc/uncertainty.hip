// uncertainty.hip -- the acquisition scan for the measures beyond BvSB: margin, least confidence, entropy (and BvSB itself, the
// yardstick against the headline scan).
//
// The round's tail is measure-agnostic: per (region, arg-max class) it wants the fixed-point sum of an UNWEIGHTED per-pixel value,
// the arg-max-class histogram and the per-picture class-probability sums (single_pass.hip's accumulators); class weights, the ban,
// normalisation and the budget walk come afterwards.  k_uncertainty fills the same three accumulators with the value uncertainty.h
// defines -- one header, used by the kernel and by the host loop at the end of this file, so the two agree bit for bit.
//
// Shape: a workgroup owns a 256 x 16 pixel tile; a lane owns one COLUMN of it and walks down the 16 rows.  Every load of a wave is
// 256 contiguous bytes of one class plane (any W, any alignment), and a lane's consecutive pixels mostly stay inside one superpixel
// with one arg-max class: equal (id, class) keys are merged in registers and leave as one u64 + one u32 global atomic per run.  The
// class-prior quanta stay in per-thread u32 registers (16 pixels; mas_probq is exact over 511) and leave through a wave shuffle, LDS
// and one atomic per class and workgroup.  All sums are integers: the result does not depend on the order.
//
// LOWRES: z is the model's quarter-resolution tensor [B,C,h,w]; each pixel's C logits are its bilinear upsampling evaluated in
// registers with the tap of upsample_tap.h and the expression of k_upsample_fwd, so they equal mas_upsample_bilinear_fwd's output bit
// for bit -- the [B,C,H,W] tensor is never written.  The four taps are read through the vector cache (a wave's 64 columns touch ~17
// consecutive floats of two rows).
//
// Measured (profiles/uncertainty/README.md; [4,20,256,512] -> 1024 x 2048, 2048 superpixels): 268-270 us per batch for every measure,
// 1.07x k_single_pass<LOWRES> in the same trace.  The atomics of the probe's random logits (3.4 M key runs) are ~54 us of it, the tap
// reads ~20 us; ~0.2 ms do not depend on C and are not attributed by a counter yet.
#include "common.h"
#include "uncertainty.h"
#include "upsample_tap.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = kThreads;      // one column per lane
constexpr int kTileH = 16;            // rows a lane walks: 16 quanta per u32 accumulator

struct UncArgs {
    const float* z;          // [B,C,H,W], or [B,C,h,w] (LOWRES)
    const void* spx;         // [B,H,W] of spx_dtype
    int spx_dtype;
    int C, H, W, S;
    int h, w;                // LOWRES
    float sh, sw;            // LOWRES: (float)h / (float)H, (float)w / (float)W
    float invT, inv_log_c;
    int measure;
    int tiles_x, tiles_y;
    mas_u64* prob_sum;       // [B,C]
    mas_u64* class_sum;      // [B,S,C]
    unsigned* hist;          // [B,S,C]
};

__device__ __forceinline__ int load_id(const void* spx, int dtype, size_t i) {
    if (dtype == MAS_ID_I64) {
        const long long v = static_cast<const long long*>(spx)[i];
        return (v < 0 || v > 0x7fffffffLL) ? -1 : (int)v;
    }
    if (dtype == MAS_ID_I32) return static_cast<const int*>(spx)[i];
    return (int)static_cast<const unsigned short*>(spx)[i];
}

template <int CT, bool EXACT, bool LOWRES>
__global__ __launch_bounds__(kThreads) void k_uncertainty(const UncArgs a) {
    __shared__ mas_u64 s_part[kThreads / MAS_WAVE][CT];
    const int C = EXACT ? CT : a.C;
    const int H = a.H, W = a.W, S = a.S;
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x; bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int b = bid / a.tiles_y;
    const size_t HW = (size_t)H * W;
    const size_t plane = LOWRES ? (size_t)a.h * a.w : HW;
    const float* zb = a.z + (size_t)b * C * plane;
    mas_u64* gsum = a.class_sum + (size_t)b * S * C;
    unsigned* ghist = a.hist + (size_t)b * S * C;
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    const int wave = threadIdx.x / MAS_WAVE;
    const int px = tx * kTileW + (int)threadIdx.x;
    const bool live = px < W;
    Tap tcol = {0, 0, 0.f, 0.f};
    if (LOWRES) tcol = make_tap(a.sw, live ? px : W - 1, a.w);

    unsigned acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0;
    int run_key = -1;            // (id * MAS_MAX_CLASSES + class) of the open run, -1: none
    mas_u64 run_q = 0;
    unsigned run_n = 0;
    auto flush = [&]() {
        if (run_key >= 0) {
            const size_t g = (size_t)(run_key / MAS_MAX_CLASSES) * C + (run_key % MAS_MAX_CLASSES);
            atomicAdd(&gsum[g], run_q);
            atomicAdd(&ghist[g], run_n);
        }
    };

    if (live) {
        const int y_end = min(ty * kTileH + kTileH, H);
#pragma unroll 1
        for (int y = ty * kTileH; y < y_end; ++y) {
            const size_t pix = (size_t)y * W + px;
            int id = load_id(a.spx, a.spx_dtype, (size_t)b * HW + pix);
            if (id >= S) id = -1;
            float x[CT];
            if (LOWRES) {
                const Tap trow = make_tap(a.sh, y, a.h);
                const float* r0 = zb + (size_t)trow.i0 * a.w;
                const float* r1 = zb + (size_t)trow.i1 * a.w;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    if (EXACT || c < C) {
                        const float* q0 = r0 + (size_t)c * plane;
                        const float* q1 = r1 + (size_t)c * plane;
                        x[c] = trow.l0 * (tcol.l0 * q0[tcol.i0] + tcol.l1 * q0[tcol.i1]) +
                               trow.l1 * (tcol.l0 * q1[tcol.i0] + tcol.l1 * q1[tcol.i1]);
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (EXACT || c < C) x[c] = __builtin_nontemporal_load(zb + (size_t)c * plane + pix);
            }
            int arg;
            float R;
            const float u = mas_uncertainty_pixel(x, CT, C, a.invT, a.measure, a.inv_log_c, &arg, &R);
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (EXACT || c < C) acc[c] += mas_probq(x[c], R);
            const int key = id < 0 ? -1 : id * MAS_MAX_CLASSES + arg;
            if (key != run_key) {
                flush();
                run_key = key;
                run_q = 0;
                run_n = 0;
            }
            run_q += mas_uncertainty_quantum(u);
            run_n += 1;
        }
        flush();
    }

    // class sums: wave shuffle reduction, 4 waves through LDS, one atomic per class per workgroup
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        mas_u64 s = acc[c];
#pragma unroll
        for (int off = MAS_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, MAS_WAVE);
        if (lane == 0) s_part[wave][c] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        mas_u64 s = 0;
#pragma unroll
        for (int k = 0; k < kThreads / MAS_WAVE; ++k) s += s_part[k][threadIdx.x];
        if (s) atomicAdd(&a.prob_sum[(size_t)b * C + threadIdx.x], s);
    }
}

template <int CT, bool EXACT>
int launch(const UncArgs& a, int B, bool lowres, hipStream_t st) {
    const long long nblk = (long long)B * a.tiles_x * a.tiles_y;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return MAS_ERR_SHAPE;
    if (lowres)
        hipLaunchKernelGGL((k_uncertainty<CT, EXACT, true>), dim3((unsigned)nblk), dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL((k_uncertainty<CT, EXACT, false>), dim3((unsigned)nblk), dim3(kThreads), 0, st, a);
    return mas_launch_status();
}

int check_common(const void* z, const void* spx, int spx_dtype, int B, int C, int H, int W, int S, int measure, const void* prob_sum,
                 const void* class_sum, const void* hist) {
    if (!z || !spx || !prob_sum || !class_sum || !hist) return MAS_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || S <= 0 || (long long)H * W > (1LL << 23)) return MAS_ERR_SHAPE;
    if (S > 0x7fffffff / MAS_MAX_CLASSES) return MAS_ERR_SHAPE;          // the run key id * MAS_MAX_CLASSES + class is an int
    if (C < 2 || C > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    if (spx_dtype != MAS_ID_I64 && spx_dtype != MAS_ID_I32 && spx_dtype != MAS_ID_U16) return MAS_ERR_DTYPE;
    if (measure < 0 || measure >= MAS_UNC_MEASURES) return MAS_ERR_RANGE;
    return 0;
}

int run(UncArgs a, int B, bool lowres, hipStream_t st) {
    a.inv_log_c = mas_uncertainty_inv_log_classes(a.C);
    a.tiles_x = (a.W + kTileW - 1) / kTileW;
    a.tiles_y = (a.H + kTileH - 1) / kTileH;
    // the Cityscapes / VOC channel counts get loops without guards; every other C runs the guarded 32-slot instantiation (measured per
    // low-resolution pool batch: C = 2 0.20 ms, C = 8 0.27 ms, C = 32 0.60 ms against 0.28 ms at C = 20 -- no smaller bucket: a small
    // C pays at most the ~0.2 ms that do not depend on C)
    switch (a.C) {
        case 19: return launch<19, true>(a, B, lowres, st);
        case 20: return launch<20, true>(a, B, lowres, st);
        case 21: return launch<21, true>(a, B, lowres, st);
        default: return launch<MAS_MAX_CLASSES, false>(a, B, lowres, st);
    }
}

}  // namespace

extern "C" int mas_uncertainty_accum(const float* z, const void* spx, int spx_dtype, int B, int C, int H, int W, int S, float invT,
                                     int measure, uint64_t* prob_sum, uint64_t* class_sum, uint32_t* hist, void* stream) {
    if (int e = check_common(z, spx, spx_dtype, B, C, H, W, S, measure, prob_sum, class_sum, hist)) return e;
    UncArgs a = {};
    a.z = z, a.spx = spx, a.spx_dtype = spx_dtype;
    a.C = C, a.H = H, a.W = W, a.S = S, a.invT = invT, a.measure = measure;
    a.prob_sum = reinterpret_cast<mas_u64*>(prob_sum), a.class_sum = reinterpret_cast<mas_u64*>(class_sum), a.hist = hist;
    return run(a, B, false, static_cast<hipStream_t>(stream));
}

extern "C" int mas_uncertainty_accum_lowres(const float* zq, int h, int w, const void* spx, int spx_dtype, int B, int C, int H, int W,
                                            int S, float invT, int measure, uint64_t* prob_sum, uint64_t* class_sum, uint32_t* hist,
                                            void* stream) {
    if (int e = check_common(zq, spx, spx_dtype, B, C, H, W, S, measure, prob_sum, class_sum, hist)) return e;
    if (h <= 0 || w <= 0) return MAS_ERR_SHAPE;
    if (h == H && w == W)           // the identity: the logits themselves
        return mas_uncertainty_accum(zq, spx, spx_dtype, B, C, H, W, S, invT, measure, prob_sum, class_sum, hist, stream);
    // the ratios of mas_naive_plbl / mas_candidate_plbl (what mas_upsample_bilinear_fwd can materialise): an upsampling, at most x6
    // along the rows.  Refused before anything is launched.
    if (h > H || w > W || (long long)W > 6LL * w || H > 65535) return MAS_ERR_RANGE;
    UncArgs a = {};
    a.z = zq, a.spx = spx, a.spx_dtype = spx_dtype;
    a.C = C, a.H = H, a.W = W, a.S = S, a.invT = invT, a.measure = measure;
    a.h = h, a.w = w, a.sh = (float)h / (float)H, a.sw = (float)w / (float)W;
    a.prob_sum = reinterpret_cast<mas_u64*>(prob_sum), a.class_sum = reinterpret_cast<mas_u64*>(class_sum), a.hist = hist;
    return run(a, B, true, static_cast<hipStream_t>(stream));
}

// The CPU-side statement of the spec: host pointers, a plain loop over the pixels through uncertainty.h.  No device is touched.
extern "C" int mas_uncertainty_reference(const float* z, const void* spx, int spx_dtype, int B, int C, int H, int W, int S, float invT,
                                         int measure, uint64_t* prob_sum, uint64_t* class_sum, uint32_t* hist) {
    if (int e = check_common(z, spx, spx_dtype, B, C, H, W, S, measure, prob_sum, class_sum, hist)) return e;
    const float inv_log_c = mas_uncertainty_inv_log_classes(C);
    const size_t HW = (size_t)H * W;
    for (int b = 0; b < B; ++b) {
        for (size_t p = 0; p < HW; ++p) {
            float x[MAS_MAX_CLASSES];
            for (int c = 0; c < C; ++c) x[c] = z[((size_t)b * C + c) * HW + p];
            int arg;
            float R;
            const float u = mas_uncertainty_pixel(x, C, C, invT, measure, inv_log_c, &arg, &R);
            for (int c = 0; c < C; ++c) prob_sum[(size_t)b * C + c] += mas_probq(x[c], R);
            long long id;
            const size_t i = (size_t)b * HW + p;
            if (spx_dtype == MAS_ID_I64) id = static_cast<const long long*>(spx)[i];
            else if (spx_dtype == MAS_ID_I32) id = static_cast<const int*>(spx)[i];
            else id = static_cast<const unsigned short*>(spx)[i];
            if (id < 0 || id >= S) continue;
            const size_t g = ((size_t)b * S + (size_t)id) * C + arg;
            class_sum[g] += mas_uncertainty_quantum(u);
            hist[g] += 1;
        }
    }
    return 0;
}
