// photometric.hip -- colour jitter and grayscale on the device, for the samples that draw them (reference
// dataloader/transform.py:139-153: ExtColorJitter(0.4, 0.4, 0.4, 0.1, p=0.2) + ExtRandomGrayscale(p=0.2) after crop and flip).  A
// sample that draws neither takes the single mas_train_augment launch; a sample that draws either takes two passes here:
//
//   pass 1  k_train_augment_u8: the geometry of augment_pixel.h, once; the crop is written as u8 HWC (1.8 MB at 768 x 768) and the
//           maps exactly as k_train_augment writes them.  When contrast is in the chain, the ops that precede it in this sample's
//           order are applied to the pixel in registers and its L joins ONE u32 accumulator (wave shuffle, LDS, one atomic per
//           workgroup; an integer sum, so the order does not matter; u32 holds 255 * 16.8 M pixels).
//   pass 2  k_photometric: reads the u8 crop, forms the contrast mean from the accumulator on the device (no host read, no
//           synchronisation), applies the whole chain in the drawn order, grayscale and the normalisation, writes f32 CHW.  Four
//           pixels per thread: three dword loads, and one 16-byte store per plane when the plane size is a multiple of four.
//
// The arithmetic is photometric.h's, used by both kernels and by the host loop mas_photometric_reference at the end of this file.
//
// Measured (profiles/photometric/README.md; 1024 x 2048 -> 768 x 768): pass 1 35.0 us, pass 2 13.2 us, against 12.5 us for k_train_augment
// in the same trace.  22 us of pass 1 are the sum (pass 1 without it: 11.0 us): 2 304 workgroups add to one word.
#include "common.h"
#include "augment_pixel.h"
#include "photometric.h"

namespace {
constexpr int kThreads = 256;
constexpr int kPix = 4;          // pixels per thread of pass 2

__global__ __launch_bounds__(kThreads) void k_train_augment_u8(const AugGeom q, const mas_pm_chain c, int cpos,
                                                                unsigned char* __restrict__ out, unsigned* __restrict__ lsum) {
    __shared__ unsigned s_part[kThreads / MAS_WAVE];
    const int o = blockIdx.x * kThreads + threadIdx.x;
    unsigned l = 0;
    if (o < q.oh * q.ow) {
        int r, g, b;
        augment_pixel(q, o, r, g, b);
        unsigned char* px = out + (size_t)o * 3;
        px[0] = (unsigned char)r; px[1] = (unsigned char)g; px[2] = (unsigned char)b;
        if (lsum) {
            mas_pm_apply(&c, 0, cpos, 0, &r, &g, &b);          // (no contrast among them: the mean is not read)
            l = (unsigned)mas_pm_grey(r, g, b);
        }
    }
    if (!lsum) return;          // uniform over the grid
#pragma unroll
    for (int off = MAS_WAVE / 2; off > 0; off >>= 1) l += __shfl_down(l, off, MAS_WAVE);
    if ((threadIdx.x & (MAS_WAVE - 1)) == 0) s_part[threadIdx.x / MAS_WAVE] = l;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
#pragma unroll
        for (int k = 0; k < kThreads / MAS_WAVE; ++k) s += s_part[k];
        atomicAdd(lsum, s);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_photometric(const unsigned char* __restrict__ crop, int n, const mas_pm_chain c,
                                                           const unsigned* __restrict__ lsum, float m0, float m1, float m2, float s0,
                                                           float s1, float s2, float* __restrict__ out, unsigned char* __restrict__ out_u8) {
    const int o = (blockIdx.x * kThreads + threadIdx.x) * kPix;
    if (o >= n) return;
    const int cmean = lsum ? mas_pm_contrast_mean(*lsum, (unsigned long long)n) : 0;
    const int cnt = min(kPix, n - o);
    unsigned char px[3 * kPix];
    if (cnt == kPix) {          // 12 bytes at a multiple of 12: three aligned dwords
        const unsigned* w = reinterpret_cast<const unsigned*>(crop + (size_t)o * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned v = w[k];
            px[4 * k] = v & 0xFF; px[4 * k + 1] = (v >> 8) & 0xFF; px[4 * k + 2] = (v >> 16) & 0xFF; px[4 * k + 3] = v >> 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * kPix; ++k) px[k] = k < 3 * cnt ? crop[(size_t)o * 3 + k] : 0;
    }
    float fr[kPix], fg[kPix], fb[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        int r = px[3 * k], g = px[3 * k + 1], b = px[3 * k + 2];
        mas_pm_pixel(&c, cmean, &r, &g, &b);
        px[3 * k] = (unsigned char)r; px[3 * k + 1] = (unsigned char)g; px[3 * k + 2] = (unsigned char)b;
        fr[k] = mas_pm_normalise(r, m0, s0);
        fg[k] = mas_pm_normalise(g, m1, s1);
        fb[k] = mas_pm_normalise(b, m2, s2);
    }
    const size_t plane = (size_t)n;
    if (VEC) {          // n % 4 == 0: every plane offset is 16-byte aligned and every thread holds four pixels
        *reinterpret_cast<float4*>(out + o) = make_float4(fr[0], fr[1], fr[2], fr[3]);
        *reinterpret_cast<float4*>(out + plane + o) = make_float4(fg[0], fg[1], fg[2], fg[3]);
        *reinterpret_cast<float4*>(out + 2 * plane + o) = make_float4(fb[0], fb[1], fb[2], fb[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            if (k < cnt) {
                out[o + k] = fr[k];
                out[plane + o + k] = fg[k];
                out[2 * plane + o + k] = fb[k];
            }
        }
    }
    if (out_u8) {
#pragma unroll
        for (int k = 0; k < 3 * kPix; ++k)
            if (k < 3 * cnt) out_u8[(size_t)o * 3 + k] = px[k];
    }
}

// order: a permutation of 0..3; factors of the ops present; -> the chain, or an error code
int make_chain(const int* order, const float* factor, int present, int grey, mas_pm_chain* c) {
    if (present & ~((1 << MAS_PM_OPS) - 1)) return MAS_ERR_RANGE;
    if (present && (!order || !factor)) return MAS_ERR_NULL;
    int seen = 0;
    for (int k = 0; k < MAS_PM_OPS; ++k) {
        c->order[k] = order ? order[k] : k;
        c->factor[k] = (factor && ((present >> k) & 1)) ? factor[k] : 1.0f;
        if (c->order[k] < 0 || c->order[k] >= MAS_PM_OPS) return MAS_ERR_RANGE;
        seen |= 1 << c->order[k];
    }
    if (seen != (1 << MAS_PM_OPS) - 1) return MAS_ERR_RANGE;
    for (int k = 0; k < MAS_PM_HUE; ++k)          // ColorJitter's ranges start at max(0, 1 - x): no negative factor; NaN is refused too
        if (((present >> k) & 1) && !(c->factor[k] >= 0.0f)) return MAS_ERR_RANGE;
    if (((present >> MAS_PM_HUE) & 1) && !(c->factor[MAS_PM_HUE] >= -0.5f && c->factor[MAS_PM_HUE] <= 0.5f)) return MAS_ERR_RANGE;
    c->present = present;
    c->shift = ((present >> MAS_PM_HUE) & 1) ? mas_pm_hue_shift(c->factor[MAS_PM_HUE]) : 0;
    c->grey = grey ? 1 : 0;
    return 0;
}
}  // namespace

extern "C" int mas_train_augment_u8(const uint8_t* img, int H, int W, int th, int tw, const int32_t* hbounds, const int32_t* hk, int hks,
                                    const int32_t* vbounds, const int32_t* vk, int vks, const int32_t* xidx, const int32_t* yidx,
                                    int gap_y, int gap_x, int crop_i, int crop_j, int flip, int out_h, int out_w, const uint8_t* fill,
                                    const void* map0, int map0_dtype, int64_t pad0, void* out_map0, int out0_u8, const void* map1,
                                    int map1_dtype, int64_t pad1, void* out_map1, int out1_u8, const int32_t* order, const float* factor,
                                    int present, uint8_t* out_crop, uint32_t* lsum, void* stream) {
    if (!out_crop) return MAS_ERR_NULL;
    if (int e = augment_check(img, hbounds, hk, vbounds, vk, xidx, yidx, fill, H, W, th, tw, hks, vks, gap_y, gap_x, crop_i, crop_j, out_h,
                              out_w, map0, map0_dtype, out_map0, map1, map1_dtype, out_map1))
        return e;
    mas_pm_chain c;
    if (int e = make_chain(order, factor, present, 0, &c)) return e;
    const int cpos = mas_pm_contrast_pos(&c);
    if (cpos < MAS_PM_OPS && !lsum) return MAS_ERR_NULL;          // contrast needs the sum
    if ((long long)out_h * out_w > (1LL << 24)) return MAS_ERR_SHAPE;          // 255 * 2^24 < 2^32
    MapArg a0{map0, out_map0, (long long)pad0, map0_dtype, out0_u8}, a1{map1, out_map1, (long long)pad1, map1_dtype, out1_u8};
    const AugGeom q{img, H, W, th, tw, hbounds, hk, hks, vbounds, vk, vks, xidx, yidx, gap_y, gap_x, crop_i, crop_j, flip, out_h, out_w,
                    (int)fill[0], (int)fill[1], (int)fill[2], a0, a1};
    const int n = out_h * out_w;
    hipLaunchKernelGGL(k_train_augment_u8, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), q, c, cpos, out_crop, cpos < MAS_PM_OPS ? lsum : nullptr);
    return mas_launch_status();
}

static int photometric_check(const void* crop, int h, int w, const float* mean, const float* std) {
    if (!crop || !mean || !std) return MAS_ERR_NULL;
    if (h <= 0 || w <= 0 || (long long)h * w > (1LL << 24)) return MAS_ERR_SHAPE;
    return 0;
}

extern "C" int mas_photometric(const uint8_t* crop, int h, int w, const int32_t* order, const float* factor, int present, int grey,
                               const float* mean, const float* std, const uint32_t* lsum, float* out_img, uint8_t* out_u8, void* stream) {
    if (int e = photometric_check(crop, h, w, mean, std)) return e;
    if (!out_img) return MAS_ERR_NULL;
    if ((reinterpret_cast<uintptr_t>(crop) & 3) || (reinterpret_cast<uintptr_t>(out_img) & 15)) return MAS_ERR_ALIGN;
    mas_pm_chain c;
    if (int e = make_chain(order, factor, present, grey, &c)) return e;
    const bool contrast = mas_pm_contrast_pos(&c) < MAS_PM_OPS;
    if (contrast && !lsum) return MAS_ERR_NULL;
    const int n = h * w;
    const unsigned blocks = (unsigned)(((n + kPix - 1) / kPix + kThreads - 1) / kThreads);
    const unsigned* ls = contrast ? lsum : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n % kPix == 0)
        hipLaunchKernelGGL(k_photometric<true>, dim3(blocks), dim3(kThreads), 0, st, crop, n, c, ls, mean[0], mean[1], mean[2], std[0],
                           std[1], std[2], out_img, out_u8);
    else
        hipLaunchKernelGGL(k_photometric<false>, dim3(blocks), dim3(kThreads), 0, st, crop, n, c, ls, mean[0], mean[1], mean[2], std[0],
                           std[1], std[2], out_img, out_u8);
    return mas_launch_status();
}

// The CPU-side statement of the spec: host pointers, plain loops through photometric.h, the contrast sum included.  No device is
// touched.  out_u8 (HWC), out_img (f32 CHW) and lsum_out may each be NULL.
extern "C" int mas_photometric_reference(const uint8_t* crop, int h, int w, const int32_t* order, const float* factor, int present,
                                         int grey, const float* mean, const float* std, uint8_t* out_u8, float* out_img,
                                         uint32_t* lsum_out) {
    if (int e = photometric_check(crop, h, w, mean, std)) return e;
    mas_pm_chain c;
    if (int e = make_chain(order, factor, present, grey, &c)) return e;
    const int cpos = mas_pm_contrast_pos(&c);
    const size_t n = (size_t)h * w;
    unsigned long long sum = 0;
    if (cpos < MAS_PM_OPS) {
        for (size_t p = 0; p < n; ++p) {
            int r = crop[3 * p], g = crop[3 * p + 1], b = crop[3 * p + 2];
            mas_pm_apply(&c, 0, cpos, 0, &r, &g, &b);
            sum += (unsigned)mas_pm_grey(r, g, b);
        }
    }
    if (lsum_out) *lsum_out = (uint32_t)sum;
    const int cmean = cpos < MAS_PM_OPS ? mas_pm_contrast_mean(sum, n) : 0;
    for (size_t p = 0; p < n; ++p) {
        int r = crop[3 * p], g = crop[3 * p + 1], b = crop[3 * p + 2];
        mas_pm_pixel(&c, cmean, &r, &g, &b);
        if (out_u8) {
            out_u8[3 * p] = (uint8_t)r; out_u8[3 * p + 1] = (uint8_t)g; out_u8[3 * p + 2] = (uint8_t)b;
        }
        if (out_img) {
            out_img[p] = mas_pm_normalise(r, mean[0], std[0]);
            out_img[n + p] = mas_pm_normalise(g, mean[1], std[1]);
            out_img[2 * n + p] = mas_pm_normalise(b, mean[2], std[2]);
        }
    }
    return 0;
}
