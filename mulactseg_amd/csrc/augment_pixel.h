// augment_pixel.h -- the per-pixel geometry of the training augmentation, shared by k_train_augment (augment.hip: f32 CHW out) and
// k_train_augment_u8 (photometric.hip: u8 HWC out for the photometric pass): one output pixel of the crop walks back through flip,
// crop and padding to a pixel of the SCALED image, evaluates Pillow's two-pass 8-bit BILINEAR resampling for it and copies the
// NEAREST-resampled maps.  Integer arithmetic only; what a caller does with (r, g, b) is its own business.
#ifndef MULACTSEG_AUGMENT_PIXEL_H
#define MULACTSEG_AUGMENT_PIXEL_H

#include "common.h"

namespace {
constexpr int kAugPrec = 22;      // Pillow: PRECISION_BITS = 32 - 8 - 2

struct MapArg {
    const void* src;
    void* dst;
    long long pad;
    int in_dtype;       // MAS_ID_I64 / MAS_ID_I32 / MAS_ID_U16 / MAS_MAP_U8
    int out_u8;         // 1: uint8 output, 0: int64 output
};

struct AugGeom {
    const unsigned char* img;
    int H, W, th, tw;
    const int* hb; const int* hk; int hks;
    const int* vb; const int* vk; int vks;
    const int* xidx; const int* yidx;
    int gap_y, gap_x, ci, cj, flip, oh, ow;
    int f0, f1, f2;
    MapArg a0, a1;
};

__device__ __forceinline__ long long load_map(const void* p, int dtype, size_t i) {
    switch (dtype) {
        case MAS_ID_I64: return static_cast<const long long*>(p)[i];
        case MAS_ID_I32: return static_cast<const int*>(p)[i];
        case MAS_ID_U16: return static_cast<const unsigned short*>(p)[i];
        default: return static_cast<const unsigned char*>(p)[i];
    }
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Output pixel o < oh * ow: its colour goes to (r, g, b), its map values are written.
__device__ __forceinline__ void augment_pixel(const AugGeom& q, int o, int& r, int& g, int& b) {
    const unsigned char* __restrict__ img = q.img;
    const int* __restrict__ hb = q.hb; const int* __restrict__ hk = q.hk;
    const int* __restrict__ vb = q.vb; const int* __restrict__ vk = q.vk;
    const int H = q.H, W = q.W, th = q.th, tw = q.tw, hks = q.hks, vks = q.vks, ow = q.ow;
    const int oy = o / ow, ox = o - oy * ow;
    const int sx = q.flip ? (ow - 1 - ox) : ox;
    const int y = q.ci + oy - q.gap_y, x = q.cj + sx - q.gap_x;          // pixel of the scaled image
    const bool inside = (y >= 0 && y < th && x >= 0 && x < tw);
    r = q.f0; g = q.f1; b = q.f2;
    if (inside) {
        const int x0 = hb[2 * x], xn = hb[2 * x + 1];
        const int y0 = vb[2 * y], yn = vb[2 * y + 1];
        const bool need_h = (tw != W), need_v = (th != H);
        long long ar = 1 << (kAugPrec - 1), ag = ar, ab = ar;
        const int rows = need_v ? yn : 1;
        for (int t = 0; t < rows; ++t) {
            const int sy = need_v ? (y0 + t) : y;
            const unsigned char* row = img + (size_t)sy * W * 3;
            int hr, hg, hbv;
            if (need_h) {
                int cr = 1 << (kAugPrec - 1), cg = cr, cb = cr;      // <= 5 taps * 255 * 2^22 fits 32 bits
                for (int u = 0; u < xn; ++u) {
                    const int k = hk[x * hks + u];
                    const unsigned char* px = row + (size_t)(x0 + u) * 3;
                    cr += px[0] * k; cg += px[1] * k; cb += px[2] * k;
                }
                hr = clip8(cr >> kAugPrec); hg = clip8(cg >> kAugPrec); hbv = clip8(cb >> kAugPrec);
            } else {
                const unsigned char* px = row + (size_t)x * 3;
                hr = px[0]; hg = px[1]; hbv = px[2];
            }
            if (need_v) {
                const int k = vk[y * vks + t];
                ar += (long long)hr * k; ag += (long long)hg * k; ab += (long long)hbv * k;
            } else {
                r = hr; g = hg; b = hbv;
            }
        }
        if (need_v) {
            r = clip8((int)(ar >> kAugPrec)); g = clip8((int)(ag >> kAugPrec)); b = clip8((int)(ab >> kAugPrec));
        }
    }
    const MapArg* maps[2] = {&q.a0, &q.a1};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const MapArg& a = *maps[k];
        if (!a.src) continue;
        const long long v = inside ? load_map(a.src, a.in_dtype, (size_t)q.yidx[y] * W + q.xidx[x]) : a.pad;
        if (a.out_u8) static_cast<unsigned char*>(a.dst)[o] = (unsigned char)v;
        else static_cast<long long*>(a.dst)[o] = v;
    }
}

// the argument checks of mas_train_augment, shared by mas_train_augment_u8 (0: fine)
inline int augment_check(const void* img, const void* hbounds, const void* hk, const void* vbounds, const void* vk, const void* xidx,
                         const void* yidx, const void* fill, int H, int W, int th, int tw, int hks, int vks, int gap_y, int gap_x,
                         int crop_i, int crop_j, int out_h, int out_w, const void* map0, int map0_dtype, const void* out_map0,
                         const void* map1, int map1_dtype, const void* out_map1) {
    if (!img || !hbounds || !hk || !vbounds || !vk || !xidx || !yidx || !fill) return MAS_ERR_NULL;
    if ((map0 && !out_map0) || (map1 && !out_map1)) return MAS_ERR_NULL;
    if (H <= 0 || W <= 0 || th <= 0 || tw <= 0 || out_h <= 0 || out_w <= 0 || hks <= 0 || vks <= 0 || hks > 9 || vks > 9 ||
        (long long)out_h * out_w > 0x7fffffffLL)
        return MAS_ERR_SHAPE;
    if (gap_y < 0 || gap_x < 0 || crop_i < 0 || crop_j < 0 || crop_i + out_h > th + 2 * gap_y || crop_j + out_w > tw + 2 * gap_x)
        return MAS_ERR_RANGE;
    for (int d : {map0 ? map0_dtype : 0, map1 ? map1_dtype : 0})
        if (d < 0 || d > MAS_MAP_U8) return MAS_ERR_DTYPE;
    return 0;
}
}  // namespace

#endif  // MULACTSEG_AUGMENT_PIXEL_H
