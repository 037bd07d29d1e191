// augment.hip -- training-time geometry on the device: random scale (Pillow BILINEAR for the
// picture, NEAREST for label / superpixel maps), pad-if-needed, random crop, horizontal flip, to-float, normalise --
// reference dataloader/transform.py:105-113 with dataloader/ext_transforms.py:172-192, 443-520, 323-341, 384-437.
//
// One output-driven kernel per sample: every output pixel of the crop walks back through flip, crop and padding to a
// pixel (y, x) of the SCALED image and evaluates Pillow's two-pass 8-bit resampling for just that pixel: the vertical
// pass over <= ksize_v rows of the horizontally resampled picture, each of which is <= ksize_h taps of the source row,
// rounded to u8 in between exactly as Pillow's temporary image is.  The fixed-point coefficient tables (22 fractional
// bits) and the nearest-neighbour index tables are computed on the host in double precision, as Pillow computes them
// (dataloader/device_transforms.py); the kernel is integer arithmetic up to the final (v/255 - mean)/std in f32.
// The source picture (6 MB for 1024x2048) and the tables stay in L2; HBM traffic is the 7 MB crop that is written.
#include "common.h"
#include "augment_pixel.h"

namespace {
constexpr int kThreads = 256;

// the per-pixel geometry is augment_pixel.h's (shared with photometric.hip: k_train_augment_u8); this kernel normalises and writes f32 CHW
__global__ __launch_bounds__(kThreads) void k_train_augment(const AugGeom q, float m0, float m1, float m2, float s0, float s1, float s2,
                                                             float* __restrict__ out) {
    const int o = blockIdx.x * kThreads + threadIdx.x;
    if (o >= q.oh * q.ow) return;
    int r, g, b;
    augment_pixel(q, o, r, g, b);
    const size_t plane = (size_t)q.oh * q.ow;
    out[o] = ((float)r / 255.0f - m0) / s0;
    out[plane + o] = ((float)g / 255.0f - m1) / s1;
    out[2 * plane + o] = ((float)b / 255.0f - m2) / s2;
}

// The maps alone: what augment_pixel does with its two map slots, for a third and fourth map of a sample whose picture the main launch
// has resampled already.  Same walk back through flip, crop and padding, same NEAREST tables; no picture is read.
struct MapsGeom {
    int W, th, tw;
    const int* xidx; const int* yidx;
    int gap_y, gap_x, ci, cj, flip, oh, ow;
    MapArg a0, a1;
};

__global__ __launch_bounds__(kThreads) void k_train_augment_maps(const MapsGeom q) {
    const int o = blockIdx.x * kThreads + threadIdx.x;
    if (o >= q.oh * q.ow) return;
    const int oy = o / q.ow, ox = o - oy * q.ow;
    const int sx = q.flip ? (q.ow - 1 - ox) : ox;
    const int y = q.ci + oy - q.gap_y, x = q.cj + sx - q.gap_x;          // pixel of the scaled image
    const bool inside = (y >= 0 && y < q.th && x >= 0 && x < q.tw);
    const size_t at = inside ? (size_t)q.yidx[y] * q.W + q.xidx[x] : 0;
    const MapArg* maps[2] = {&q.a0, &q.a1};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const MapArg& a = *maps[k];
        if (!a.src) continue;
        const long long v = inside ? load_map(a.src, a.in_dtype, at) : a.pad;
        if (a.out_u8) static_cast<unsigned char*>(a.dst)[o] = (unsigned char)v;
        else static_cast<long long*>(a.dst)[o] = v;
    }
}
}  // namespace

extern "C" int mas_train_augment_maps(int H, int W, int th, int tw, const int32_t* xidx, const int32_t* yidx, int gap_y, int gap_x, int crop_i,
                                      int crop_j, int flip, int out_h, int out_w, const void* map0, int map0_dtype, int64_t pad0,
                                      void* out_map0, int out0_u8, const void* map1, int map1_dtype, int64_t pad1, void* out_map1, int out1_u8,
                                      void* stream) {
    if (!xidx || !yidx || (!map0 && !map1)) return MAS_ERR_NULL;
    if ((map0 && !out_map0) || (map1 && !out_map1)) return MAS_ERR_NULL;
    if (H <= 0 || W <= 0 || th <= 0 || tw <= 0 || out_h <= 0 || out_w <= 0 || (long long)out_h * out_w > 0x7fffffffLL) return MAS_ERR_SHAPE;
    if (gap_y < 0 || gap_x < 0 || crop_i < 0 || crop_j < 0 || crop_i + out_h > th + 2 * gap_y || crop_j + out_w > tw + 2 * gap_x)
        return MAS_ERR_RANGE;
    for (int d : {map0 ? map0_dtype : 0, map1 ? map1_dtype : 0})
        if (d < 0 || d > MAS_MAP_U8) return MAS_ERR_DTYPE;
    const MapsGeom q{W, th, tw, xidx, yidx, gap_y, gap_x, crop_i, crop_j, flip, out_h, out_w,
                     MapArg{map0, out_map0, (long long)pad0, map0_dtype, out0_u8}, MapArg{map1, out_map1, (long long)pad1, map1_dtype, out1_u8}};
    const int n = out_h * out_w;
    hipLaunchKernelGGL(k_train_augment_maps, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), q);
    return mas_launch_status();
}

extern "C" int mas_train_augment(const uint8_t* img, int H, int W, int th, int tw, const int32_t* hbounds, const int32_t* hk, int hks,
                                 const int32_t* vbounds, const int32_t* vk, int vks, const int32_t* xidx, const int32_t* yidx,
                                 int gap_y, int gap_x, int crop_i, int crop_j, int flip, int out_h, int out_w, const float* mean,
                                 const float* std, const uint8_t* fill, const void* map0, int map0_dtype, int64_t pad0, void* out_map0,
                                 int out0_u8, const void* map1, int map1_dtype, int64_t pad1, void* out_map1, int out1_u8,
                                 float* out_img, void* stream) {
    if (!mean || !std || !out_img) return MAS_ERR_NULL;
    if (int e = augment_check(img, hbounds, hk, vbounds, vk, xidx, yidx, fill, H, W, th, tw, hks, vks, gap_y, gap_x, crop_i, crop_j, out_h,
                              out_w, map0, map0_dtype, out_map0, map1, map1_dtype, out_map1))
        return e;
    MapArg a0{map0, out_map0, (long long)pad0, map0_dtype, out0_u8}, a1{map1, out_map1, (long long)pad1, map1_dtype, out1_u8};
    const AugGeom q{img, H, W, th, tw, hbounds, hk, hks, vbounds, vk, vks, xidx, yidx, gap_y, gap_x, crop_i, crop_j, flip, out_h, out_w,
                    (int)fill[0], (int)fill[1], (int)fill[2], a0, a1};
    const int n = out_h * out_w;
    hipLaunchKernelGGL(k_train_augment, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       q, mean[0], mean[1], mean[2], std[0], std[1], std[2], out_img);
    return mas_launch_status();
}
