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
}  // namespace

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
