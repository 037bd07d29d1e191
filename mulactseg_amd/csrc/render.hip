// render.hip -- colour images of label maps for --save_vis and eval_naive_vis.
//
// Reference: trainer/eval_save_cosplbl_prop.py:77-86 (and the five other stage-2 generators) and trainer/eval_naive_vis.py:70-83.
//   mark_boundaries(decode_target(masked_fill(plbl, plbl == 255, F)).astype('uint8'), superpixels) * 255, .astype('uint8')
//   decode_target(preds[:, :-1].max(1)[1])
// Semantics (normative; tests/render_restated.py restates them in numpy, INTEGRATION.md section 5 derives them from skimage):
//   1. colour: label 255 -> fill; then palette[label], a label outside [0, P) counted in *n_bad (the pixel is written black).
//   2. mark_boundaries form only (skimage's defaults: mode 'outer', background 0, colour (1, 1, 0)), on the int64 id map s with the
//      neighbour outside the picture = the edge pixel (scipy's 'reflect' for a 3 x 3 footprint):
//        thick = max over the 3 x 3 cross of s != min over the cross
//        bg    = s == 0;  inv = s with bg set to INT64_MAX
//        mark  = thick && (bg || max over the 3 x 3 square of s != min over the square of inv)
//      A marked pixel is (255, 255, 0); every other channel value c becomes uint8(float64(c) * (1.0 / 255) * 255) (img_as_float and
//      the * 255 / astype of the reference: 24 byte values go down by one, e.g. 244 -> 243, 180 -> 179).
//   3. the plain form (no superpixels) writes the palette colours themselves.
//
// Shape: a lane owns 4 consecutive pixels of the flat [N,H,W] map and writes their 12 bytes as 3 aligned dwords (the last, partial
// group byte by byte).  When the 4 pixels share a row the 3 x 6 window of ids around them is read once; otherwise each pixel reads
// its own 3 x 3.  The palette (<= 256 entries, round trip applied) sits in LDS as packed 0x00BBGGRR words.
#include "common.h"

namespace {
constexpr int kThreads = 256;
constexpr int kPix = 4;
constexpr int kMaxPalette = 256;

struct RenderArgs {
    const void* labels;           // [N,H,W] int64 (MAS_ID_I64) or uint8 (MAS_MAP_U8)
    const int64_t* spx;           // [N,H,W] or NULL (plain form)
    const uint8_t* palette;       // [P,3]
    uint8_t* rgb;                 // [N,H,W,3]
    unsigned* n_bad;              // labels outside the palette after the fill (NULL: the caller guarantees there are none)
    size_t total;                 // N * H * W
    int H, W, P, fill;
};

// float64 round trip of skimage's img_as_float (* 1/255) and the reference's * 255 / astype('uint8') (truncation)
__device__ __forceinline__ unsigned round_trip(unsigned c) {
    return (unsigned)((double)c * (1.0 / 255.0) * 255.0);
}

// the outer-mode mark of the centre of a 3 x 3 window w[r][c] (r, c = 0..2; (1, 1) the pixel)
__device__ __forceinline__ bool outer_mark(const int64_t (&w)[3][3]) {
    const int64_t c = w[1][1];
    int64_t mx = c, mn = c;
    mx = max(mx, max(max(w[0][1], w[2][1]), max(w[1][0], w[1][2])));
    mn = min(mn, min(min(w[0][1], w[2][1]), min(w[1][0], w[1][2])));
    if (mx == mn) return false;                   // not on the thick boundary
    if (c == 0) return true;                      // background side
    int64_t mx9 = INT64_MIN, mn9 = INT64_MAX;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t v = w[r][k];
            mx9 = max(mx9, v);
            mn9 = min(mn9, v == 0 ? (int64_t)INT64_MAX : v);
        }
    return mx9 != mn9;
}

template <typename LabelT>
__global__ __launch_bounds__(kThreads) void k_render_labels(const RenderArgs a) {
    __shared__ unsigned pal[kMaxPalette];
    const bool marks = a.spx != nullptr;
    for (int i = threadIdx.x; i < a.P; i += kThreads) {
        unsigned r = a.palette[3 * i], g = a.palette[3 * i + 1], b = a.palette[3 * i + 2];
        if (marks) r = round_trip(r), g = round_trip(g), b = round_trip(b);
        pal[i] = r | (g << 8) | (b << 16);
    }
    __syncthreads();
    const LabelT* lab = static_cast<const LabelT*>(a.labels);
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    const size_t groups = (a.total + kPix - 1) / kPix;
    for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (size_t)gridDim.x * kThreads) {
        const size_t p0 = g * kPix;
        const int n = a.total - p0 < (size_t)kPix ? (int)(a.total - p0) : kPix;
        unsigned col[kPix] = {0, 0, 0, 0};
        for (int k = 0; k < n; ++k) {
            long long v = (long long)lab[p0 + k];
            if (v == 255) v = a.fill;
            if (v < 0 || v >= a.P) {
                if (a.n_bad) atomicAdd(a.n_bad, 1u);
            } else {
                col[k] = pal[v];
            }
        }
        if (marks) {
            const size_t pic = p0 / plane, pix = p0 - pic * plane;
            const int64_t* s = a.spx + pic * plane;
            const int y = (int)(pix / W), x0 = (int)(pix - (size_t)y * W);
            const int yr[3] = {max(y - 1, 0), y, min(y + 1, H - 1)};
            if (n == kPix && x0 + kPix <= W) {        // one row: the 3 x 6 window, read once
                int64_t win[3][kPix + 2];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < kPix + 2; ++c) win[r][c] = s[(size_t)yr[r] * W + min(max(x0 - 1 + c, 0), W - 1)];
#pragma unroll
                for (int k = 0; k < kPix; ++k) {
                    int64_t w3[3][3];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) w3[r][c] = win[r][k + c];
                    if (outer_mark(w3)) col[k] = 0x00ffffu;
                }
            } else {                                  // the group crosses a row or picture end: each pixel on its own
                for (int k = 0; k < n; ++k) {
                    const size_t q = p0 + k, qc = q / plane, qp = q - qc * plane;
                    const int64_t* sq = a.spx + qc * plane;
                    const int qy = (int)(qp / W), qx = (int)(qp - (size_t)qy * W);
                    int64_t w3[3][3];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            w3[r][c] = sq[(size_t)min(max(qy - 1 + r, 0), H - 1) * W + min(max(qx - 1 + c, 0), W - 1)];
                    if (outer_mark(w3)) col[k] = 0x00ffffu;
                }
            }
        }
        uint8_t* out = a.rgb + 3 * p0;
        if (n == kPix) {                              // 12 bytes, 4-byte aligned (the host checked rgb)
            unsigned* o = reinterpret_cast<unsigned*>(out);
            o[0] = col[0] | (col[1] << 24);
            o[1] = (col[1] >> 8) | (col[2] << 16);
            o[2] = (col[2] >> 16) | (col[3] << 8);
        } else {
            for (int k = 0; k < n; ++k) {
                out[3 * k] = (uint8_t)col[k];
                out[3 * k + 1] = (uint8_t)(col[k] >> 8);
                out[3 * k + 2] = (uint8_t)(col[k] >> 16);
            }
        }
    }
}

int launch_render(const RenderArgs& a, int label_dtype, hipStream_t st) {
    const size_t groups = (a.total + kPix - 1) / kPix;
    size_t blocks = (groups + kThreads - 1) / kThreads;
    blocks = blocks > 8192 ? 8192 : blocks;           // (grid-stride beyond 8192 x 256 lanes: 2 M groups per sweep)
    if (label_dtype == MAS_ID_I64)
        hipLaunchKernelGGL(k_render_labels<int64_t>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(k_render_labels<uint8_t>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    return mas_launch_status();
}
}  // namespace

extern "C" int mas_render_labels(const void* labels, int label_dtype, int N, int H, int W, const uint8_t* palette, int P, int fill,
                                 const int64_t* spx, int mark_boundaries, uint8_t* rgb, unsigned* n_bad, void* stream) {
    if (!labels || !palette || !rgb || !n_bad || (mark_boundaries && !spx)) return MAS_ERR_NULL;
    if (label_dtype != MAS_ID_I64 && label_dtype != MAS_MAP_U8) return MAS_ERR_DTYPE;
    if (N < 1 || H < 1 || W < 1) return MAS_ERR_SHAPE;
    if (P < 1 || P > kMaxPalette || fill < 0 || fill >= P) return MAS_ERR_RANGE;
    if (((uintptr_t)rgb & 3) != 0) return MAS_ERR_ALIGN;
    RenderArgs a;
    a.labels = labels, a.spx = mark_boundaries ? spx : nullptr, a.palette = palette, a.rgb = rgb, a.n_bad = n_bad;
    a.total = (size_t)N * H * W, a.H = H, a.W = W, a.P = P, a.fill = fill;
    return launch_render(a, label_dtype, static_cast<hipStream_t>(stream));
}

// First form: mas_naive_plbl on picture i's first CH - 1 channels (a contiguous prefix of the picture) with an all-ones mask into
// work[i HW, (i + 1) HW), then one plain render of the N label maps.  The labels lie in [0, CH - 1) and P >= CH - 1, so no pixel can
// fall outside the palette.  work: (N + 1) H W bytes (the labels, then the mask).
extern "C" int mas_render_lowres_pred(const float* z_q, int N, int CH, int h, int w, int H, int W, const uint8_t* palette, int P,
                                      uint8_t* work, uint8_t* rgb, void* stream) {
    if (!z_q || !palette || !work || !rgb) return MAS_ERR_NULL;
    if (CH < 2 || CH - 1 > 255) return MAS_ERR_CLASSES;
    if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1) return MAS_ERR_SHAPE;
    const bool ident = h == H && w == W;
    if (!ident && (h > H || w > W || (long long)W > 6LL * w || H > 65535)) return MAS_ERR_SHAPE;     // mas_naive_plbl's geometries
    if (P < CH - 1 || P > kMaxPalette) return MAS_ERR_RANGE;
    if (((uintptr_t)rgb & 3) != 0) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t plane = (size_t)H * W;
    uint8_t* ones = work + (size_t)N * plane;
    hipError_t e = hipMemsetAsync(ones, 1, plane, st);
    if (e != hipSuccess) return (int)e;
    for (int i = 0; i < N; ++i) {
        const int rc = mas_naive_plbl(z_q + (size_t)i * CH * h * w, 1, CH - 1, h, w, H, W, ones, 0.0f, work + (size_t)i * plane, stream);
        if (rc != 0) return rc;
    }
    RenderArgs a;
    a.labels = work, a.spx = nullptr, a.palette = palette, a.rgb = rgb, a.n_bad = nullptr;
    a.total = (size_t)N * plane, a.H = H, a.W = W, a.P = P, a.fill = 0;
    return launch_render(a, MAS_MAP_U8, st);
}
