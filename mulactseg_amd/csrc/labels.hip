// labels.hip -- region labels of one picture for the data-generation step (multi-hot query labels and dominant-label maps).
//
// Reference: dataloader/region_cityscapes_tensor.py:23-86 (tools/label_assignment_tensor[_voc].py) and
// dataloader/region_cityscapes_dominant_all[_sample].py:24-62 (tools/label_assignment_dominant[_voc].py).  The reference loops in
// Python over every listed superpixel and compares the whole id map for each; here one pass over the pixels builds, per superpixel,
// the histogram of its labels (column C = the ignore value 255), and every per-id answer is read off that histogram.
//
//   k_region_counts    tile of 64 x 16 pixels per workgroup.  With trimming, the id tile plus a halo of k/2 + 1 is staged in LDS,
//                      the thick boundary (skimage find_boundaries(mode='thick'): some in-image 4-neighbour has another id) is
//                      computed there and dilated by the k x k square separably (rows, then columns; the window is clipped at the
//                      picture's edge, ndimage.binary_dilation with border_value 0).  Two int32 [nseg, C+1] histograms: all pixels
//                      of an id, and those outside the dilated band.  A lane owns 4 neighbouring pixels of a row and adds one run per
//                      (id, label) into an LDS slot table of the ids seen in the tile; an id that finds no free slot goes straight
//                      to global atomics.  Integer atomics: the counts do not depend on the order of arrival.
//   k_region_finalize  one lane per id: the multi-hot row (trimmed counts, or the full ones when the trimmed region is empty) and
//                      its size, or the dominant label (arg-max with ties to the smaller value, or a choice drawn on the host).
//   k_region_paint     one lane per pixel: the dominant-label map.
//   k_spx_max_onehot   stage 2 with dominant labels (trainer/eval_save_cosplbl_prop_onehotignore.py:29-58): per superpixel the largest
//                      target value (torch_scatter.scatter_max), and the mask target != 255.  A workgroup owns a contiguous run of
//                      pixels, a lane 8 consecutive ones; each run of equal ids within a lane goes into an LDS table of all nseg
//                      ids with one LDS atomicMax, and the table reaches the global maxima with one atomicMax per touched id.
//   k_spx_onehot_rows  the finalize step: one lane per (id, class) writes the one-hot row of the id's maximum (255 -> C - 1; an id
//                      with no pixel gets the row of value 0, torch_scatter's fill for an empty segment).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64;                      // 16 lanes x 4 pixels per row
constexpr int kTileH = 16;                      // 16 rows: 256 lanes
constexpr int kMaxK = 15;
constexpr int kMaxR = kMaxK / 2 + 1;            // halo of the id tile
constexpr int kCols = kTileW + 2 * kMaxR;       // 80
constexpr int kRows = kTileH + 2 * kMaxR;       // 32
constexpr int kLogSlots = 6;
constexpr int kSlots = 1 << kLogSlots;
constexpr int kNoId = 0x7fffffff;

template <typename IdT>
__device__ __forceinline__ int load_id32(const IdT* p, size_t i) {
    return (int)p[i];
}
template <>
__device__ __forceinline__ int load_id32<long long>(const long long* p, size_t i) {
    const long long v = p[i];                   // saturated: ids beyond int32 compare equal to each other (they belong to no region)
    return v < -0x7fffffffLL ? -0x7fffffff : (v > 0x7ffffffeLL ? 0x7ffffffe : (int)v);
}

__device__ __forceinline__ int table_slot(int* keys, int id) {
    unsigned h = ((unsigned)id * 2654435769u) >> (32 - kLogSlots);
    for (int probe = 0; probe < kSlots; ++probe) {
        const int k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == id) return (int)h;
        if (k == -1) {
            const int old = atomicCAS(&keys[h], -1, id);
            if (old == -1 || old == id) return (int)h;
        }
        h = (h + 1) & (kSlots - 1);
    }
    return -1;
}

// add one run of `nf` pixels of (id, col), `nt` of them outside the trimmed band
template <bool TRIM>
__device__ __forceinline__ void add_run(int* t_keys, unsigned* t_full, unsigned* t_trim, unsigned* full, unsigned* trim, int C1, int id,
                                        int col, unsigned nf, unsigned nt) {
    const int s = table_slot(t_keys, id);
    if (s >= 0) {
        atomicAdd(&t_full[s * C1 + col], nf);
        if (TRIM && nt) atomicAdd(&t_trim[s * C1 + col], nt);
    } else {
        atomicAdd(&full[(size_t)id * C1 + col], nf);
        if (TRIM && nt) atomicAdd(&trim[(size_t)id * C1 + col], nt);
    }
}

template <typename IdT, bool TRIM>
__global__ __launch_bounds__(kThreads) void k_region_counts(const IdT* __restrict__ spx, const unsigned char* __restrict__ lab, int H,
                                                             int W, int nseg, int C, int half, unsigned* __restrict__ full,
                                                             unsigned* __restrict__ trim, int* __restrict__ status) {
    __shared__ int s_id[TRIM ? kRows * kCols : 1];
    __shared__ unsigned char s_b[TRIM ? kRows * kCols : 1];       // boundary bit
    __shared__ unsigned char s_h[TRIM ? kRows * kTileW : 1];      // boundary OR-ed along the row
    __shared__ int t_keys[kSlots];
    __shared__ unsigned t_full[kSlots * MAS_MAX_CLASSES];
    __shared__ unsigned t_trim[TRIM ? kSlots * MAS_MAX_CLASSES : 1];
    const int C1 = C + 1;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;

    for (int i = tid; i < kSlots; i += kThreads) t_keys[i] = -1;
    for (int i = tid; i < kSlots * C1; i += kThreads) {
        t_full[i] = 0;
        if (TRIM) t_trim[i] = 0;
    }
    if (TRIM) {
        // LDS cell (ly, lx) holds picture pixel (y0 - kMaxR + ly, x0 - kMaxR + lx)
        const int r = half + 1;
        const int rows = kTileH + 2 * r, cols = kTileW + 2 * r;
        for (int i = tid; i < rows * cols; i += kThreads) {
            const int ly = i / cols, lx = i - (i / cols) * cols;
            const int gy = y0 - r + ly, gx = x0 - r + lx;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W)
                s_id[(ly + kMaxR - r) * kCols + lx + kMaxR - r] = load_id32(spx, (size_t)gy * W + gx);
        }
        __syncthreads();
        const int rb = kTileH + 2 * half, cb = kTileW + 2 * half;
        for (int i = tid; i < rb * cb; i += kThreads) {
            const int ly = i / cb, lx = i - (i / cb) * cb;
            const int gy = y0 - half + ly, gx = x0 - half + lx;
            const int L = (ly + kMaxR - half) * kCols + lx + kMaxR - half;
            unsigned char b = 0;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const int v = s_id[L];
                b = (gy > 0 && s_id[L - kCols] != v) || (gy + 1 < H && s_id[L + kCols] != v) || (gx > 0 && s_id[L - 1] != v) ||
                    (gx + 1 < W && s_id[L + 1] != v);
            }
            s_b[L] = b;
        }
        __syncthreads();
        for (int i = tid; i < rb * kTileW; i += kThreads) {
            const int ly = i / kTileW, lx = i - (i / kTileW) * kTileW;
            const int Ly = ly + kMaxR - half;
            const unsigned char* row = &s_b[Ly * kCols + lx + kMaxR];
            unsigned char o = 0;
            for (int d = -half; d <= half; ++d) o |= row[d];
            s_h[Ly * kTileW + lx] = o;
        }
    }
    __syncthreads();

    // a lane's 4 pixels: row ty, columns sx .. sx + 3 of the tile
    const int ty = tid >> 4, sx = (tid & 15) * 4;
    const int gy = y0 + ty;
    int cur_id = kNoId, cur_col = 0;
    unsigned nf = 0, nt = 0;
    int bad = 0;
    if (gy < H) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gx = x0 + sx + j;
            if (gx >= W) break;
            const size_t pix = (size_t)gy * W + gx;
            const int id = TRIM ? s_id[(ty + kMaxR) * kCols + sx + j + kMaxR] : load_id32(spx, pix);
            const int l = lab[pix];
            if (l >= C && l != 255) { bad = 1; continue; }
            if (id < 0 || id >= nseg) continue;
            const int col = l == 255 ? C : l;
            unsigned in_band = 0;
            if (TRIM) {
                const unsigned char* c = &s_h[(ty + kMaxR) * kTileW + sx + j];
                for (int d = -half; d <= half; ++d) in_band |= c[d * kTileW];
            }
            if (id != cur_id || col != cur_col) {
                if (cur_id != kNoId) add_run<TRIM>(t_keys, t_full, t_trim, full, trim, C1, cur_id, cur_col, nf, nt);
                cur_id = id;
                cur_col = col;
                nf = nt = 0;
            }
            nf += 1;
            nt += in_band ? 0u : 1u;
        }
    }
    if (cur_id != kNoId) add_run<TRIM>(t_keys, t_full, t_trim, full, trim, C1, cur_id, cur_col, nf, nt);
    if (bad) atomicOr(status, MAS_LABELS_BAD_VALUE);
    __syncthreads();
    for (int i = tid; i < kSlots * C1; i += kThreads) {
        const int key = t_keys[i / C1];
        if (key < 0) continue;
        const int col = i - (i / C1) * C1;
        if (t_full[i]) atomicAdd(&full[(size_t)key * C1 + col], t_full[i]);
        if (TRIM && t_trim[i]) atomicAdd(&trim[(size_t)key * C1 + col], t_trim[i]);
    }
}

// bits/size != NULL: multi-hot rows; choice != NULL: dominant values (drawn != NULL: the host's draw, a column index or -1)
__global__ __launch_bounds__(kThreads) void k_region_finalize(const int* __restrict__ full, const int* __restrict__ trim,
                                                               const unsigned char* __restrict__ listed, const int* __restrict__ drawn,
                                                               int nseg, int C, int generate_ignore, unsigned char* __restrict__ bits,
                                                               long long* __restrict__ size, int* __restrict__ choice) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= nseg) return;
    const int C1 = C + 1;
    const bool on = listed[p] != 0;
    if (bits) {
        const int* row = full + (size_t)p * C1;
        if (trim && on) {
            long long nt = 0;
            for (int c = 0; c < C1; ++c) nt += trim[(size_t)p * C1 + c];
            if (nt > 0) row = trim + (size_t)p * C1;         // the trimmed region when it is not empty (:64-66)
        }
        long long n = 0;
        for (int c = 0; c < C1; ++c) {
            const int v = on ? row[c] : 0;
            bits[(size_t)p * C1 + c] = v > 0;
            n += v;
        }
        size[p] = on ? n : -1;
    }
    if (choice) {
        int best = -1;
        if (on) {
            if (drawn) {
                best = drawn[p];
            } else {
                const int hi = generate_ignore ? C1 : C;        // without generate_ignore the ignore pixels are left out
                int bv = 0;
                for (int c = 0; c < hi; ++c) {
                    const int v = full[(size_t)p * C1 + c];
                    if (v > bv) { bv = v; best = c; }           // strict: ties go to the smaller value; 255 (column C) is the largest
                }
            }
        }
        choice[p] = best < 0 ? -1 : (best == C ? 255 : best);
    }
}

template <typename IdT>
__global__ __launch_bounds__(kThreads) void k_region_paint(const IdT* __restrict__ spx, const unsigned char* __restrict__ lab, long long n,
                                                            int nseg, const int* __restrict__ choice, int generate_ignore,
                                                            unsigned char* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const int id = load_id32(spx, (size_t)i);
        const int l = lab[i];
        int v = l;
        if (id >= 0 && id < nseg && (generate_ignore || l != 255)) {
            const int c = choice[id];
            if (c >= 0) v = c;
        }
        out[i] = (unsigned char)v;
    }
}

int check_picture(const void* spx, int spx_dtype, const uint8_t* labels, int H, int W, int nseg) {
    if (!spx || !labels) return MAS_ERR_NULL;
    if (spx_dtype != MAS_ID_I64 && spx_dtype != MAS_ID_I32 && spx_dtype != MAS_ID_U16) return MAS_ERR_DTYPE;
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || nseg <= 0) return MAS_ERR_SHAPE;
    return 0;
}

template <typename IdT>
void launch_counts(const void* spx, const uint8_t* labels, int H, int W, int nseg, int C, int trim_k, int32_t* full, int32_t* trimmed,
                   int32_t* status, hipStream_t st) {
    const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH));
    const IdT* s = static_cast<const IdT*>(spx);
    unsigned* f = reinterpret_cast<unsigned*>(full);
    if (trim_k)
        hipLaunchKernelGGL((k_region_counts<IdT, true>), grid, dim3(kThreads), 0, st, s, labels, H, W, nseg, C, trim_k / 2, f,
                           reinterpret_cast<unsigned*>(trimmed), status);
    else
        hipLaunchKernelGGL((k_region_counts<IdT, false>), grid, dim3(kThreads), 0, st, s, labels, H, W, nseg, C, 0, f, nullptr, status);
}
// ------------------------------------------------------------------------------------------------------------------------------
// dominant-label target rows of one picture (k_spx_max_onehot + k_spx_onehot_rows)
constexpr int kMaxPix = 8;                     // consecutive pixels per lane
constexpr int kMaxChunk = kThreads * kMaxPix;  // pixels per workgroup
constexpr int kMaxSeg = 16384;                 // LDS table: 64 KB

template <typename TgtT>
__device__ __forceinline__ int load_target(const TgtT* p, size_t i) {
    return (int)p[i];
}
template <>
__device__ __forceinline__ int load_target<long long>(const long long* p, size_t i) {
    const long long v = p[i];                   // anything outside [0, 255] is a bad value; -1 keeps it recognisable as one
    return v < 0 || v > 255 ? -1 : (int)v;
}

template <typename IdT, typename TgtT>
__global__ __launch_bounds__(kThreads) void k_spx_max_onehot(const TgtT* __restrict__ target, const IdT* __restrict__ spx, long long n,
                                                              int nseg, int C, int* __restrict__ seg_max, unsigned char* __restrict__ mask,
                                                              int* __restrict__ status) {
    extern __shared__ int t_max[];              // [nseg], -1 = no pixel of this id in the workgroup's run
    const int tid = threadIdx.x;
    for (int i = tid; i < nseg; i += kThreads) t_max[i] = -1;
    __syncthreads();
    const long long p0 = (long long)blockIdx.x * kMaxChunk + (long long)tid * kMaxPix;
    int cur_id = -1, cur = -1, bad = 0;
    for (int j = 0; j < kMaxPix; ++j) {
        const long long p = p0 + j;
        if (p >= n) break;
        const int t = load_target(target, (size_t)p);
        const int id = load_id32(spx, (size_t)p);
        mask[p] = t != 255;
        if ((t < 0 || t >= C) && t != 255) { bad = 1; continue; }
        if (id < 0 || id >= nseg) continue;
        if (id != cur_id) {
            if (cur_id >= 0) atomicMax(&t_max[cur_id], cur);
            cur_id = id;
            cur = t;
        } else {
            cur = t > cur ? t : cur;
        }
    }
    if (cur_id >= 0) atomicMax(&t_max[cur_id], cur);
    if (bad) atomicOr(status, MAS_LABELS_BAD_VALUE);
    __syncthreads();
    for (int i = tid; i < nseg; i += kThreads)
        if (t_max[i] >= 0) atomicMax(&seg_max[i], t_max[i]);
}

__global__ __launch_bounds__(kThreads) void k_spx_onehot_rows(const int* __restrict__ seg_max, int nseg, int C,
                                                               unsigned char* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)nseg * C) return;
    const int id = (int)(i / C), c = (int)(i - (long long)id * C);
    const int m = seg_max[id];
    const int v = m < 0 ? 0 : (m == 255 ? C - 1 : m);
    rows[i] = c == v;
}

template <typename IdT, typename TgtT>
void launch_spx_max(const void* target, const void* spx, long long n, int nseg, int C, int32_t* seg_max, uint8_t* mask, int32_t* status,
                    hipStream_t st) {
    hipLaunchKernelGGL((k_spx_max_onehot<IdT, TgtT>), dim3((unsigned)((n + kMaxChunk - 1) / kMaxChunk)), dim3(kThreads),
                       sizeof(int) * (size_t)nseg, st, static_cast<const TgtT*>(target), static_cast<const IdT*>(spx), n, nseg, C, seg_max,
                       mask, status);
}

template <typename IdT>
void launch_spx_max_ids(const void* target, int target_dtype, const void* spx, long long n, int nseg, int C, int32_t* seg_max,
                        uint8_t* mask, int32_t* status, hipStream_t st) {
    if (target_dtype == MAS_MAP_U8)
        launch_spx_max<IdT, unsigned char>(target, spx, n, nseg, C, seg_max, mask, status, st);
    else
        launch_spx_max<IdT, long long>(target, spx, n, nseg, C, seg_max, mask, status, st);
}
}  // namespace

extern "C" int mas_spx_max_onehot(const void* target, int target_dtype, const void* spx, int spx_dtype, int H, int W, int nseg,
                                  int num_classes, int32_t* seg_max, int32_t* status, uint8_t* mask, uint8_t* rows, void* stream) {
    if (!target || !spx || !seg_max || !status || !mask || !rows) return MAS_ERR_NULL;
    if (target_dtype != MAS_MAP_U8 && target_dtype != MAS_ID_I64) return MAS_ERR_DTYPE;
    if (spx_dtype != MAS_ID_I64 && spx_dtype != MAS_ID_I32 && spx_dtype != MAS_ID_U16) return MAS_ERR_DTYPE;
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return MAS_ERR_SHAPE;
    if (nseg <= 0 || nseg > kMaxSeg) return MAS_ERR_RANGE;
    if (num_classes < 1 || num_classes > 255) return MAS_ERR_CLASSES;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(seg_max, 0xff, sizeof(int32_t) * (size_t)nseg, st);      // -1: no pixel
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const long long n = (long long)H * W;
    if (spx_dtype == MAS_ID_I64)
        launch_spx_max_ids<long long>(target, target_dtype, spx, n, nseg, num_classes, seg_max, mask, status, st);
    else if (spx_dtype == MAS_ID_I32)
        launch_spx_max_ids<int>(target, target_dtype, spx, n, nseg, num_classes, seg_max, mask, status, st);
    else
        launch_spx_max_ids<unsigned short>(target, target_dtype, spx, n, nseg, num_classes, seg_max, mask, status, st);
    if (int r = mas_launch_status()) return r;
    const long long cells = (long long)nseg * num_classes;
    hipLaunchKernelGGL(k_spx_onehot_rows, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, seg_max, nseg,
                       num_classes, rows);
    return mas_launch_status();
}

extern "C" int mas_region_label_counts(const void* spx, int spx_dtype, const uint8_t* labels, int H, int W, int nseg, int num_classes,
                                       int trim_k, int32_t* full, int32_t* trimmed, int32_t* status, void* stream) {
    if (int e = check_picture(spx, spx_dtype, labels, H, W, nseg)) return e;
    if (!full || !status || (trim_k && !trimmed)) return MAS_ERR_NULL;
    if (num_classes < 1 || num_classes + 1 > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    if (trim_k < 0 || trim_k > kMaxK || (trim_k && trim_k % 2 == 0)) return MAS_ERR_RANGE;
    if ((long long)nseg * (num_classes + 1) > 0x7fffffffLL) return MAS_ERR_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t bytes = sizeof(int32_t) * (size_t)nseg * (num_classes + 1);
    hipError_t e = hipMemsetAsync(full, 0, bytes, st);
    if (e == hipSuccess && trim_k) e = hipMemsetAsync(trimmed, 0, bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    if (spx_dtype == MAS_ID_I64)
        launch_counts<long long>(spx, labels, H, W, nseg, num_classes, trim_k, full, trimmed, status, st);
    else if (spx_dtype == MAS_ID_I32)
        launch_counts<int>(spx, labels, H, W, nseg, num_classes, trim_k, full, trimmed, status, st);
    else
        launch_counts<unsigned short>(spx, labels, H, W, nseg, num_classes, trim_k, full, trimmed, status, st);
    return mas_launch_status();
}

extern "C" int mas_region_multi_hot(const int32_t* full, const int32_t* trimmed, const uint8_t* listed, int nseg, int num_classes,
                                    uint8_t* bits, int64_t* size, void* stream) {
    if (!full || !listed || !bits || !size) return MAS_ERR_NULL;
    if (nseg <= 0) return MAS_ERR_SHAPE;
    if (num_classes < 1 || num_classes + 1 > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    hipLaunchKernelGGL(k_region_finalize, dim3((unsigned)((nseg + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), full, trimmed, listed, nullptr, nseg, num_classes, 0, bits,
                       reinterpret_cast<long long*>(size), nullptr);
    return mas_launch_status();
}

extern "C" int mas_region_dominant(const int32_t* full, const uint8_t* listed, const int32_t* drawn, int nseg, int num_classes,
                                   int generate_ignore, int32_t* choice, void* stream) {
    if (!full || !listed || !choice) return MAS_ERR_NULL;
    if (nseg <= 0) return MAS_ERR_SHAPE;
    if (num_classes < 1 || num_classes + 1 > MAS_MAX_CLASSES) return MAS_ERR_CLASSES;
    hipLaunchKernelGGL(k_region_finalize, dim3((unsigned)((nseg + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), full, nullptr, listed, drawn, nseg, num_classes, generate_ignore ? 1 : 0,
                       nullptr, nullptr, choice);
    return mas_launch_status();
}

extern "C" int mas_region_paint(const void* spx, int spx_dtype, const uint8_t* labels, int H, int W, int nseg, const int32_t* choice,
                                int generate_ignore, uint8_t* out, void* stream) {
    if (int e = check_picture(spx, spx_dtype, labels, H, W, nseg)) return e;
    if (!choice || !out) return MAS_ERR_NULL;
    const long long n = (long long)H * W;
    long long nblk = (n + kThreads - 1) / kThreads;
    if (nblk > 4096) nblk = 4096;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int gi = generate_ignore ? 1 : 0;
    if (spx_dtype == MAS_ID_I64)
        hipLaunchKernelGGL(k_region_paint<long long>, dim3((unsigned)nblk), dim3(kThreads), 0, st, static_cast<const long long*>(spx),
                           labels, n, nseg, choice, gi, out);
    else if (spx_dtype == MAS_ID_I32)
        hipLaunchKernelGGL(k_region_paint<int>, dim3((unsigned)nblk), dim3(kThreads), 0, st, static_cast<const int*>(spx), labels, n,
                           nseg, choice, gi, out);
    else
        hipLaunchKernelGGL(k_region_paint<unsigned short>, dim3((unsigned)nblk), dim3(kThreads), 0, st,
                           static_cast<const unsigned short*>(spx), labels, n, nseg, choice, gi, out);
    return mas_launch_status();
}
