// stage2.hip -- K9: stage-2 cosine pseudo-label generation with one-ring propagation, for gfx950.
//
// Reference: trainer/eval_save_cosplbl_prop.py:121-314 (+ ..._includeonehot.py): nested Python loops over the selected
// superpixels, a 2.1 GB full-resolution feature tensor per image (feat_forward upsamples 256 channels to 1024x2048),
// skimage dilation on the CPU per superpixel.  Here:
//   * the per-(superpixel, class) arg-max pixel table comes from mas_partial_loss_fwd (invT = 1, group flags);
//   * features are read from the QUARTER-resolution map and interpolated in registers (align_corners=False, same
//     operation order as F.interpolate) -- the 2.1 GB tensor is never materialised;
//   * k_stage2_assign      nearest prototype of the own superpixel for every valid pixel;
//   * k_stage2_assign_labels  the label map of that assignment alone (eval_save_cosplbl.py: no expansion);
//   * k_stage2_adjacency   3x3-dilation adjacency of superpixels as an S x S bit matrix (one pass over the id map);
//   * k_stage2_propagate   every pixel looks at the valid superpixels adjacent to its own superpixel in ascending id
//                          order; the last one whose prototype similarity passes that prototype's threshold wins --
//                          exactly the result of the reference's sequential overwrite.
//   * k_s2thr_*            per-prototype threshold between assign and propagate: the minimum or the lower median of the
//                          similarities of the pixels a prototype attracted, picked by rank on integer keys (no sort,
//                          no arithmetic on the similarities but sim + 0.0f, integer atomics only).
// Dot products are sequential fma chains over the channels (normative, mirrored by oracle/exact.c).
#include "common.h"

namespace {
constexpr int kThreads = 256;

struct FeatMap {
    const float* f;
    int Ch, fh, fw, H, W;
};

struct Interp {
    int o00, o01, o10, o11;
    float l0h, l1h, l0w, l1w;
    bool direct;
};

__device__ __forceinline__ Interp make_interp(const FeatMap& m, int y, int x) {
    Interp it;
    it.direct = (m.fh == m.H && m.fw == m.W);
    if (it.direct) {
        it.o00 = y * m.W + x;
        it.o01 = it.o10 = it.o11 = it.o00;
        it.l0h = it.l0w = 1.0f;
        it.l1h = it.l1w = 0.0f;
        return it;
    }
    const float sh = (float)m.fh / (float)m.H, sw = (float)m.fw / (float)m.W;
    float sy = sh * ((float)y + 0.5f) - 0.5f;
    sy = sy < 0.0f ? 0.0f : sy;
    float sx = sw * ((float)x + 0.5f) - 0.5f;
    sx = sx < 0.0f ? 0.0f : sx;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < m.fh - 1 ? 1 : 0), x1 = x0 + (x0 < m.fw - 1 ? 1 : 0);
    it.l1h = sy - (float)y0;
    it.l0h = 1.0f - it.l1h;
    it.l1w = sx - (float)x0;
    it.l0w = 1.0f - it.l1w;
    it.o00 = y0 * m.fw + x0; it.o01 = y0 * m.fw + x1;
    it.o10 = y1 * m.fw + x0; it.o11 = y1 * m.fw + x1;
    return it;
}

__device__ __forceinline__ float feat_at(const FeatMap& m, const Interp& it, int k) {
    const float* p = m.f + (size_t)k * m.fh * m.fw;
    if (it.direct) return p[it.o00];
    return it.l0h * (it.l0w * p[it.o00] + it.l1w * p[it.o01]) + it.l1h * (it.l0w * p[it.o10] + it.l1w * p[it.o11]);
}

__global__ __launch_bounds__(kThreads) void k_stage2_gather_protos(FeatMap m, const int* __restrict__ proto_pix, int n_proto,
                                                                    float* __restrict__ P) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)n_proto * m.Ch) return;
    const int j = (int)(i / m.Ch), k = (int)(i - (long long)j * m.Ch);
    const int pix = proto_pix[j];
    const Interp it = make_interp(m, pix / m.W, pix % m.W);
    P[i] = feat_at(m, it, k);
}

// similarities of one pixel to the prototypes [j0, j1): first maximum and "any above its threshold"
__device__ __forceinline__ void proto_scan(const FeatMap& m, const Interp& it, const float* __restrict__ P,
                                           const float* __restrict__ thr, int j0, int j1, float& best, int& arg, bool& ok) {
    for (int j = j0; j < j1; j += 4) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const int n = (j1 - j) < 4 ? (j1 - j) : 4;
        for (int k = 0; k < m.Ch; ++k) {
            const float fx = feat_at(m, it, k);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < n) acc[u] = mas_fmaf(P[(size_t)(j + u) * m.Ch + k], fx, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u < n) {
                if (arg < 0 || acc[u] > best) { best = acc[u]; arg = j + u; }
                if (thr && thr[j + u] < acc[u]) ok = true;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_stage2_assign(FeatMap m, const long long* __restrict__ spx,
                                                             const unsigned char* __restrict__ mask, int S,
                                                             const int* __restrict__ p_start, const float* __restrict__ P,
                                                             int* __restrict__ nn, float* __restrict__ nn_sim) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m.H * m.W) return;
    int arg = -1;
    float best = 0.0f;
    if (mask[i]) {
        const long long id = spx[i];
        if (id >= 0 && id < S && p_start[id + 1] > p_start[id]) {
            const Interp it = make_interp(m, i / m.W, i % m.W);
            bool ok = false;
            proto_scan(m, it, P, nullptr, p_start[id], p_start[id + 1], best, arg, ok);
        }
    }
    nn[i] = arg;
    nn_sim[i] = best;
}

// the label map of the generator that stops after the assignment (trainer/eval_save_cosplbl.py:186-192)
__global__ __launch_bounds__(kThreads) void k_stage2_assign_labels(const int* __restrict__ nn, const int* __restrict__ p_cls, int HW,
                                                                    long long* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= HW) return;
    const int own = nn[i];
    out[i] = own >= 0 ? p_cls[own] : 255;
}

__global__ __launch_bounds__(kThreads) void k_stage2_adjacency(const long long* __restrict__ spx, int H, int W, int S,
                                                                const int* __restrict__ p_start, unsigned* __restrict__ adj) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= H * W) return;
    const long long t = spx[i];
    if (t < 0 || t >= S) return;
    const int words = (S + 31) / 32;
    const int y = i / W, x = i % W;
    long long last = -1;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const long long g = spx[(size_t)yy * W + xx];
            if (g < 0 || g >= S || g == last || p_start[g + 1] == p_start[g]) continue;
            last = g;
            const unsigned bit = 1u << (g & 31);
            unsigned* w = &adj[(size_t)t * words + (g >> 5)];
            if (!(*w & bit)) atomicOr(w, bit);
        }
}

__global__ __launch_bounds__(kThreads) void k_stage2_propagate(FeatMap m, const long long* __restrict__ spx, int S,
                                                                const unsigned* __restrict__ adj, const int* __restrict__ p_start,
                                                                const int* __restrict__ p_cls, const float* __restrict__ P,
                                                                const float* __restrict__ thr, const int* __restrict__ nn,
                                                                long long* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m.H * m.W) return;
    int label = 255;
    const long long t = spx[i];
    if (t >= 0 && t < S) {
        const int words = (S + 31) / 32;
        const Interp it = make_interp(m, i / m.W, i % m.W);
        for (int w = 0; w < words; ++w) {
            unsigned bitsw = adj[(size_t)t * words + w];
            while (bitsw) {                       // ascending superpixel id: later neighbours overwrite earlier ones
                const int b = __ffs(bitsw) - 1;
                bitsw &= bitsw - 1;
                const int s = w * 32 + b;
                float best = 0.0f;
                int arg = -1;
                bool ok = false;
                proto_scan(m, it, P, thr, p_start[s], p_start[s + 1], best, arg, ok);
                if (ok) label = p_cls[arg];
            }
        }
    }
    const int own = nn[i];
    if (own >= 0) label = p_cls[own];
    out[i] = label;
}

// ------------------------------------------------------------------------------------------------
// Per-prototype thresholds (trainer/eval_save_cosplbl_prop.py:243-254): thr[k] over {nn_sim[i] : nn_proto[i] == k}.
// Similarities are ordered by the monotone 32-bit key of sim + 0.0f (-0.0 and +0.0 are one key): negatives with all
// bits flipped, non-negatives with the sign bit set.  The result is the float whose key was picked.
//   min:    atomicMin on the key.
//   median: 4 x 8-bit radix select of the key of rank (cnt - 1) / 2.  Per prototype the state is {prefix, rank}; a round
//           counts, per prototype, the next digit of the keys that share the prefix found so far (k_s2thr_hist), then
//           one wave per prototype scans the 256 bins, appends the digit that holds the rank, takes the bins below it
//           off the rank and zeroes the bins for the next round (k_s2thr_pick).  The first round matches every key, so
//           its bins also give cnt.
// Neighbouring pixels mostly share prototype and digit (round 0 hits a handful of bins: similarities lie in a narrow
// band), so a wave first merges its lanes on the bin and one lane adds the count; lanes left after kMergeRounds
// distinct bins add on their own.
// ------------------------------------------------------------------------------------------------
constexpr int kMergeRounds = 4;
constexpr unsigned kNoKey = 0xffffffffu;       // min: no pixel yet; median: rank of a prototype without pixels
// min: one key per 128-byte line.  Packed, the ~500 keys of a picture share 18 lines and every wave's atomic queues on one of them
// (42 us for the 2 M pixels of a 1024 x 2048 picture); a line each, and a coherent read that skips what cannot lower the key: 15 us.
constexpr int kMinStride = 32;

__device__ __forceinline__ unsigned sim_key(float v) {
    const unsigned u = mas_f2u(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_sim(unsigned key) {
    return mas_u2f((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// state [n_proto] {prefix, rank} = {0, 0}; hist [n_proto * 256] = 0   (median)  /  keys [n_proto * kMinStride] = kNoKey   (min)
__global__ __launch_bounds__(kThreads) void k_s2thr_init(unsigned* __restrict__ words, long long n, unsigned value) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) words[i] = value;
}

// merged(same, writer, s): for up to kMergeRounds distinct slots s of the wave, `same` marks the lanes that hold s and `writer` one
// of them; called by every lane of the wave (so the caller returns from no lane before this, and merged() may use wave operations).
// single(): called by the lanes whose slot was not served, each for itself.
template <typename Merged, typename Single>
__device__ __forceinline__ void wave_merge(bool todo, int slot, Merged merged, Single single) {
    const int lane = threadIdx.x & (MAS_WAVE - 1);
    for (int r = 0; r < kMergeRounds; ++r) {
        const mas_u64 open = __ballot(todo);
        if (!open) return;
        const int leader = __ffsll((long long)open) - 1;
        const int s = __shfl(slot, leader);
        const bool same = todo && slot == s;
        merged(same, lane == leader, s);
        todo = todo && !same;
    }
    if (todo) single();
}

__global__ __launch_bounds__(kThreads) void k_s2thr_min(const int* __restrict__ nn, const float* __restrict__ nn_sim, int HW,
                                                         int n_proto, unsigned* __restrict__ keys) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    int k = -1;
    unsigned key = kNoKey;
    if (i < HW) {
        k = nn[i];
        if (k >= 0 && k < n_proto) key = sim_key(nn_sim[i]);
        else k = -1;
    }
    wave_merge(k >= 0, k, [&](bool same, bool writer, int s) {
        unsigned m = same ? key : kNoKey;
#pragma unroll
        for (int d = 1; d < MAS_WAVE; d <<= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)m, d);
            m = o < m ? o : m;
        }
        // (keys only go down: an old value read here costs an atomic, never a result)
        if (writer && m < __hip_atomic_load(&keys[(size_t)s * kMinStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMin(&keys[(size_t)s * kMinStride], m);
    }, [&]() { atomicMin(&keys[(size_t)k * kMinStride], key); });
}

__global__ __launch_bounds__(kThreads) void k_s2thr_min_out(const unsigned* __restrict__ keys, int n_proto, float* __restrict__ thr) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k < n_proto) {
        const unsigned key = keys[(size_t)k * kMinStride];
        thr[k] = key == kNoKey ? 1.0f : key_sim(key);
    }
}

// round with digit at bit `shift` (24, 16, 8, 0): hist[k][digit] += 1 for every pixel of k whose key continues k's prefix
__global__ __launch_bounds__(kThreads) void k_s2thr_hist(const int* __restrict__ nn, const float* __restrict__ nn_sim, int HW,
                                                          int n_proto, int shift, const uint2* __restrict__ state,
                                                          unsigned* __restrict__ hist) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    int slot = -1;
    if (i < HW) {
        const int k = nn[i];
        if (k >= 0 && k < n_proto) {
            const unsigned key = sim_key(nn_sim[i]);
            // (shift == 24: no digit is fixed yet.  A prototype without pixels is never looked up here.)
            if (shift == 24 || ((key ^ state[k].x) >> (shift + 8)) == 0) slot = k * 256 + (int)((key >> shift) & 255u);
        }
    }
    wave_merge(slot >= 0, slot, [&](bool same, bool writer, int s) {
        const mas_u64 m = __ballot(same);
        if (writer) atomicAdd(&hist[s], (unsigned)__popcll(m));
    }, [&]() { atomicAdd(&hist[slot], 1u); });
}

// one wave per prototype: lane l owns bins 4 l .. 4 l + 3
__global__ __launch_bounds__(MAS_WAVE) void k_s2thr_pick(int shift, uint2* __restrict__ state, unsigned* __restrict__ hist,
                                                          float* __restrict__ thr) {
    const int k = blockIdx.x, lane = threadIdx.x;
    uint4* bins = reinterpret_cast<uint4*>(hist + (size_t)k * 256) + lane;
    const uint4 b = *bins;
    *bins = make_uint4(0u, 0u, 0u, 0u);
    const unsigned own = b.x + b.y + b.z + b.w;
    unsigned upto = own;                                        // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < MAS_WAVE; d <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)upto, d);
        if (lane >= d) upto += o;
    }
    uint2 st = state[k];
    if (shift == 24) {
        const unsigned cnt = (unsigned)__shfl((int)upto, MAS_WAVE - 1);
        st.y = cnt ? (cnt - 1u) / 2u : kNoKey;
    }
    if (st.y == kNoKey) {                                       // no pixel: 1.0 (:245)
        if (lane == 0) {
            if (shift == 24) state[k] = st;
            if (shift == 0) thr[k] = 1.0f;
        }
        return;
    }
    const unsigned below = upto - own;
    if (st.y >= below && st.y < upto) {                         // exactly one lane: the bins up to it hold the rank, those before do not
        unsigned r = st.y - below, digit = 4u * (unsigned)lane;
        if (r >= b.x) { r -= b.x; ++digit;
            if (r >= b.y) { r -= b.y; ++digit;
                if (r >= b.z) { r -= b.z; ++digit; } } }
        st.x |= digit << shift;
        st.y = r;
        state[k] = st;
        if (shift == 0) thr[k] = key_sim(st.x);
    }
}
}  // namespace

static int stage2_check(const float* feat, int Ch, int fh, int fw, int H, int W) {
    if (!feat) return MAS_ERR_NULL;
    if (Ch <= 0 || fh <= 0 || fw <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL / 2 || fh > H || fw > W)
        return MAS_ERR_SHAPE;
    return 0;
}

extern "C" int mas_stage2_gather_protos(const float* feat, int Ch, int fh, int fw, int H, int W, const int32_t* proto_pix, int n_proto,
                                        float* P, void* stream) {
    if (int e = stage2_check(feat, Ch, fh, fw, H, W)) return e;
    if (!proto_pix || !P) return MAS_ERR_NULL;
    if (n_proto <= 0) return MAS_ERR_SHAPE;
    const long long n = (long long)n_proto * Ch;
    hipLaunchKernelGGL(k_stage2_gather_protos, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), (FeatMap{feat, Ch, fh, fw, H, W}), proto_pix, n_proto, P);
    return mas_launch_status();
}

extern "C" int mas_stage2_assign(const float* feat, int Ch, int fh, int fw, int H, int W, const int64_t* spx, const uint8_t* mask, int S,
                                 const int32_t* proto_start, const float* P, int32_t* nn_proto, float* nn_sim, void* stream) {
    if (int e = stage2_check(feat, Ch, fh, fw, H, W)) return e;
    if (!spx || !mask || !proto_start || !P || !nn_proto || !nn_sim) return MAS_ERR_NULL;
    hipLaunchKernelGGL(k_stage2_assign, dim3((unsigned)((H * W + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), (FeatMap{feat, Ch, fh, fw, H, W}), reinterpret_cast<const long long*>(spx), mask,
                       S, proto_start, P, nn_proto, nn_sim);
    return mas_launch_status();
}

extern "C" int mas_stage2_assign_labels(const int32_t* nn_proto, const int32_t* proto_cls, int HW, int64_t* out, void* stream) {
    if (!nn_proto || !proto_cls || !out) return MAS_ERR_NULL;
    if (HW <= 0 || HW > 0x7fffffff - kThreads) return MAS_ERR_SHAPE;
    hipLaunchKernelGGL(k_stage2_assign_labels, dim3((unsigned)((HW + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), nn_proto, proto_cls, HW, reinterpret_cast<long long*>(out));
    return mas_launch_status();
}

extern "C" int mas_stage2_adjacency(const int64_t* spx, int H, int W, int S, const int32_t* proto_start, uint32_t* adj, void* stream) {
    if (!spx || !proto_start || !adj) return MAS_ERR_NULL;
    if (H <= 0 || W <= 0 || S <= 0) return MAS_ERR_SHAPE;
    hipLaunchKernelGGL(k_stage2_adjacency, dim3((unsigned)((H * W + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const long long*>(spx), H, W, S, proto_start, adj);
    return mas_launch_status();
}

extern "C" int mas_stage2_propagate(const float* feat, int Ch, int fh, int fw, int H, int W, const int64_t* spx, int S,
                                    const uint32_t* adj, const int32_t* proto_start, const int32_t* proto_cls, const float* P,
                                    const float* thr, const int32_t* nn_proto, int64_t* out, void* stream) {
    if (int e = stage2_check(feat, Ch, fh, fw, H, W)) return e;
    if (!spx || !adj || !proto_start || !proto_cls || !P || !thr || !nn_proto || !out) return MAS_ERR_NULL;
    hipLaunchKernelGGL(k_stage2_propagate, dim3((unsigned)((H * W + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), (FeatMap{feat, Ch, fh, fw, H, W}), reinterpret_cast<const long long*>(spx), S, adj,
                       proto_start, proto_cls, P, thr, nn_proto, reinterpret_cast<long long*>(out));
    return mas_launch_status();
}

static int64_t thresholds_words(int n_proto, int method) {
    if (n_proto <= 0 || n_proto > (0x7fffffff >> 8)) return MAS_ERR_RANGE;
    if (method == MAS_STAGE2_THR_MIN) return (int64_t)n_proto * kMinStride;
    if (method == MAS_STAGE2_THR_MEDIAN) return (int64_t)n_proto * (256 + 2);
    return MAS_ERR_SHAPE;
}

extern "C" int64_t mas_stage2_thresholds_scratch_bytes(int n_proto, int method) {
    const int64_t w = thresholds_words(n_proto, method);
    return w < 0 ? w : w * 4;
}

extern "C" int mas_stage2_thresholds(const int32_t* nn_proto, const float* nn_sim, int HW, int n_proto, int method, void* scratch,
                                     int64_t scratch_bytes, float* thr, void* stream) {
    if (method != MAS_STAGE2_THR_MEDIAN && method != MAS_STAGE2_THR_MIN) return MAS_ERR_SHAPE;
    if (!nn_proto || !nn_sim || !scratch || !thr) return MAS_ERR_NULL;
    if (HW <= 0 || HW > 0x7fffffff - kThreads) return MAS_ERR_SHAPE;
    const int64_t words = thresholds_words(n_proto, method);
    if (words < 0) return (int)words;
    if (scratch_bytes < words * 4) return MAS_ERR_WORKSPACE;
    if ((uintptr_t)scratch & 15) return MAS_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 px((unsigned)((HW + kThreads - 1) / kThreads)), tb(kThreads);
    unsigned* w = static_cast<unsigned*>(scratch);
    const bool is_min = method == MAS_STAGE2_THR_MIN;
    hipLaunchKernelGGL(k_s2thr_init, dim3((unsigned)((words + kThreads - 1) / kThreads)), tb, 0, st, w, (long long)words,
                       is_min ? kNoKey : 0u);
    if (is_min) {
        hipLaunchKernelGGL(k_s2thr_min, px, tb, 0, st, nn_proto, nn_sim, HW, n_proto, w);
        hipLaunchKernelGGL(k_s2thr_min_out, dim3((unsigned)((n_proto + kThreads - 1) / kThreads)), tb, 0, st, w, n_proto, thr);
        return mas_launch_status();
    }
    unsigned* hist = w;                                         // [n_proto, 256], 16-byte aligned rows
    uint2* state = reinterpret_cast<uint2*>(w + (size_t)n_proto * 256);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_s2thr_hist, px, tb, 0, st, nn_proto, nn_sim, HW, n_proto, shift, state, hist);
        hipLaunchKernelGGL(k_s2thr_pick, dim3((unsigned)n_proto), dim3(MAS_WAVE), 0, st, shift, state, hist, thr);
    }
    return mas_launch_status();
}
