// ms_ensemble.hip -- the multi-scale + flip ensemble of the VOC stage-2 generator in one launch.
//
// Reference: trainer/eval_save_cosplbl_prop_includeonehot_voc_ms.py:56-79.  Every source k (a scaled, possibly flipped copy of the
// picture) went through feat_forward: quarter-resolution features / logits upsampled x4 bilinearly to the scaled size (Hs, Ws),
// flipped back, F.interpolate'd to the original (H, W), averaged, the features re-normalised over the channels.  Materialised, that is
// 256 channels at every scaled size and again at the original size per source (~11 GB of traffic for a 500x375 picture).  Here the
// quarter-resolution maps are read once per output tile and the scaled-size values live in LDS only.
//
// Arithmetic (normative; tests/ms_ensemble_restated.py restates it in numpy).  tap(scale, o, n):
//   s = max(0, scale*(o+0.5)-0.5), i0 = (int)s, i1 = i0 + (i0 < n-1), l1 = s - i0, l0 = 1 - l1       (upsample.hip, ATen's
//   area_pixel_compute_source_index); scale = (float)in / (float)out, computed on the host.
//   1. stage 1, quarter (hq, wq) -> scaled (Hs, Ws):   S(r,c) = l0h*(l0w*q[i0h][i0w] + l1w*q[i0h][i1w]) + l1h*(l0w*q[i1h][i0w] + l1w*q[i1h][i1w])
//      -- the expression of k_upsample_fwd, so S equals mas_upsample_bilinear_fwd on the materialised tensor bit for bit;
//   2. flip (flipped sources): stage-2 taps are computed in flipped coordinates, stage-1 column j is read as column Ws-1-j;
//   3. stage 2, scaled -> original (H, W), the same tap and expression over S (a downsample for factors > 1);
//   4. mean: v_0 + v_1 + ... + v_{n-1} in source order, then / (float)n;
//   5. features only: ss = sum over channels in channel order of m*m (multiply, then add -- no fma under -ffp-contract=off),
//      d = max(sqrtf(ss), 1e-12) (correctly rounded sqrt), out = m / d.
//
// Shape: a workgroup owns an 8 x 32 output tile and walks the channels in blocks of kCB, sources innermost.  Per (block, source):
//   A. the quarter rows the tile needs, lerped horizontally once per needed stage-1 column, into LDS;
//   B. the stage-1 rows the tile needs, combined vertically from A, into LDS (the S values above, in the same operation order);
//   C. one output pixel per thread, stage 2 from B, accumulated in registers.
// The mean features are written once, the per-pixel sum of squares stays in a register, and the normalisation re-reads the
// thread's own freshly written lines (L2 / Infinity Cache) -- no full-picture round trip.  LDS extents are the exact maxima over
// tiles and sources, computed on the host with the same tap arithmetic.
#include "common.h"

namespace {
constexpr int kTH = 8, kTW = 32;           // output tile
constexpr int kThreads = kTH * kTW;        // one output pixel per thread
constexpr int kCB = 8;                     // channels per LDS block
constexpr int kWaves = kThreads / MAS_WAVE;
constexpr size_t kMaxLds = 64 * 1024;

struct Tap { int i0, i1; float l0, l1; };

__host__ __device__ __forceinline__ Tap make_tap(float scale, int o, int n_in) {
    float s = scale * ((float)o + 0.5f) - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    Tap t;
    t.i0 = (int)s;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

struct MsSrc {
    const float* feat;            // [Ch, hq, wq]
    const float* logit;           // [C, hq, wq]
    int hq, wq, hs, ws, flip;
    float s1h, s1w, s2h, s2w;     // stage-1 (quarter -> scaled) and stage-2 (scaled -> original) scales
};

struct MsArgs {
    MsSrc src[MAS_MS_MAX_SOURCES];
    float* feat_out;              // [Ch, H, W]
    float* logit_out;             // [C, H, W]
    int n, Ch, C, H, W;
    int nrq, nr1, nc1;            // LDS extents: quarter rows, stage-1 rows, stage-1 columns of one tile
};

// stage-1 row range [r_lo, r_hi] and quarter row range [q_lo, q_hi] of output rows y0..y1 (unflipped axis)
__host__ __device__ __forceinline__ void row_span(const MsSrc& s, int y0, int y1, int& r_lo, int& r_hi, int& q_lo, int& q_hi) {
    r_lo = make_tap(s.s2h, y0, s.hs).i0;
    r_hi = make_tap(s.s2h, y1, s.hs).i1;
    q_lo = make_tap(s.s1h, r_lo, s.hq).i0;
    q_hi = make_tap(s.s1h, r_hi, s.hq).i1;
}

// stage-1 column range [c_lo, c_hi] (unflipped stage-1 coordinates) of output columns x0..x1
__host__ __device__ __forceinline__ void col_span(const MsSrc& s, int x0, int x1, int& c_lo, int& c_hi) {
    const int b_lo = make_tap(s.s2w, x0, s.ws).i0, b_hi = make_tap(s.s2w, x1, s.ws).i1;
    c_lo = s.flip ? s.ws - 1 - b_hi : b_lo;
    c_hi = s.flip ? s.ws - 1 - b_lo : b_hi;
}

// grid: (ceil(W / kTW), ceil(H / kTH)); dynamic LDS: kCB * (nrq + nr1) * nc1 floats
__global__ __launch_bounds__(kThreads) void k_ms_ensemble(const MsArgs a) {
    extern __shared__ float lds[];
    float* hbuf = lds;                                   // [kCB][nrq][nc1]: quarter rows lerped horizontally
    float* sbuf = lds + kCB * a.nrq * a.nc1;             // [kCB][nr1][nc1]: stage-1 values
    const int tid = threadIdx.x, lane = tid & (MAS_WAVE - 1), wave = tid / MAS_WAVE;
    const int H = a.H, W = a.W, NCH = a.Ch + a.C;
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    const int y1 = min(y0 + kTH, H) - 1, x1 = min(x0 + kTW, W) - 1;
    const int py = y0 + tid / kTW, px = x0 + tid % kTW;
    const bool live = py < H && px < W;
    const int cy = min(py, y1), cx = min(px, x1);        // taps of a pixel outside the picture: those of the tile's last one
    const size_t plane = (size_t)H * W, pix = (size_t)cy * W + cx;
    float ss = 0.0f;
    for (int ch0 = 0; ch0 < NCH; ch0 += kCB) {
        const int nb = min(kCB, NCH - ch0);
        float acc[kCB];
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) acc[cb] = 0.0f;
        for (int k = 0; k < a.n; ++k) {
            const MsSrc& s = a.src[k];
            int r_lo, r_hi, q_lo, q_hi, c_lo, c_hi;
            row_span(s, y0, y1, r_lo, r_hi, q_lo, q_hi);
            col_span(s, x0, x1, c_lo, c_hi);
            const int nq = q_hi - q_lo + 1, nr = r_hi - r_lo + 1, nc = c_hi - c_lo + 1;
            if (nq > a.nrq || nr > a.nr1 || nc > a.nc1) {   // (uniform over the workgroup; the host sized these -- never taken)
                if (live)
                    for (int ch = 0; ch < NCH; ++ch)
                        (ch < a.Ch ? a.feat_out + ch * plane : a.logit_out + (ch - a.Ch) * plane)[pix] = __builtin_nanf("");
                return;
            }
            const size_t qplane = (size_t)s.hq * s.wq;
            // A: horizontal lerp of the quarter rows, once per needed stage-1 column
            for (int cb = 0; cb < nb; ++cb) {
                const int ch = ch0 + cb;
                const float* q = ch < a.Ch ? s.feat + ch * qplane : s.logit + (ch - a.Ch) * qplane;
                float* hb = hbuf + cb * a.nrq * a.nc1;
                for (int c = lane; c < nc; c += MAS_WAVE) {
                    const Tap t = make_tap(s.s1w, c_lo + c, s.wq);
                    for (int r = wave; r < nq; r += kWaves) {
                        const float* row = q + (size_t)(q_lo + r) * s.wq;
                        hb[r * a.nc1 + c] = t.l0 * row[t.i0] + t.l1 * row[t.i1];
                    }
                }
            }
            __syncthreads();
            // B: vertical combination into the stage-1 values the tile needs
            for (int r = wave; r < nr; r += kWaves) {
                const Tap t = make_tap(s.s1h, r_lo + r, s.hq);
                const int h0 = t.i0 - q_lo, h1 = t.i1 - q_lo;
                for (int cb = 0; cb < nb; ++cb) {
                    const float* hb = hbuf + cb * a.nrq * a.nc1;
                    float* sb = sbuf + (cb * a.nr1 + r) * a.nc1;
                    for (int c = lane; c < nc; c += MAS_WAVE) sb[c] = t.l0 * hb[h0 * a.nc1 + c] + t.l1 * hb[h1 * a.nc1 + c];
                }
            }
            __syncthreads();
            // C: stage 2 for this thread's pixel (flipped sources: taps in flipped coordinates, column j read as Ws-1-j)
            const Tap ty = make_tap(s.s2h, cy, s.hs), tx = make_tap(s.s2w, cx, s.ws);
            const int r0 = ty.i0 - r_lo, r1 = ty.i1 - r_lo;
            const int c0 = (s.flip ? s.ws - 1 - tx.i0 : tx.i0) - c_lo, c1 = (s.flip ? s.ws - 1 - tx.i1 : tx.i1) - c_lo;
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb) {
                if (cb < nb) {
                    const float* sb = sbuf + cb * a.nr1 * a.nc1;
                    const float v = ty.l0 * (tx.l0 * sb[r0 * a.nc1 + c0] + tx.l1 * sb[r0 * a.nc1 + c1]) +
                                    ty.l1 * (tx.l0 * sb[r1 * a.nc1 + c0] + tx.l1 * sb[r1 * a.nc1 + c1]);
                    acc[cb] = k == 0 ? v : acc[cb] + v;
                }
            }
            // (no barrier here: the next A writes hbuf, which every thread finished reading before the barrier above; the next B
            // writes sbuf only after the barrier that follows the next A, which every thread reaches after its C)
        }
        const float fn = (float)a.n;
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
            const int ch = ch0 + cb;
            if (cb < nb && live) {
                const float m = acc[cb] / fn;
                if (ch < a.Ch) {
                    const float m2 = m * m;
                    ss = ss + m2;
                    a.feat_out[ch * plane + pix] = m;
                } else {
                    a.logit_out[(ch - a.Ch) * plane + pix] = m;
                }
            }
        }
    }
    if (!live) return;
    float d = sqrtf(ss);
    d = d < 1e-12f ? 1e-12f : d;
    for (int ch = 0; ch < a.Ch; ++ch) {
        float* p = a.feat_out + ch * plane + pix;
        *p = *p / d;
    }
}
}  // namespace

extern "C" int mas_ms_ensemble(const float* const* feats_q, const float* const* logits_q, const int32_t* geometry, int n, int Ch, int C, int H,
                               int W, float* feat_out, float* logit_out, void* stream) {
    if (!feats_q || !logits_q || !geometry || !feat_out || !logit_out) return MAS_ERR_NULL;
    if (n < 1 || n > MAS_MS_MAX_SOURCES) return MAS_ERR_RANGE;
    if (Ch < 1 || C < 1 || H < 1 || W < 1 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    MsArgs a;
    a.feat_out = feat_out;
    a.logit_out = logit_out;
    a.n = n, a.Ch = Ch, a.C = C, a.H = H, a.W = W;
    for (int k = 0; k < MAS_MS_MAX_SOURCES; ++k) a.src[k] = MsSrc{};
    for (int k = 0; k < n; ++k) {
        const int32_t* g = geometry + 5 * k;
        MsSrc& s = a.src[k];
        if (!feats_q[k] || !logits_q[k]) return MAS_ERR_NULL;
        s.feat = feats_q[k], s.logit = logits_q[k];
        s.hq = g[0], s.wq = g[1], s.hs = g[2], s.ws = g[3], s.flip = g[4] != 0;
        // stage 1 is an upsampling (the network's x4); the scaled picture is not empty
        if (s.hq < 1 || s.wq < 1 || s.hs < 1 || s.ws < 1 || s.hq > s.hs || s.wq > s.ws) return MAS_ERR_SHAPE;
        s.s1h = (float)s.hq / (float)s.hs, s.s1w = (float)s.wq / (float)s.ws;
        s.s2h = (float)s.hs / (float)H, s.s2w = (float)s.ws / (float)W;
    }
    // LDS extents: the exact maxima over tiles and sources (same tap arithmetic as the kernel)
    int nrq = 1, nr1 = 1, nc1 = 1;
    for (int k = 0; k < n; ++k) {
        const MsSrc& s = a.src[k];
        for (int y0 = 0; y0 < H; y0 += kTH) {
            int r_lo, r_hi, q_lo, q_hi;
            row_span(s, y0, (y0 + kTH < H ? y0 + kTH : H) - 1, r_lo, r_hi, q_lo, q_hi);
            nr1 = r_hi - r_lo + 1 > nr1 ? r_hi - r_lo + 1 : nr1;
            nrq = q_hi - q_lo + 1 > nrq ? q_hi - q_lo + 1 : nrq;
        }
        for (int x0 = 0; x0 < W; x0 += kTW) {
            int c_lo, c_hi;
            col_span(s, x0, (x0 + kTW < W ? x0 + kTW : W) - 1, c_lo, c_hi);
            nc1 = c_hi - c_lo + 1 > nc1 ? c_hi - c_lo + 1 : nc1;
        }
    }
    const size_t lds = sizeof(float) * kCB * (size_t)(nrq + nr1) * nc1;
    if (lds > kMaxLds) return MAS_ERR_RANGE;         // a stage-2 downsample far beyond the 1.5 of the VOC factors
    a.nrq = nrq, a.nr1 = nr1, a.nc1 = nc1;
    hipLaunchKernelGGL(k_ms_ensemble, dim3((unsigned)((W + kTW - 1) / kTW), (unsigned)((H + kTH - 1) / kTH)), dim3(kThreads), lds,
                       static_cast<hipStream_t>(stream), a);
    return mas_launch_status();
}
