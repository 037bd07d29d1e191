// ms_ensemble.hip -- the multi-scale + flip ensemble of the VOC stage-2 generator in one launch.
//
// Reference: trainer/eval_save_cosplbl_prop_includeonehot_voc_ms.py:56-79.  Every source k (a scaled, possibly flipped copy of the
// picture) went through feat_forward: quarter-resolution features / logits upsampled x4 bilinearly to the scaled size (Hs, Ws),
// flipped back, F.interpolate'd to the original (H, W), averaged, the features re-normalised over the channels.  Materialised, that is
// 256 channels at every scaled size and again at the original size per source (~11 GB of traffic for a 500x375 picture).  Here the
// quarter-resolution maps are read once per output tile and the scaled-size values live in LDS only.
//
// Arithmetic (normative; tests/ms_ensemble_restated.py restates it in numpy).  tap(scale, o, n):
//   s = max(0, scale*(o+0.5)-0.5), i0 = (int)s, i1 = i0 + (i0 < n-1), l1 = s - i0, l0 = 1 - l1       (upsample_tap.h, ATen's
//   area_pixel_compute_source_index); scale = (float)in / (float)out, computed on the host.
//   1. stage 1, quarter (hq, wq) -> scaled (Hs, Ws):   S(r,c) = l0h*(l0w*q[i0h][i0w] + l1w*q[i0h][i1w]) + l1h*(l0w*q[i1h][i0w] + l1w*q[i1h][i1w])
//      -- the expression of k_upsample_fwd, so S equals mas_upsample_bilinear_fwd on the materialised tensor bit for bit;
//   2. flip (flipped sources): stage-2 taps are computed in flipped coordinates, stage-1 column j is read as column Ws-1-j;
//   3. stage 2, scaled -> original (H, W), the same tap and expression over S (a downsample for factors > 1);
//   4. mean: v_0 + v_1 + ... + v_{n-1} in source order, then / (float)n;
//   5. features only: ss = sum over channels in channel order of m*m (multiply, then add -- no fma under -ffp-contract=off),
//      d = max(sqrtf(ss), 1e-12) (correctly rounded sqrt), out = m / d.
//
// Shape: the two-stage tile of ms_tile.h (an 8 x 32 output tile per workgroup, channel blocks of kCB, sources innermost); a channel
// block may hold feature and logit channels.  The mean features are written once, the per-pixel sum of squares stays in a register,
// and the normalisation re-reads the thread's own freshly written lines (L2 / Infinity Cache) -- no full-picture round trip.
#include "ms_tile.h"

namespace {
struct MsArgs {
    MsTile t;
    const float* feat[MAS_MS_MAX_SOURCES];    // [Ch, hq, wq] per source
    const float* logit[MAS_MS_MAX_SOURCES];   // [C, hq, wq] per source
    float* feat_out;              // [Ch, H, W]
    float* logit_out;             // [C, H, W]
    int Ch, C;
};

// grid: ms_tile_grid; dynamic LDS: ms_tile_extents
__global__ __launch_bounds__(kThreads) void k_ms_ensemble(const MsArgs a) {
    extern __shared__ float lds[];
    const int NCH = a.Ch + a.C;
    const MsPixel p = ms_tile_pixel(a.t);
    const size_t plane = (size_t)a.t.H * a.t.W, pix = (size_t)p.cy * a.t.W + p.cx;
    float ss = 0.0f;
    for (int ch0 = 0; ch0 < NCH; ch0 += kCB) {
        const int nb = min(kCB, NCH - ch0);
        float acc[kCB];
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) acc[cb] = 0.0f;
        for (int k = 0; k < a.t.n; ++k) {
            const size_t qplane = (size_t)a.t.src[k].hq * a.t.src[k].wq;
            const float *fq = a.feat[k], *zq = a.logit[k];
            const int Ch = a.Ch;
            const auto slot = [=](int cb) { return ch0 + cb < Ch ? fq + (ch0 + cb) * qplane : zq + (ch0 + cb - Ch) * qplane; };
            if (!ms_tile_add(a.t, k, p, nb, slot, lds, acc)) {
                if (p.live)
                    for (int ch = 0; ch < NCH; ++ch)
                        (ch < a.Ch ? a.feat_out + ch * plane : a.logit_out + (ch - a.Ch) * plane)[pix] = __builtin_nanf("");
                return;
            }
        }
        const float fn = (float)a.t.n;
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
            const int ch = ch0 + cb;
            if (cb < nb && p.live) {
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
    if (!p.live) return;
    float d = sqrtf(ss);
    d = d < 1e-12f ? 1e-12f : d;
    for (int ch = 0; ch < a.Ch; ++ch) {
        float* q = a.feat_out + ch * plane + pix;
        *q = *q / d;
    }
}
}  // namespace

extern "C" int mas_ms_ensemble(const float* const* feats_q, const float* const* logits_q, const int32_t* geometry, int n, int Ch, int C, int H,
                               int W, float* feat_out, float* logit_out, void* stream) {
    if (!feats_q || !logits_q || !geometry || !feat_out || !logit_out) return MAS_ERR_NULL;
    if (n < 1 || n > MAS_MS_MAX_SOURCES) return MAS_ERR_RANGE;
    if (Ch < 1 || C < 1 || H < 1 || W < 1 || H > 65535 * kTH) return MAS_ERR_SHAPE;
    MsArgs a = {};
    a.feat_out = feat_out;
    a.logit_out = logit_out;
    a.Ch = Ch, a.C = C;
    for (int k = 0; k < n; ++k) {
        if (!feats_q[k] || !logits_q[k]) return MAS_ERR_NULL;
        a.feat[k] = feats_q[k], a.logit[k] = logits_q[k];
    }
    if (int st = ms_tile_sources(a.t, geometry, n, H, W)) return st;
    const size_t lds = ms_tile_extents(a.t);
    if (lds > kMaxLds) return MAS_ERR_RANGE;
    hipLaunchKernelGGL(k_ms_ensemble, ms_tile_grid(a.t), dim3(kThreads), lds, static_cast<hipStream_t>(stream), a);
    return mas_launch_status();
}
