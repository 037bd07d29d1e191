// ms_tile.h -- the two-stage tile of the multi-scale + flip kernels (k_ms_ensemble in ms_ensemble.hip, k_ms_naive in ms_naive.hip): one
// copy of the geometry, the LDS sizing and the per-(channel block, source) accumulation, so the mean values of the two kernels are
// the same code and not two copies that agree.
//
// A source is a quarter-resolution map [*, hq, wq] of the network on the picture scaled to (hs, ws) and possibly flipped.  Its value at
// an output pixel is stage 1 (quarter -> scaled, the tap and expression of k_upsample_fwd: upsample_tap.h), the flip, and stage 2
// (scaled -> original (H, W), the same tap and expression over the stage-1 values); the callers' header comments number these steps.
//
// Shape: a workgroup owns an 8 x 32 output tile, one pixel per thread, and walks the channels in blocks of kCB, sources innermost.  Per
// (block, source), ms_tile_add:
//   A. every (quarter row, stage-1 column) position the tile needs, lerped horizontally for the block's channels into LDS.  A thread
//      issues the loads of all its positions and channels of a round first and stores to LDS after, so a step waits on one round of
//      load latency rather than on one per value;
//   B. the stage-1 rows the tile needs, combined vertically from A, into LDS (the stage-1 values, in k_upsample_fwd's operation order);
//   C. stage 2 for the thread's pixel from B, added to the caller's accumulators in registers.
// The scaled-size values live in LDS only.  The LDS extents are the exact maxima over tiles and sources, computed on the host with the
// kernel's tap arithmetic (ms_tile_extents).
#pragma once
#include "common.h"
#include "upsample_tap.h"

namespace {
constexpr int kTH = 8, kTW = 32;           // output tile
constexpr int kThreads = kTH * kTW;        // one output pixel per thread
constexpr int kCB = 8;                     // channels per LDS block
constexpr int kPos = 2;                    // (quarter row, stage-1 column) positions per thread and load round in A
constexpr int kWaves = kThreads / MAS_WAVE;
constexpr size_t kMaxLds = 64 * 1024;      // of one workgroup: the dynamic buffers and a kernel's static LDS together

struct MsGeom {
    int hq, wq, hs, ws, flip;
    float s1h, s1w, s2h, s2w;     // stage-1 (quarter -> scaled) and stage-2 (scaled -> original) scales
};

struct MsTile {                   // the geometry part of a kernel's arguments
    MsGeom src[MAS_MS_MAX_SOURCES];
    int n, H, W;
    int nrq, nr1, nc1;            // LDS extents: quarter rows, stage-1 rows, stage-1 columns of one tile
};

// stage-1 row range [r_lo, r_hi] and quarter row range [q_lo, q_hi] of output rows y0..y1 (unflipped axis)
__host__ __device__ __forceinline__ void row_span(const MsGeom& s, int y0, int y1, int& r_lo, int& r_hi, int& q_lo, int& q_hi) {
    r_lo = make_tap(s.s2h, y0, s.hs).i0;
    r_hi = make_tap(s.s2h, y1, s.hs).i1;
    q_lo = make_tap(s.s1h, r_lo, s.hq).i0;
    q_hi = make_tap(s.s1h, r_hi, s.hq).i1;
}

// stage-1 column range [c_lo, c_hi] (unflipped stage-1 coordinates) of output columns x0..x1
__host__ __device__ __forceinline__ void col_span(const MsGeom& s, int x0, int x1, int& c_lo, int& c_hi) {
    const int b_lo = make_tap(s.s2w, x0, s.ws).i0, b_hi = make_tap(s.s2w, x1, s.ws).i1;
    c_lo = s.flip ? s.ws - 1 - b_hi : b_lo;
    c_hi = s.flip ? s.ws - 1 - b_lo : b_hi;
}

// Host: the n sources of an H x W picture from the caller's [n,5] table (hq, wq, hs, ws, flip).  Stage 1 is an upsampling (the
// network's x4) and the scaled picture is not empty, else MAS_ERR_SHAPE.  The caller has checked n, H and W.
inline int ms_tile_sources(MsTile& t, const int32_t* geometry, int n, int H, int W) {
    t = MsTile{};
    t.n = n, t.H = H, t.W = W;
    for (int k = 0; k < n; ++k) {
        const int32_t* g = geometry + 5 * k;
        MsGeom& s = t.src[k];
        s.hq = g[0], s.wq = g[1], s.hs = g[2], s.ws = g[3], s.flip = g[4] != 0;
        if (s.hq < 1 || s.wq < 1 || s.hs < 1 || s.ws < 1 || s.hq > s.hs || s.wq > s.ws) return MAS_ERR_SHAPE;
        s.s1h = (float)s.hq / (float)s.hs, s.s1w = (float)s.wq / (float)s.ws;
        s.s2h = (float)s.hs / (float)H, s.s2w = (float)s.ws / (float)W;
    }
    return 0;
}

// Host: sets the LDS extents of one tile, the exact maxima over tiles and sources, and returns the dynamic LDS bytes of the launch.
// The caller compares them (plus its static LDS) with kMaxLds: a stage-2 downsample far beyond the 1.5 of the VOC factors does not fit
// (x2, the largest factor of an evaluation, does).
inline size_t ms_tile_extents(MsTile& t) {
    int nrq = 1, nr1 = 1, nc1 = 1;
    for (int k = 0; k < t.n; ++k) {
        const MsGeom& s = t.src[k];
        for (int y0 = 0; y0 < t.H; y0 += kTH) {
            int r_lo, r_hi, q_lo, q_hi;
            row_span(s, y0, (y0 + kTH < t.H ? y0 + kTH : t.H) - 1, r_lo, r_hi, q_lo, q_hi);
            nr1 = r_hi - r_lo + 1 > nr1 ? r_hi - r_lo + 1 : nr1;
            nrq = q_hi - q_lo + 1 > nrq ? q_hi - q_lo + 1 : nrq;
        }
        for (int x0 = 0; x0 < t.W; x0 += kTW) {
            int c_lo, c_hi;
            col_span(s, x0, (x0 + kTW < t.W ? x0 + kTW : t.W) - 1, c_lo, c_hi);
            nc1 = c_hi - c_lo + 1 > nc1 ? c_hi - c_lo + 1 : nc1;
        }
    }
    t.nrq = nrq, t.nr1 = nr1, t.nc1 = nc1;
    return sizeof(float) * kCB * (size_t)(nrq + nr1) * nc1;
}

inline dim3 ms_tile_grid(const MsTile& t) { return dim3((unsigned)((t.W + kTW - 1) / kTW), (unsigned)((t.H + kTH - 1) / kTH)); }

struct MsPixel {                  // a thread's place in the grid of ms_tile_grid
    int y0, x0, y1, x1;           // the workgroup's tile, clipped to the picture
    int cy, cx;                   // the thread's pixel; outside the picture: the tile's last one (for its taps)
    bool live;                    // the pixel lies inside the picture
};

__device__ __forceinline__ MsPixel ms_tile_pixel(const MsTile& t) {
    MsPixel p;
    p.y0 = blockIdx.y * kTH, p.x0 = blockIdx.x * kTW;
    p.y1 = min(p.y0 + kTH, t.H) - 1, p.x1 = min(p.x0 + kTW, t.W) - 1;
    const int py = p.y0 + threadIdx.x / kTW, px = p.x0 + threadIdx.x % kTW;
    p.live = py < t.H && px < t.W;
    p.cy = min(py, p.y1), p.cx = min(px, p.x1);
    return p;
}

// Device: source k's values of the `nb` channels of one block at the thread's pixel, into acc (k == 0) or added to it.  slot(cb) is the
// [hq, wq] plane of the block's channel slot cb in source k.  lds: the launch's dynamic LDS, kCB * (nrq + nr1) * nc1 floats.  Every
// thread of the workgroup calls it (two barriers).  false: the extents do not hold this tile (uniform over the workgroup; the host
// sized them -- never taken).
template <class Slot>
__device__ __forceinline__ bool ms_tile_add(const MsTile& t, int k, const MsPixel& p, int nb, Slot slot, float* lds, float (&acc)[kCB]) {
    float* hbuf = lds;                                   // [kCB][nrq][nc1]: quarter rows lerped horizontally
    float* sbuf = lds + kCB * t.nrq * t.nc1;             // [kCB][nr1][nc1]: stage-1 values
    const int tid = threadIdx.x, lane = tid & (MAS_WAVE - 1), wave = tid / MAS_WAVE;
    const MsGeom& s = t.src[k];
    int r_lo, r_hi, q_lo, q_hi, c_lo, c_hi;
    row_span(s, p.y0, p.y1, r_lo, r_hi, q_lo, q_hi);
    col_span(s, p.x0, p.x1, c_lo, c_hi);
    const int nq = q_hi - q_lo + 1, nr = r_hi - r_lo + 1, nc = c_hi - c_lo + 1;
    if (nq > t.nrq || nr > t.nr1 || nc > t.nc1) return false;
    // A: horizontal lerp of the quarter rows, once per needed stage-1 column; loads of a round first, LDS stores after
    const int npos = nq * nc;
    for (int p0 = 0; p0 < npos; p0 += kPos * kThreads) {
        float v0[kPos][kCB], v1[kPos][kCB], w0[kPos], w1[kPos];
        int dst[kPos];
#pragma unroll
        for (int u = 0; u < kPos; ++u) {
            const int q = p0 + u * kThreads + tid;
            dst[u] = -1;
            w0[u] = w1[u] = 0.0f;
            if (q < npos) {
                const int r = q / nc, c = q - r * nc;
                const Tap tc = make_tap(s.s1w, c_lo + c, s.wq);
                const size_t row = (size_t)(q_lo + r) * s.wq;
                dst[u] = r * t.nc1 + c;
                w0[u] = tc.l0, w1[u] = tc.l1;
#pragma unroll
                for (int cb = 0; cb < kCB; ++cb) {
                    if (cb < nb) {
                        v0[u][cb] = slot(cb)[row + tc.i0];
                        v1[u][cb] = slot(cb)[row + tc.i1];
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kPos; ++u) {
            if (dst[u] >= 0) {
#pragma unroll
                for (int cb = 0; cb < kCB; ++cb)
                    if (cb < nb) hbuf[cb * t.nrq * t.nc1 + dst[u]] = w0[u] * v0[u][cb] + w1[u] * v1[u][cb];
            }
        }
    }
    __syncthreads();
    // B: vertical combination into the stage-1 values the tile needs
    for (int r = wave; r < nr; r += kWaves) {
        const Tap tr = make_tap(s.s1h, r_lo + r, s.hq);
        const int h0 = tr.i0 - q_lo, h1 = tr.i1 - q_lo;
        for (int cb = 0; cb < nb; ++cb) {
            const float* hb = hbuf + cb * t.nrq * t.nc1;
            float* sb = sbuf + (cb * t.nr1 + r) * t.nc1;
            for (int c = lane; c < nc; c += MAS_WAVE) sb[c] = tr.l0 * hb[h0 * t.nc1 + c] + tr.l1 * hb[h1 * t.nc1 + c];
        }
    }
    __syncthreads();
    // C: stage 2 for this thread's pixel (flipped sources: taps in flipped coordinates, column j read as Ws-1-j)
    const Tap ty = make_tap(s.s2h, p.cy, s.hs), tx = make_tap(s.s2w, p.cx, s.ws);
    const int r0 = ty.i0 - r_lo, r1 = ty.i1 - r_lo;
    const int c0 = (s.flip ? s.ws - 1 - tx.i0 : tx.i0) - c_lo, c1 = (s.flip ? s.ws - 1 - tx.i1 : tx.i1) - c_lo;
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb) {
        if (cb < nb) {
            const float* sb = sbuf + cb * t.nr1 * t.nc1;
            const float v = ty.l0 * (tx.l0 * sb[r0 * t.nc1 + c0] + tx.l1 * sb[r0 * t.nc1 + c1]) +
                            ty.l1 * (tx.l0 * sb[r1 * t.nc1 + c0] + tx.l1 * sb[r1 * t.nc1 + c1]);
            acc[cb] = k == 0 ? v : acc[cb] + v;
        }
    }
    // (no barrier here: the next A writes hbuf, which every thread finished reading before the barrier above; the next B writes sbuf
    // only after the barrier that follows the next A, which every thread reaches after its C)
    return true;
}
}  // namespace
