// upsample_tap.h -- the bilinear tap of k_upsample_fwd (upsample.hip) for kernels that upsample quarter-resolution maps in registers
// (naive_plbl.hip, lowres_iou.hip) or in LDS (ms_tile.h), the host computation of a tile's quarter-resolution footprint, and the
// arg-max rule of the label kernels (naive_plbl.hip, ms_naive.hip).  upsample.hip itself includes it: one copy of the arithmetic every
// bit-exactness claim of this family rests on.
//
// Tap (F.interpolate, bilinear, align_corners=False): s = max(scale * (o + 0.5) - 0.5, 0), i0 = (int)s, i1 = i0 + (i0 < n_in - 1),
// l1 = s - i0, l0 = 1 - l1, with scale = (float)n_in / (float)n_out computed on the host.  A value is then
//   y = l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11)
// each operation rounded to float32 (the units that include this build with -ffp-contract=off).
#pragma once

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

// torch.max over the channels, walked in channel order from best = channel 0's value, idx = 0: the first maximum wins; a NaN replaces
// a number and is never replaced.
__device__ __forceinline__ void arg_update(float v, int c, float& best, int& idx) {
    if (best != best) return;
    if (v > best || v != v) {
        best = v;
        idx = c;
    }
}

// Extents of the quarter-resolution footprint of a tile_h x tile_w output tile: the exact maxima over the tiles of an H x W output of
// the rows (*nrq) and columns (*ncq) one tile reads, with the kernels' tap arithmetic.  At least 1; for an upsampling
// nrq <= tile_h + 1 and ncq <= tile_w + 1.
static inline void tile_footprint(float sh, float sw, int h, int w, int H, int W, int tile_h, int tile_w, int* nrq, int* ncq) {
    int r = 1, c = 1;
    for (int y0 = 0; y0 < H; y0 += tile_h) {
        const int y1 = (y0 + tile_h < H ? y0 + tile_h : H) - 1;
        const int v = make_tap(sh, y1, h).i1 - make_tap(sh, y0, h).i0 + 1;
        r = v > r ? v : r;
    }
    for (int x0 = 0; x0 < W; x0 += tile_w) {
        const int x1 = (x0 + tile_w < W ? x0 + tile_w : W) - 1;
        const int v = make_tap(sw, x1, w).i1 - make_tap(sw, x0, w).i0 + 1;
        c = v > c ? v : c;
    }
    *nrq = r;
    *ncq = c;
}
