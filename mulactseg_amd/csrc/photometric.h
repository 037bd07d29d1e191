/*
 * photometric.h -- the ARITHMETIC SPECIFICATION of the photometric augmentation: torchvision's ColorJitter (brightness, contrast,
 * saturation, hue in a drawn order) and RandomGrayscale as Pillow executes them on 8-bit RGB (ImageEnhance -> Image.blend,
 * convert('L'), convert('HSV') / convert('RGB'); src/libImaging/Blend.c, Convert.c), restated per pixel.  Like uncertainty.h the header
 * compiles as device code (hipcc, gfx950) and as plain host C++, and is used by the kernels (photometric.hip) and by the host loop
 * (mas_photometric_reference), so the two give the same bits.  Pinned to Pillow 12.2.0 by tests/test_photometric_cpu.py.
 *
 * Every f32 blend is a separate multiply and add: NO fused multiply-add may be formed (contraction is switched off below, and the
 * units are compiled with -ffp-contract=off).  Doubles are IEEE add, multiply, divide, floor and round only.
 *
 *   L (grey)      (19595 r + 38470 g + 7471 b + 0x8000) >> 16
 *   blend(x,d,a)  t = f32(d) + a * f32(x - d)  (x - d an int);  0 <= a <= 1: (int)t;  otherwise 0 for t <= 0, 255 for t >= 255, (int)t
 *   brightness    d = 0;   saturation  d = L of the pixel;   contrast  d = (int)(sum_L / n + 0.5) in double, sum_L over the whole crop
 *   hue           RGB -> HSV, h += shift (mod 256), HSV -> RGB;  shift = (int)(double(hue) * 255.0) & 0xFF
 *   grayscale     r = g = b = L
 *   normalise     ((float)u8 / 255.0f - mean) / std
 */
#ifndef MULACTSEG_PHOTOMETRIC_H
#define MULACTSEG_PHOTOMETRIC_H

#include "detmath.h"

#pragma clang fp contract(off)

#define MAS_PM_BRIGHTNESS 0
#define MAS_PM_CONTRAST 1
#define MAS_PM_SATURATION 2
#define MAS_PM_HUE 3
#define MAS_PM_OPS 4

/* One sample's chain: ops are applied in `order`; an op whose bit is clear in `present` is skipped. */
struct mas_pm_chain {
    int order[MAS_PM_OPS];
    float factor[MAS_PM_OPS];      /* indexed by op (not by position) */
    int present;                   /* bit k: op k is in the chain */
    int shift;                     /* the hue shift of h, 0..255 */
    int grey;
};

MAS_HD int mas_pm_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

MAS_HD int mas_pm_hue_shift(float hue) { return (int)((double)hue * 255.0) & 0xFF; }

MAS_HD int mas_pm_grey(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

MAS_HD int mas_pm_blend(int x, int d, float a) {
    const float prod = a * (float)(x - d);
    const float t = (float)d + prod;
    if (a >= 0.0f && a <= 1.0f) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

MAS_HD int mas_pm_contrast_mean(unsigned long long sum_l, unsigned long long n) { return (int)((double)sum_l / (double)n + 0.5); }

/* Convert.c: rgb2hsv_row */
MAS_HD void mas_pm_rgb2hsv(int r, int g, int b, int* uh, int* us, int* uv) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    *uv = maxc;
    if (minc == maxc) {
        *uh = 0;
        *us = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double w = (double)h / 6.0 + 1.0;          /* in [5/6, 11/6]: fmod(w, 1.0) == w - floor(w), exactly */
    h = (float)(w - __builtin_floor(w));
    *uh = mas_pm_clip8((int)((double)h * 255.0));
    *us = mas_pm_clip8((int)((double)s * 255.0));
}

/* Convert.c: hsv2rgb */
MAS_HD void mas_pm_hsv2rgb(int h, int s, int v, int* r, int* g, int* b) {
    if (s == 0) {
        *r = *g = *b = v;
        return;
    }
    const double hf = (double)h * 6.0 / 255.0;
    const double fl = __builtin_floor(hf);
    const int i = (int)fl;
    const float f = (float)(hf - fl);
    const float fs = (float)((double)s / 255.0);
    const double dv = (double)v;
    const int p = mas_pm_clip8((int)__builtin_round(dv * (1.0 - (double)fs)));
    const int q = mas_pm_clip8((int)__builtin_round(dv * (1.0 - (double)fs * (double)f)));
    const int t = mas_pm_clip8((int)__builtin_round(dv * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: *r = v; *g = t; *b = p; break;
        case 1: *r = q; *g = v; *b = p; break;
        case 2: *r = p; *g = v; *b = t; break;
        case 3: *r = p; *g = q; *b = v; break;
        case 4: *r = t; *g = p; *b = v; break;
        default: *r = v; *g = p; *b = q; break;
    }
}

/* one op on one pixel; `cmean` is the contrast degenerate value */
MAS_HD void mas_pm_op(int op, const mas_pm_chain* c, int cmean, int* r, int* g, int* b) {
    const float a = c->factor[op & 3];
    if (op == MAS_PM_BRIGHTNESS) {
        *r = mas_pm_blend(*r, 0, a); *g = mas_pm_blend(*g, 0, a); *b = mas_pm_blend(*b, 0, a);
    } else if (op == MAS_PM_CONTRAST) {
        *r = mas_pm_blend(*r, cmean, a); *g = mas_pm_blend(*g, cmean, a); *b = mas_pm_blend(*b, cmean, a);
    } else if (op == MAS_PM_SATURATION) {
        const int l = mas_pm_grey(*r, *g, *b);
        *r = mas_pm_blend(*r, l, a); *g = mas_pm_blend(*g, l, a); *b = mas_pm_blend(*b, l, a);
    } else {
        int h, s, v;
        mas_pm_rgb2hsv(*r, *g, *b, &h, &s, &v);
        mas_pm_hsv2rgb((h + c->shift) & 0xFF, s, v, r, g, b);
    }
}

/* position of contrast in the chain, MAS_PM_OPS when it is absent */
MAS_HD int mas_pm_contrast_pos(const mas_pm_chain* c) {
    if (!((c->present >> MAS_PM_CONTRAST) & 1)) return MAS_PM_OPS;
    for (int k = 0; k < MAS_PM_OPS; ++k)
        if (c->order[k] == MAS_PM_CONTRAST) return k;
    return MAS_PM_OPS;
}

/* the ops at positions [from, to) of the chain */
MAS_HD void mas_pm_apply(const mas_pm_chain* c, int from, int to, int cmean, int* r, int* g, int* b) {
    for (int k = from; k < to; ++k) {
        const int op = c->order[k];
        if ((c->present >> op) & 1) mas_pm_op(op, c, cmean, r, g, b);
    }
}

/* the whole chain and grayscale */
MAS_HD void mas_pm_pixel(const mas_pm_chain* c, int cmean, int* r, int* g, int* b) {
    mas_pm_apply(c, 0, MAS_PM_OPS, cmean, r, g, b);
    if (c->grey) *r = *g = *b = mas_pm_grey(*r, *g, *b);
}

MAS_HD float mas_pm_normalise(int v, float mean, float std) { return ((float)v / 255.0f - mean) / std; }

#endif /* MULACTSEG_PHOTOMETRIC_H */
