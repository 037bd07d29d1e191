/*
 * online_plbl.h -- the ARITHMETIC SPECIFICATION of the online local-prototype pseudo labels and of the cross entropy on them.
 *
 * Included by online_plbl.hip only, where the kernels (device) and mas_online_plbl_reference (a host loop) both go through it, so the two
 * give the same bits.  Correctly rounded add, multiply, divide and mas_fmaf, mas_expf_np, mas_logf only; compile with -ffp-contract=off.
 *
 *   tap       a pixel (y, x) of the H x W picture reads the four quarter-resolution elements of make_tap (upsample_tap.h) in both axes;
 *             a value is  l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11)  -- the arithmetic of mas_upsample_bilinear_fwd and of the
 *             quarter-resolution loss scans (losses.hip: load_logits).
 *   softmax   m = max_c z_c ; M = m*invT ; e_c = exp_np(fma(z_c, invT, -M)) ; sum = ((e_0+e_1)+e_2)... ; p_c = e_c * (1/sum)
 *             -- the operation order of mas_softmax_regs (common.h), so p_c equals the probability the group scan packs into its table.
 *   sim       sim(pixel, prototype) = fma chain over the channels k = 0.. from 0.0f of  f_k(prototype) * f_k(pixel), both interpolated.
 *   label     candidates c in Y (ascending); the first one is taken, a later one replaces it on sim > best.
 *   ce        -log(max(p_label, FLT_MIN))   (a probability below the smallest normal float is held there, as the scans' temperature CE)
 *   term      mode UNWEIGHTED: ce;  WEIGHTED: weight * ce;  THRESHOLD: ((th < weight) ? 1 : 0) * ce.  counted: UNWEIGHTED always, else
 *             term != 0.0f.  A term below zero (the rounding of mas_logf next to p = 1) is counted and adds 0 (mas_fix).
 *   gradient  k = ((grad / (float)count) * invT) * wgt ;  d_c = k * (p_c - [c == label]) ;  every tap adds
 *             round_to_nearest_even(d_c * (ly * lx) * 2^MAS_GRAD_FRAC_BITS) to its element.
 */
#ifndef MULACTSEG_ONLINE_PLBL_H
#define MULACTSEG_ONLINE_PLBL_H

#include "../../include/mulactseg_hip.h"
#include "detmath.h"
#include "upsample_tap.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define MAS_OPL_UNROLL _Pragma("unroll")
#else
#define MAS_OPL_UNROLL
#endif

struct OplTap { int o00, o01, o10, o11; float l0h, l1h, l0w, l1w; };

MAS_HD OplTap mas_opl_tap(float sh, float sw, int y, int x, int h, int w) {
    const Tap ty = make_tap(sh, y, h), tx = make_tap(sw, x, w);
    OplTap t;
    t.o00 = ty.i0 * w + tx.i0; t.o01 = ty.i0 * w + tx.i1;
    t.o10 = ty.i1 * w + tx.i0; t.o11 = ty.i1 * w + tx.i1;
    t.l0h = ty.l0; t.l1h = ty.l1; t.l0w = tx.l0; t.l1w = tx.l1;
    return t;
}

/* the interpolated value of one quarter-resolution plane [h,w] */
MAS_HD float mas_opl_at(const float* q, const OplTap t) {
    return t.l0h * (t.l0w * q[t.o00] + t.l1w * q[t.o01]) + t.l1h * (t.l0w * q[t.o10] + t.l1w * q[t.o11]);
}

/* v[0..C) = the interpolated logits of the pixel, from planes `hw` floats apart; CT is the extent the loops are unrolled over */
template <int CT>
MAS_HD void mas_opl_logits(const float* zb, size_t hw, const OplTap t, int C, float (&v)[CT]) {
    MAS_OPL_UNROLL
    for (int c = 0; c < CT; ++c) v[c] = (c < C) ? mas_opl_at(zb + (size_t)c * hw, t) : 0.0f;
}

/* logits in, probabilities out */
template <int CT>
MAS_HD void mas_opl_softmax(float (&v)[CT], int C, float invT) {
    float m = v[0];
    MAS_OPL_UNROLL
    for (int c = 1; c < CT; ++c)
        if (c < C) m = (v[c] > m) ? v[c] : m;
    const float negM = -(m * invT);
    float sum = 0.0f;
    MAS_OPL_UNROLL
    for (int c = 0; c < CT; ++c) {
        if (c < C) {
            v[c] = mas_expf_np(mas_fmaf(v[c], invT, negM));
            sum = (c == 0) ? v[c] : (sum + v[c]);
        }
    }
    const float rinv = 1.0f / sum;
    MAS_OPL_UNROLL
    for (int c = 0; c < CT; ++c)
        if (c < C) v[c] = v[c] * rinv;
}

/* p[k] without a runtime index into the register array */
template <int CT>
MAS_HD float mas_opl_pick(const float (&p)[CT], int C, int k) {
    float r = 0.0f;
    MAS_OPL_UNROLL
    for (int c = 0; c < CT; ++c)
        if (c < C) r = (c == k) ? p[c] : r;
    return r;
}

/* the word of the (superpixel, class) table: probability bits above the complemented pixel index (a larger word = a larger
 * probability, then a LOWER pixel) -- pack_max of losses.hip */
MAS_HD uint64_t mas_opl_pack(float p, uint32_t pix) { return ((uint64_t)mas_f2u(p) << 32) | (uint64_t)(0xffffffffu - pix); }
MAS_HD uint32_t mas_opl_word_pixel(uint64_t w) { return 0xffffffffu - (uint32_t)w; }

/* the weight the mode gives a labelled pixel */
MAS_HD float mas_opl_mode_weight(int mode, float weight, float th) {
    if (mode == MAS_LCE_WEIGHTED) return weight;
    if (mode == MAS_LCE_THRESHOLD) return (th < weight) ? 1.0f : 0.0f;
    return 1.0f;
}

MAS_HD float mas_opl_ce(float p_label) { return -mas_logf(p_label < 1.17549435e-38f ? 1.17549435e-38f : p_label); }

/* term of one labelled pixel; *counted = whether it enters the normaliser */
MAS_HD float mas_opl_term(int mode, float wgt, float ce, int* counted) {
    if (mode == MAS_LCE_UNWEIGHTED) { *counted = 1; return ce; }
    const float t = wgt * ce;
    *counted = (t != 0.0f) ? 1 : 0;
    return t;
}

/* acc = {sum, count} -> the loss value */
MAS_HD float mas_opl_value(uint64_t sum, uint64_t count, int flags) {
    if (count == 0) return (flags & MAS_LCE_EMPTY_NAN) ? mas_u2f(0x7fc00000u) : 0.0f;
    union { double d; uint64_t u; } s;
    s.u = (uint64_t)(1023 - MAS_LOSS_FRAC_BITS) << 52;
    return (float)(((double)sum * s.d) / (double)count);
}

/* signed fixed point (MAS_GRAD_FRAC_BITS) of one gradient contribution, round to nearest even -- grad_fix of losses.hip */
MAS_HD long long mas_opl_grad_fix(float t) {
    union { double d; uint64_t u; } s;
    s.u = (uint64_t)(1023 + MAS_GRAD_FRAC_BITS) << 52;
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2ll_rn((double)t * s.d);
#else
    return __builtin_llrint((double)t * s.d);
#endif
}

#endif /* MULACTSEG_ONLINE_PLBL_H */
