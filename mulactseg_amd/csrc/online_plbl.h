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
 *
 * The similarity-weighted forms (LocalsimWProtoCE, JointLocalProtoWeightingCE):
 *   sim weight   with MAS_OPL_WEIGHT_SIM the weight of a valid pixel is the chain value `best` of the chosen candidate, which may be
 *                negative; labels are unchanged.
 *   signed term  with MAS_LCE_SIGNED (mode WEIGHTED) the sum is two's complement: mas_fix(|term|) is added for term > 0 and subtracted
 *                for term < 0; value = (double)(int64)sum * 2^-MAS_LOSS_FRAC_BITS / count.  Counting and gradient are unchanged
 *                (k = scale * wgt carries the sign).
 *   live         a picture is live when it has at least one valid pixel.
 *   counted      mask set, id in [0, S), picture live.  (A masked pixel with an id outside [0, S) makes the reference raise an index
 *                error; here it is not counted.)
 *   soft weight  of a valid pixel, over its candidates c in Y (ascending): m = max sim_c ; e_c = exp_np(fma(sim_c, invtau, -(m*invtau))) ;
 *                sum = ((e_0+e_1)+...) ; w_c = e_c * (1/sum)  -- the operation order of mas_opl_softmax.
 *   soft term    p = softmax(up(zq) * invT).  Valid pixel: t = sum over c in Y ascending of w_c * (-log(p_c + 1e-8f)), added in f32 from
 *                0.0f; a counted pixel with one candidate: t = -log(p_c + 1e-8f); with none: t = 0.  acc[0] += mas_fix(t), acc[1] += 1.
 *   soft grad    q_c = p_c / (p_c + 1e-8f) ; A = sum over c in Y ascending of w_c * q_c (w = 1 for a one-candidate pixel) ;
 *                d_j = ((grad / (float)count) * invT) * (p_j * A - w_j * q_j), w_j = 0 off Y; through the taps as above.
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

/* what one counted term adds to the u64 sum: mas_fix(term) (0 for a negative term), or with `sgn` the two's complement of
 * mas_fix(|term|) for a negative one */
MAS_HD uint64_t mas_opl_fix_term(float term, int sgn) {
    if (!sgn) return mas_fix(term, MAS_LOSS_FRAC_BITS);
    const uint64_t q = mas_fix(mas_u2f(mas_f2u(term) & 0x7fffffffu), MAS_LOSS_FRAC_BITS);
    return (term < 0.0f) ? (uint64_t)0 - q : q;
}

/* acc = {sum, count} -> the loss value; with MAS_LCE_SIGNED the sum is read as two's complement */
MAS_HD float mas_opl_value(uint64_t sum, uint64_t count, int flags) {
    if (count == 0) return (flags & MAS_LCE_EMPTY_NAN) ? mas_u2f(0x7fc00000u) : 0.0f;
    union { double d; uint64_t u; } s;
    s.u = (uint64_t)(1023 - MAS_LOSS_FRAC_BITS) << 52;
    const double v = (flags & MAS_LCE_SIGNED) ? (double)(int64_t)sum : (double)sum;
    return (float)((v * s.d) / (double)count);
}

/* ---- soft targets from the prototype similarities ---- */
#define MAS_OPL_EPS 1e-8f

/* the raw similarities of one pixel, `stride` floats apart at the classes of Y, become its soft weights in place */
MAS_HD void mas_opl_soft_normalise(float* sw, size_t stride, uint32_t Y, float invtau) {
    if (!Y) return;
    float m = sw[(size_t)__builtin_ctz(Y) * stride];
    for (uint32_t y = Y & (Y - 1u); y; y &= y - 1u) {
        const float v = sw[(size_t)__builtin_ctz(y) * stride];
        m = (v > m) ? v : m;
    }
    const float negM = -(m * invtau);
    float sum = 0.0f;
    for (uint32_t y = Y; y; y &= y - 1u) {
        float* p = sw + (size_t)__builtin_ctz(y) * stride;
        const float e = mas_expf_np(mas_fmaf(*p, invtau, negM));
        *p = e;
        sum = (y == Y) ? e : (sum + e);
    }
    const float rinv = 1.0f / sum;
    for (uint32_t y = Y; y; y &= y - 1u) {
        float* p = sw + (size_t)__builtin_ctz(y) * stride;
        *p = *p * rinv;
    }
}

/* the candidates of a counted pixel within the C classes, and whether it reads soft weights (a valid pixel) */
MAS_HD uint32_t mas_opl_cands(uint32_t Y, int C, int* multi) {
    *multi = __builtin_popcount(Y) > 1;
    return C < 32 ? (Y & ((1u << C) - 1u)) : Y;
}

/* soft CE term of a counted pixel with probabilities p: its candidates Yc, soft weights `stride` apart at sw (read when multi).
 * *A = sum w_c * q_c for the gradient. */
template <int CT>
MAS_HD float mas_opl_soft_term(const float (&p)[CT], int C, uint32_t Yc, int multi, const float* sw, size_t stride, float* A) {
    float t = 0.0f, a = 0.0f;
    MAS_OPL_UNROLL
    for (int c = 0; c < CT; ++c) {
        if (c < C && ((Yc >> c) & 1u)) {
            const float w = multi ? sw[(size_t)c * stride] : 1.0f;
            const float pe = p[c] + MAS_OPL_EPS;
            t = t + w * (-mas_logf(pe));
            a = a + w * (p[c] / pe);
        }
    }
    *A = a;
    return t;
}

/* d_j / k of the soft CE: p_j * A - w_j * q_j */
MAS_HD float mas_opl_soft_dir(float pj, float A, int in_y, float wj) {
    return in_y ? (pj * A - wj * (pj / (pj + MAS_OPL_EPS))) : (pj * A);
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
