/*
 * uncertainty.h -- the ARITHMETIC SPECIFICATION of the per-pixel acquisition measures.
 *
 * One pixel's C logits go in, one uncertainty value u in (0, 1.0000001] comes out, together with what the round's other
 * accumulators need: the arg-max class, the un-normalised probabilities e_c and the class-prior scale R.  Like detmath.h the header
 * compiles as device code (hipcc, gfx950) and as plain host C; it uses mas_fmaf, mas_expf_np, mas_logf and correctly rounded add,
 * multiply and divide only, so the kernel (uncertainty.hip: k_uncertainty) and the host loop (mas_uncertainty_reference) give the
 * same bits.  Compile with -ffp-contract=off.
 *
 * Set-up, in the operation order of the class-prior arithmetic of the headline scan (common.h: mas_softmax_quad with the maximum known;
 * oracle/exact.c: softmax_row) -- prob_sum is therefore bit-identical to mas_single_pass_accum's for every measure:
 *   top-2 scan in channel order from (b1, b2, arg) = (-inf, -inf, 0): v > b1 -> (b2, b1, arg) = (b1, v, c); else v > b2 -> b2 = v
 *     (strict '>': the first maximum is the arg-max; b2 is the second-largest logit, equal to b1 on a tie)
 *   negM = -(b1 * invT);  t_c = fma(z_c, invT, negM);  e_c = mas_expf_np(t_c)
 *   sum  = ((e_0 + e_1) + e_2) + ...;  rinv = 1 / sum = p1;  R = rinv * 2^23          (mas_probq(e_c, R) is the class-prior quantum)
 *
 * Measures (the three new ones are clamped to [0, 1]; each then adds 1e-8f, as BvSB does: a region that is present never scores
 * exactly 0 before the ban):
 *   bvsb              mas_bvsb(b1, b2, invT)                                            p2 / p1 (detmath.h, unchanged)
 *   margin            1 - (1 - e_2) * rinv,  e_2 = mas_expf_np(fma(b2, invT, negM))     1 - (p1 - p2)
 *   least_confidence  1 - rinv                                                          1 - p1
 *   entropy           (mas_logf(sum) - dot * rinv) * inv_log_c,                         -sum_c p_c ln p_c / ln C
 *                     dot = fma(e_c, t_c, dot) in channel order from 0,  inv_log_c = 1 / mas_logf((float)C)
 * The clamp is needed by all three: t of the arg-max is fma(b1, invT, -(b1 * invT)), the rounding error of the product and not 0,
 * so its e is 1 -+ 1e-7, a confident pixel's sum may fall just below 1 and rinv just above it.  e_c * t_c is 0, a normal float or
 * (for the arg-max, |t| < 1e-6 times e ~ 1) far above the subnormals: e_c saturates at exp(-86) where t_c < -86.
 */
#ifndef MULACTSEG_UNCERTAINTY_H
#define MULACTSEG_UNCERTAINTY_H

#include "detmath.h"

#ifndef MAS_UNC_BVSB      /* (the codes of include/mulactseg_hip.h, for a unit that includes this header alone) */
#define MAS_UNC_BVSB 0
#define MAS_UNC_MARGIN 1
#define MAS_UNC_LEAST_CONFIDENCE 2
#define MAS_UNC_ENTROPY 3
#endif
#define MAS_UNC_MEASURES 4

#if defined(__HIP_DEVICE_COMPILE__)   /* full unrolling keeps x[] in registers; the host loop runs to C */
#define MAS_UNC_UNROLL _Pragma("unroll")
#else
#define MAS_UNC_UNROLL
#endif

/* 1 / ln C, computed once per call on the host and handed to every pixel */
MAS_HD float mas_uncertainty_inv_log_classes(int C) { return 1.0f / mas_logf((float)C); }

/* x[0..C) holds the logits on entry and e_c on return (x[C..CT) is not touched); `CT` is the extent the loops are unrolled over
 * (a compile-time constant in the kernel, C on the host), 2 <= C <= CT.  Returns u + 1e-8f; *arg = first arg-max; *R = rinv * 2^23. */
MAS_HD float mas_uncertainty_pixel(float* x, const int CT, const int C, float invT, int measure, float inv_log_c, int* arg, float* R) {
    float b1 = -__builtin_inff(), b2 = -__builtin_inff();
    int a1 = 0;
    MAS_UNC_UNROLL
    for (int c = 0; c < CT; ++c) {
        if (c < C) {
            const float v = x[c];
            if (v > b1) {
                b2 = b1;
                b1 = v;
                a1 = c;
            } else if (v > b2) {
                b2 = v;
            }
        }
    }
    const float negM = -(b1 * invT);
    float sum = 0.0f, dot = 0.0f;
    MAS_UNC_UNROLL
    for (int c = 0; c < CT; ++c) {
        if (c < C) {
            const float t = mas_fmaf(x[c], invT, negM);
            const float e = mas_expf_np(t);
            x[c] = e;
            sum = (c == 0) ? e : (sum + e);
            dot = mas_fmaf(e, t, dot);
        }
    }
    const float rinv = 1.0f / sum;
    *arg = a1;
    *R = rinv * 8388608.0f;
    float u;
    if (measure == MAS_UNC_MARGIN) {
        const float e2 = mas_expf_np(mas_fmaf(b2, invT, negM));
        u = 1.0f - (1.0f - e2) * rinv;
    } else if (measure == MAS_UNC_LEAST_CONFIDENCE) {
        u = 1.0f - rinv;
    } else if (measure == MAS_UNC_ENTROPY) {
        u = (mas_logf(sum) - dot * rinv) * inv_log_c;
    } else {
        return mas_bvsb(b1, b2, invT);      /* adds the 1e-8 itself */
    }
    u = u < 0.0f ? 0.0f : u;
    u = u > 1.0f ? 1.0f : u;
    return u + 1e-8f;
}

/* fixed-point quantum of a value for class_sum (40 fractional bits) */
MAS_HD uint64_t mas_uncertainty_quantum(float u) { return mas_fix(u, MAS_SCORE_FRAC); }

#endif /* MULACTSEG_UNCERTAINTY_H */
