/*
 * partial_label.h -- the ARITHMETIC SPECIFICATION of the multi-hot pixel term of the stage-1 partial-label losses.
 *
 * One selected pixel's probabilities p_c (the scan's v[c] after mas_softmax_regs and the multiplication by rinv) and its target bit
 * mask Y (nb = popcount(Y) candidates) go in; the loss term l and the gradient coefficients d_c = dl/dz_c * a come out, a = scale * invT.
 * Like uncertainty.h the header compiles as device code (hipcc, gfx950) and as plain host C; it uses mas_logf and correctly rounded
 * add, multiply and divide only, so the kernels (losses.hip: k_partial_loss_fwd / _bwd) and the host loop
 * (mas_partial_loss_reference) give the same bits.  Compile with -ffp-contract=off.
 *
 * eps = 1e-8f; every sum runs in ascending channel order; pos = sum_{c in Y} p_c from 0.0f.
 *
 *   choice  (merged positive; trainer/active_joint_multi_predignore_lossdecomp.py:53-70 -- the bits of oracle/exact.c)
 *     l   = -log(pos + eps)
 *     d_c = coef * (p_c * (pos - y_c)),  coef = a * (1 / (pos + eps))
 *   topone  (naive top-1 within the candidate set; trainer/active_joint_multi_lossdecomp_topone.py)
 *     m   = the first maximum of p_c over c in Y by a strict '>' scan from -1 (a tie goes to the lowest class index)
 *     l   = -log(p_m + eps)
 *     d_c = k * (p_c - [c = m]),  k = a * (p_m / (p_m + eps))
 *   rc      (risk-consistent weighting; utils/loss.py:653-707, RCMultiChoiceCE)
 *     w_c = p_c / pos for c in Y -- constants of the gradient (the reference detaches them)
 *     l   = sum_{c in Y} w_c * (-log(p_c + eps))
 *     r_c = p_c / (p_c + eps);  U = sum_{c in Y} w_c * r_c
 *     d_k = a * (p_k * U - [k in Y] * (w_k * r_k))
 *     pos == 0 (every candidate probability is zero; the reference divides 0 / 0 and returns NaN): w_c = 1 / nb.  Then
 *     l = -log(eps), every r_c = 0 and the gradient is zero -- finite.  The scan's softmax cannot produce it (mas_expf_np saturates at
 *     exp(-86) and the row sum is below 32), the definition covers callers that hand in other probabilities.
 *
 * For nb == 1 the three agree (w = 1, the maximum is the only candidate): callers keep one-hot pixels on the choice arithmetic.
 * p_c + eps <= 1 for p_c <= 1 (eps is below half an ulp of 1), so no -log above is negative by more than the rounding of mas_logf
 * near 1; such a term and such an l go through mas_fix, which maps negative values to 0 -- as for the existing term.
 */
#ifndef MULACTSEG_PARTIAL_LABEL_H
#define MULACTSEG_PARTIAL_LABEL_H

#include "detmath.h"

#define MAS_PL_CHOICE 0
#define MAS_PL_RC 1
#define MAS_PL_TOPONE 2

#ifndef MAS_LOSS_RC       /* (the flag bits of include/mulactseg_hip.h, for a unit that includes this header alone) */
#define MAS_LOSS_RC 32
#define MAS_LOSS_TOPONE 64
#endif

#define MAS_PL_EPS 1e-8f

#if defined(__HIP_DEVICE_COMPILE__)   /* full unrolling keeps p[] in registers; the host loop runs to C */
#define MAS_PL_UNROLL _Pragma("unroll")
#else
#define MAS_PL_UNROLL
#endif

MAS_HD int mas_pl_mode(int flags) { return (flags & MAS_LOSS_RC) ? MAS_PL_RC : ((flags & MAS_LOSS_TOPONE) ? MAS_PL_TOPONE : MAS_PL_CHOICE); }

MAS_HD int mas_pl_popcount(uint32_t y) { return __builtin_popcount(y); }

/* pos = sum_{c in Y} p_c; `CT` is the extent the loops are unrolled over (a compile-time constant in the kernel, C on the host) */
MAS_HD float mas_pl_pos(const float* p, const int CT, const int C, uint32_t Y) {
    float pos = 0.0f;
    MAS_PL_UNROLL
    for (int c = 0; c < CT; ++c)
        if (c < C) pos = ((Y >> c) & 1u) ? (pos + p[c]) : pos;
    return pos;
}

/* first maximum over the candidates: *pm = p_m, returns m (0 and p_m = -1 for an empty Y, which no caller passes) */
MAS_HD int mas_pl_top(const float* p, const int CT, const int C, uint32_t Y, float* pm) {
    float best = -1.0f;
    int m = 0;
    MAS_PL_UNROLL
    for (int c = 0; c < CT; ++c) {
        if (c < C) {
            const int better = ((Y >> c) & 1u) && (p[c] > best);
            best = better ? p[c] : best;
            m = better ? c : m;
        }
    }
    *pm = best;
    return m;
}

/* w_c of a candidate */
MAS_HD float mas_pl_rc_weight(float pc, float pos, float inv_nb) { return pos > 0.0f ? pc / pos : inv_nb; }

/* the loss term l of one pixel (not yet through mas_fix) */
MAS_HD float mas_pl_loss(const float* p, const int CT, const int C, uint32_t Y, int mode) {
    if (mode == MAS_PL_TOPONE) {
        float pm;
        (void)mas_pl_top(p, CT, C, Y, &pm);
        return -mas_logf(pm + MAS_PL_EPS);
    }
    const float pos = mas_pl_pos(p, CT, C, Y);
    if (mode == MAS_PL_RC) {
        const float inv_nb = 1.0f / (float)mas_pl_popcount(Y);
        float l = 0.0f;
        MAS_PL_UNROLL
        for (int c = 0; c < CT; ++c)
            if (c < C && ((Y >> c) & 1u)) l = l + mas_pl_rc_weight(p[c], pos, inv_nb) * (-mas_logf(p[c] + MAS_PL_EPS));
        return l;
    }
    return -mas_logf(pos + MAS_PL_EPS);
}

/* per-pixel constants of the gradient.  choice: k0 = coef, k1 = pos;  topone: k0 = k, m;  rc: k0 = a, k1 = U, pos, inv_nb */
typedef struct { float k0, k1, pos, inv_nb; int m; } mas_pl_grad_ctx;

MAS_HD mas_pl_grad_ctx mas_pl_grad_prepare(const float* p, const int CT, const int C, uint32_t Y, int mode, float a) {
    mas_pl_grad_ctx k;
    k.k0 = 0.0f, k.k1 = 0.0f, k.pos = 0.0f, k.inv_nb = 0.0f, k.m = 0;
    if (mode == MAS_PL_TOPONE) {
        float pm;
        k.m = mas_pl_top(p, CT, C, Y, &pm);
        k.k0 = a * (pm / (pm + MAS_PL_EPS));
        return k;
    }
    const float pos = mas_pl_pos(p, CT, C, Y);
    if (mode == MAS_PL_RC) {
        const float inv_nb = 1.0f / (float)mas_pl_popcount(Y);
        float U = 0.0f;
        MAS_PL_UNROLL
        for (int c = 0; c < CT; ++c)
            if (c < C && ((Y >> c) & 1u)) U = U + mas_pl_rc_weight(p[c], pos, inv_nb) * (p[c] / (p[c] + MAS_PL_EPS));
        k.k0 = a, k.k1 = U, k.pos = pos, k.inv_nb = inv_nb;
        return k;
    }
    k.k0 = a * (1.0f / (pos + MAS_PL_EPS));
    k.k1 = pos;
    return k;
}

/* d_c of class c with probability pc; in_y = bit c of Y */
MAS_HD float mas_pl_grad(const mas_pl_grad_ctx k, int mode, float pc, int in_y, int c) {
    if (mode == MAS_PL_TOPONE) return k.k0 * (pc - ((c == k.m) ? 1.0f : 0.0f));
    if (mode == MAS_PL_RC) {
        float t = pc * k.k1;
        if (in_y) {
            t = t - mas_pl_rc_weight(pc, k.pos, k.inv_nb) * (pc / (pc + MAS_PL_EPS));
        }
        return k.k0 * t;
    }
    return k.k0 * (pc * (k.k1 - (in_y ? 1.0f : 0.0f)));
}

#endif /* MULACTSEG_PARTIAL_LABEL_H */
