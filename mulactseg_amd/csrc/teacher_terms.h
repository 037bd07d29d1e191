/*
 * teacher_terms.h -- the ARITHMETIC SPECIFICATION of the two candidate-set regularisers of the stage-1 losses that need no prototypes:
 * the teacher-gated top-1 term and the candidate entropy.
 *
 * One selected pixel of a MULTI-HOT superpixel goes in: its logits z_c, its target bit mask Y (nb = popcount(Y) > 1; pixels with
 * nb <= 1 enter neither term -- unlike --partial_loss topone, whose one-hot pixels go to the CE term) and, for `top1`, the logits of
 * the eval-mode teacher forward.  The loss term and the gradient coefficients d_c = dl/dz_c * a come out, a = scale * invT with invT
 * the term's OWN inverse temperature (the co-resident merged-positive and group terms keep theirs).  Like partial_label.h the header
 * compiles as device code (hipcc, gfx950) and as plain host C; it uses mas_fmaf and mas_expf_np in the softmax, mas_logf, and correctly
 * rounded add, multiply and divide only, so the kernels (losses.hip: the TT instantiations of k_partial_loss_fwd / _bwd) and the host loop
 * (mas_teacher_loss_reference) give the same bits.  Compile with -ffp-contract=off.
 *
 * eps = 1e-8f; every sum runs in ascending channel order from 0.0f.
 *
 * softmax over a channel set M (mas_tt_softmax; the operation order of mas_softmax_regs, common.h, which it equals bit for bit when M
 * holds every channel):  m = max_{c in M} z_c;  e_c = mas_expf_np(fma(z_c, invT, -(m * invT)));  sum = ((e_a + e_b) + ...);
 * p_c = e_c * (1 / sum) for c in M, 0 elsewhere.
 *
 *   top1  (self-training on the candidates; trainer/active_joint_multi_predignore_top1plbl.py:19-82, TopOnePlbl.forward)
 *     p = softmax of the student's logits, t = softmax of the teacher's, both over all channels at the term's temperature
 *     g   = max_{c in Y} t_c                              (:68)
 *           with within_filtering: g = max_{c in Y} t_c / sum_{c in Y} t_c  (:70; the division is monotonic, so the maximum of the
 *           quotients is the quotient of the maximum).  sum_{c in Y} t_c == 0 (the reference divides 0 / 0): the pixel does not
 *           count -- finite.  mas_expf_np saturates at exp(-86) > 0, so no softmax of this header produces it; the definition covers
 *           callers that hand in other probabilities, as partial_label.h does for its own corner.
 *     the pixel counts iff plbl_th < g (strict, :73)
 *     m   = the first maximum of p_c over c in Y by a strict '>' scan (mas_pl_top)
 *     l   = -log(p_m + eps)                               (:77)
 *     d_c = k * (p_c - [c = m]),  k = a * (p_m / (p_m + eps))      -- the topone gradient of partial_label.h
 *     The teacher is a constant of the gradient (:35, :63).  The term is sum l / (1 + n_counted) (num_valid starts at 1, :33).
 *
 *   ent   (entropy of the softmax restricted to the candidates; trainer/active_joint_multi_predignore_multient.py:16-70,
 *          MultiChoiceEnt_.forward -- the base class utils/loss.py MultiChoiceEnt does not run, the trainer's override does)
 *     Y'  = {c in Y : z_c != 0}.  The reference masks by multiplying the logits with the 0/1 target (:52) and then sends every exact
 *           0.0 product to -inf (:57): a candidate whose logit is exactly 0.0f (or -0.0f) drops out of its own softmax.  Replicated
 *           here as the reference's behaviour.  An empty Y' (every candidate logit exactly zero; the reference returns NaN) gives
 *           h = 0 and a zero gradient; the pixel is still counted, as the reference counts it (:62).
 *     q   = softmax over Y' of z_c * invT                  (:59)
 *     h   = -sum_{c in Y'} q_c * log(q_c + eps)           (:61)
 *     G_j = -(log(q_j + eps) + q_j / (q_j + eps));  U = sum_{j in Y'} q_j * G_j
 *     d_k = (a * q_k) * (G_k - U) for k in Y', 0 elsewhere
 *     The term is sum h / (1 + n) over the selected multi-hot pixels (:29, :62-66).
 *     CHOICE: q is the RESTRICTED softmax (max and sum over Y' only), not p_c / sum_{Y'} p of the scan's full softmax.  The two agree
 *     in exact arithmetic; in f32 the full softmax loses the candidates when a non-candidate logit leads them by more than 86 * T
 *     (8.6 at the recipe's T = 0.1): every candidate's exponential then sits on mas_expf_np's floor exp(-86), the quotient becomes
 *     uniform and the entropy ln nb whatever the logits say.  The restricted form subtracts the candidates' own maximum, so its
 *     largest exponential is exactly 1 and q has the relative error of one softmax (tests/test_teacher_terms_cpu.py bounds both
 *     against float64, the second on such a pixel).
 *
 * h >= 0 up to the rounding of mas_logf near 1 and l >= 0 likewise; both go through mas_fix, which maps negative values to 0.
 *
 *   wgroup  (the group / max-pool term with every (superpixel, class) entry weighted by the teacher's confidence;
 *            trainer/active_joint_multi_predignore_wgroup.py:12-82, WeightedGroupMultiLabelCE.forward)
 *     This term lives in the group table, not in the fourth slot: it has no temperature of its own, both tables use the group invT.
 *     p   = the scan's softmax of the student's logits: r = mas_softmax_regs(z, invT) (common.h), p_c = e_c * r            (:27)
 *     t   = the same arithmetic on the teacher's logits (mas_tt_wg_probs states it for the host)                          (:39)
 *     P[s,c]  = max over the selected pixels of s of p_c, with its arg-pixel (the packed u64 table `gmax`), c in Y_s       (:56)
 *     Wt[s,c] = max over the SAME pixels of t_c -- the teacher's own maximum, not its value at the student's arg-pixel     (:69)
 *               Probabilities are non-negative floats, whose bit patterns order as unsigned integers: the table `tmax` holds
 *               u32 bits and is combined with an unsigned maximum.  A maximum does not depend on the order, so the bits are defined.
 *     an entry counts iff the bits of P are non-zero (:64, nonzero of the student's table; Wt may be anything, 0 included)
 *     l   = w * (-mas_logf(p + eps)), w = Wt[s,c], p = P[s,c]: the logarithm, its negation, then ONE multiplication         (:75)
 *     the term is sum l / (1 + n) over the counted entries, l through mas_fix (:74-78)
 *     t_c = -((g * w) / (p_c + eps)) at the arg-pixel of entry (s,c), g = (upstream / (1 + n)) * invT: the product g * w first,
 *           then the division, then the negation; it enters the pixel's gradient exactly as the unweighted coefficient
 *           -(g / (p_c + eps)) of the group term does (d_j += [j = c] t_c p_j - p_j sum_c t_c p_c).  The teacher is a constant (:38, :67).
 *     Consequence: teacher logits equal to the student's give Wt == (gmax >> 32) as bits wherever gmax != 0.
 */
#ifndef MULACTSEG_TEACHER_TERMS_H
#define MULACTSEG_TEACHER_TERMS_H

#include "partial_label.h"

#define MAS_TT_NONE 0
#define MAS_TT_TOP1 1
#define MAS_TT_ENT 2
#define MAS_TT_WGROUP 3

#ifndef MAS_LOSS_TOP1     /* (the flag bits of include/mulactseg_hip.h, for a unit that includes this header alone) */
#define MAS_LOSS_TOP1 128
#define MAS_LOSS_ENT 256
#define MAS_LOSS_WITHIN 512
#endif
#ifndef MAS_LOSS_WGROUP
#define MAS_LOSS_WGROUP 1024
#endif

#define MAS_TT_EPS 1e-8f

MAS_HD int mas_tt_mode(int flags) {
    return (flags & MAS_LOSS_TOP1) ? MAS_TT_TOP1 : ((flags & MAS_LOSS_ENT) ? MAS_TT_ENT : ((flags & MAS_LOSS_WGROUP) ? MAS_TT_WGROUP : MAS_TT_NONE));
}

/* the mask of all C channels */
MAS_HD uint32_t mas_tt_all(int C) { return C >= 32 ? 0xffffffffu : ((1u << C) - 1u); }

/* x[c] = z_c on entry; on return the softmax over the channels of M at inverse temperature invT, 0 outside M (an empty M: all 0) */
MAS_HD void mas_tt_softmax(float* x, const int CT, const int C, uint32_t M, float invT) {
    float m = -__builtin_inff();
    MAS_PL_UNROLL
    for (int c = 0; c < CT; ++c)
        if (c < C && ((M >> c) & 1u)) m = (x[c] > m) ? x[c] : m;
    const float negM = -(m * invT);
    float sum = 0.0f;
    MAS_PL_UNROLL
    for (int c = 0; c < CT; ++c) {
        if (c < C) {
            const int in = (int)((M >> c) & 1u);
            x[c] = in ? mas_expf_np(mas_fmaf(x[c], invT, negM)) : 0.0f;
            sum = in ? (sum + x[c]) : sum;
        }
    }
    const float rinv = 1.0f / sum;
    MAS_PL_UNROLL
    for (int c = 0; c < CT; ++c)
        if (c < C) x[c] = ((M >> c) & 1u) ? (x[c] * rinv) : 0.0f;
}

/* top1: does the pixel count?  t = the teacher's probabilities */
MAS_HD int mas_tt_gate(const float* t, const int CT, const int C, uint32_t Y, int within, float th) {
    float g;
    (void)mas_pl_top(t, CT, C, Y, &g);
    if (within) {
        const float s = mas_pl_pos(t, CT, C, Y);
        if (!(s > 0.0f)) return 0;
        g = g / s;
    }
    return th < g;
}

/* ent: the candidates that stay in the softmax */
MAS_HD uint32_t mas_tt_ent_set(const float* z, const int CT, const int C, uint32_t Y) {
    uint32_t M = Y;
    MAS_PL_UNROLL
    for (int c = 0; c < CT; ++c)
        if (c < C && z[c] == 0.0f) M &= ~(1u << c);
    return M;
}

/* ent: h of one pixel, q = mas_tt_softmax over M = mas_tt_ent_set (not yet through mas_fix) */
MAS_HD float mas_tt_ent_loss(const float* q, const int CT, const int C, uint32_t M) {
    float s = 0.0f;
    MAS_PL_UNROLL
    for (int c = 0; c < CT; ++c)
        if (c < C && ((M >> c) & 1u)) s = s + q[c] * mas_logf(q[c] + MAS_TT_EPS);
    return -s;
}

MAS_HD float mas_tt_ent_g(float qc) { return -(mas_logf(qc + MAS_TT_EPS) + qc / (qc + MAS_TT_EPS)); }

/* ent: U of one pixel */
MAS_HD float mas_tt_ent_u(const float* q, const int CT, const int C, uint32_t M) {
    float u = 0.0f;
    MAS_PL_UNROLL
    for (int c = 0; c < CT; ++c)
        if (c < C && ((M >> c) & 1u)) u = u + q[c] * mas_tt_ent_g(q[c]);
    return u;
}

/* ent: d_k of class k with restricted probability qk; in_m = bit k of M */
MAS_HD float mas_tt_ent_grad(float a, float U, float qk, int in_m) { return in_m ? ((a * qk) * (mas_tt_ent_g(qk) - U)) : 0.0f; }

/* wgroup: x[c] = logits on entry, the group probabilities on return -- the operation order of mas_softmax_regs followed by `* rinv`
 * (the first exponential starts the sum), which the scans run on the student's and on the teacher's row alike */
MAS_HD void mas_tt_wg_probs(float* x, const int C, float invT) {
    float m = x[0];
    for (int c = 1; c < C; ++c) m = (x[c] > m) ? x[c] : m;
    const float negM = -(m * invT);
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) {
        x[c] = mas_expf_np(mas_fmaf(x[c], invT, negM));
        sum = (c == 0) ? x[c] : (sum + x[c]);
    }
    const float rinv = 1.0f / sum;
    for (int c = 0; c < C; ++c) x[c] = x[c] * rinv;
}

/* wgroup: the term of one counted entry (not yet through mas_fix) */
MAS_HD float mas_tt_wg_loss(float w, float p) { return w * (-mas_logf(p + MAS_TT_EPS)); }

/* wgroup: the backward coefficient t_c of an arg-pixel entry; g = the group scale * invT */
MAS_HD float mas_tt_wg_coef(float g, float w, float pc) { return -((g * w) / (pc + MAS_TT_EPS)); }

#endif /* MULACTSEG_TEACHER_TERMS_H */
