/*
 * hier_group.h -- the ARITHMETIC SPECIFICATION of the hierarchical group term (utils/loss.py:143-235 HierGroupMultiLabelCE and
 * :439-533 AugHierGroupMultiLabelCE of the reference; trainer/active_joint_hier_multi.py).
 *
 * Included by online_plbl.hip only, where the kernels (k_hier_pairs, k_hier_fwd / _bwd: the HierCe policy of the tile-queue core) and
 * the host loops mas_hier_group_reference and mas_async_hier_reference go through it, so the two give the same bits.  Like
 * teacher_terms.h it compiles as device code (hipcc, gfx950) and as plain host C, and uses mas_logf and correctly rounded add, multiply
 * and divide only.  Compile with -ffp-contract=off.
 *
 *   p        the softmax of the pixel's interpolated logits at temperature 1.0 (mas_opl_softmax of online_plbl.h with invT = 1.0f):
 *            the reference's constructor hands temperature=1.0 to its base class whatever it is given (:145).
 *   pair     every (superpixel s, class c in Y_s) whose word of the group scan's table `gmax` is non-zero has an arg-pixel (the selected
 *            pixel of s with the largest p_c, the first one in row-major order on a tie).  s' = small[arg-pixel]; a pair with s'
 *            outside [0, Ss) is dropped.  mult[n, s', c] += 1 and bit c of any[n, s'] is set -- pairs are NOT deduplicated (the
 *            reference gathers by index, :224): mult is the multiplicity M.  Integer additions, so the table does not depend on the
 *            order.
 *   counted  a pixel with its mask byte set, small id in [0, Ss) and any[n, small] != 0.
 *   term     t = sum over c = 0, 1, ... (ascending, from 0.0f) with bit c of any[n, small] of  w_c * (-mas_logf(p_c + eps)),
 *            w_c = (float)mult[n, small, c] (exact: a multiplicity is far below 2^24): the logarithm, its negation, one
 *            multiplication, one addition.  The sum adds mas_fix(t) (a negative t, the rounding of mas_logf next to p = 1, adds 0).
 *   count    the pixel adds sum_c mult[n, small, c], an integer.
 *   value    sum / (1 + n): (double)sum * 2^-MAS_LOSS_FRAC_BITS / (double)(1 + n), rounded to float once.
 *   gradient the arg-pixel choice carries none.  r_c = p_c / (p_c + eps);  U = sum over the same c, ascending from 0.0f, of w_c * r_c;
 *            a = upstream / (float)(1 + n)  (times invT = 1.0f, which changes no bit and is left out);
 *            d_k = a * (p_k * U - w_k * r_k), w_k = 0 off the set: the two products, the subtraction, then the product with a.
 *            Every tap adds round_to_nearest_even(d_k * (ly * lx) * 2^MAS_GRAD_FRAC_BITS) to its element (mas_opl_grad_fix).
 *
 * eps = 1e-8f.
 */
#ifndef MULACTSEG_HIER_GROUP_H
#define MULACTSEG_HIER_GROUP_H

#include "online_plbl.h"

#define MAS_HG_EPS 1e-8f

/* term of one counted pixel with probabilities p: Yc = its bits of `any` within the C classes, m = its row of `mult`.
 * *U and *cnt (the pixel's share of the count) come out too. */
template <int CT>
MAS_HD float mas_hg_term(const float (&p)[CT], int C, uint32_t Yc, const uint32_t* m, float* U, uint32_t* cnt) {
    float t = 0.0f, u = 0.0f;
    uint32_t n = 0;
    MAS_OPL_UNROLL
    for (int c = 0; c < CT; ++c) {
        if (c < C && ((Yc >> c) & 1u)) {
            const uint32_t mc = m[c];
            const float w = (float)mc;
            const float pe = p[c] + MAS_HG_EPS;
            t = t + w * (-mas_logf(pe));
            u = u + w * (p[c] / pe);
            n += mc;
        }
    }
    *U = u;
    *cnt = n;
    return t;
}

/* d_k / a: p_k * U - w_k * r_k  (w_k = 0 off the set) */
MAS_HD float mas_hg_dir(float pk, float U, float wk) { return pk * U - wk * (pk / (pk + MAS_HG_EPS)); }

/* a of the backward: upstream / (1 + n) */
MAS_HD float mas_hg_scale(float upstream, uint64_t n) { return upstream / (float)(n + 1u); }

/* acc = {sum, n} -> the loss value sum / (1 + n) */
MAS_HD float mas_hg_value(uint64_t sum, uint64_t n) {
    union { double d; uint64_t u; } s;
    s.u = (uint64_t)(1023 - MAS_LOSS_FRAC_BITS) << 52;
    return (float)(((double)sum * s.d) / (double)(n + 1u));
}

/* ---- the cross-view ("async") forms: utils/loss.py:341-437 AsyncHierGroupMultiLabelCE and :237-339 WeightAsyncHierGroupMultiLabelCE of
 * the reference (trainer/active_joint_hier_multi_async.py, ..._async_weight.py).  Two views of one picture: the tables come from the WEAK
 * view (an eval-mode teacher on the whole picture, its own geometry H_o x W_o), the sum runs over the STRONG view (the student's crop).
 *
 *   tables   gmax, mult and any are those above, built from the weak view's logits, ids, fine ids and mask at temperature 1.0.  There is no
 *            only_single filter in these two classes.  The fine ids are the link between the views: a table row that no strong pixel
 *            carries adds nothing.
 *   weight   wgt[n, s', c], for the pairs that exist (bit c of any[n, s']) and 0 elsewhere, over the selected weak pixels whose fine id
 *            is s', of the teacher's p_c (mas_opl_softmax at invT = 1.0f of the interpolated logits):
 *              max   the largest p_c: an unsigned maximum of the bit patterns, which keeps the order because p_c >= 0;
 *              mean  sum of mas_ahg_fix(p_c) = floor(p_c * 2^MAS_AHG_WEIGHT_FRAC) in a u64 per pair, and the number of those pixels in a
 *                    u32 per (n, s');
 *                    wgt = (float)(((double)sum * 2^-MAS_AHG_WEIGHT_FRAC) / (double)count), rounded once (mas_ahg_mean).
 *                    p_c <= 1 + 2^-23, so one pixel adds at most 2^40 + 2^17 and the 2^21 pixels of a 1024 x 2048 view less than 2^62:
 *                    the sum cannot wrap.  Integer sums: the table does not depend on the order.
 *   term     as above with  w_c = (float)mult[n, small, c] * wgt[n, small, c]  (one multiplication) in the weighted form.
 *   count    the weighted form adds mult[n, small, c] only where wgt[n, small, c] != 0.0f -- the decidable form of the reference's
 *            size[value.nonzero()]: a pair of weight 0 is counted in neither; a pair whose value is exactly 0 over a non-empty fine
 *            superpixel (every p_c == 1.0f) is counted here and not in the reference.
 *   gradient as above with the same w_c; the weight is detached (the teacher runs under no_grad). */
#define MAS_AHG_WEIGHT_FRAC 40

/* the weighted twin of mas_hg_term: g = the pixel's row of `wgt` */
template <int CT>
MAS_HD float mas_ahg_term(const float (&p)[CT], int C, uint32_t Yc, const uint32_t* m, const float* g, float* U, uint32_t* cnt) {
    float t = 0.0f, u = 0.0f;
    uint32_t n = 0;
    MAS_OPL_UNROLL
    for (int c = 0; c < CT; ++c) {
        if (c < C && ((Yc >> c) & 1u)) {
            const uint32_t mc = m[c];
            const float gc = g[c];
            const float w = (float)mc * gc;
            const float pe = p[c] + MAS_HG_EPS;
            t = t + w * (-mas_logf(pe));
            u = u + w * (p[c] / pe);
            n += (gc != 0.0f) ? mc : 0u;
        }
    }
    *U = u;
    *cnt = n;
    return t;
}

/* floor(p * 2^MAS_AHG_WEIGHT_FRAC) of a probability p < 2: what mas_fix(p, MAS_AHG_WEIGHT_FRAC) gives there; zero, subnormal and negative
 * inputs give 0.  A function of its own: mas_fix keeps being called with one constant `frac` throughout the unit's device code, so the
 * code of the kernels that were there before is what it was. */
MAS_HD uint64_t mas_ahg_fix(float p) {
    const uint32_t b = mas_f2u(p);
    const int e = (int)((b >> 23) & 0xffu);
    const uint64_t m = (uint64_t)((b & 0x007fffffu) | 0x00800000u);
    const int sh = e - 150 + MAS_AHG_WEIGHT_FRAC;           /* value = m * 2^(e-150); sh <= 17 for p < 2 */
    const uint64_t q = sh >= 0 ? (m << (sh > 17 ? 17 : sh)) : (m >> (-sh > 63 ? 63 : -sh));
    return ((b >> 31) | (uint32_t)(e == 0)) ? (uint64_t)0 : q;
}

/* the mean weight of one pair from its fixed-point sum and the pixel count of its fine superpixel (count > 0) */
MAS_HD float mas_ahg_mean(uint64_t sum, uint32_t count) {
    union { double d; uint64_t u; } s;
    s.u = (uint64_t)(1023 - MAS_AHG_WEIGHT_FRAC) << 52;
    return (float)(((double)sum * s.d) / (double)count);
}

#endif /* MULACTSEG_HIER_GROUP_H */
