/*
 * within_eval.h -- the ARITHMETIC SPECIFICATION of the local-prototype label evaluation inside the queried superpixels
 * (trainer/eval_cosplbl_within_multihot.py, eval_cosplbl_filt_within_multihot.py, eval_maxcosplbl_within_multihot.py,
 * eval_ensemble_plbl_within_multihot.py of the reference).
 *
 * Included by within_eval.hip only, where the kernel (device) and mas_within_eval_reference (a host loop) both go through it, so the
 * two give the same bits.  The tap, the interpolated value, the softmax and the table word are those of online_plbl.h; compile with
 * -ffp-contract=off.
 *
 *   valid      mask byte set, id in [0, S), bits[n, id] != 0.  One-hot superpixels count.
 *   prototype  of (n, s, c), c in bits[n, s]: the valid pixel of s with the largest softmax(up(zq))[c] at temperature 1, ties to the
 *              lowest pixel index -- the table word of mas_opl_pack, left by the group scan without MAS_LOSS_GROUP_ONLY_MULTI.
 *   sim        fma chain over the channels k = 0.. from 0.0f of f_k(prototype) * f_k(pixel), both interpolated (online_plbl.h: sim).
 *   label      candidates c in Y & [0, C) ascending; the first one is taken, a later one replaces it on sim > best.
 *   arg-max    of the interpolated logits over all C channels, walked from channel 0, replaced on strict '>': the first maximum.
 *   global     max over c < C of (c in Y ? up(zq)[c] : 0.0f), walked the same way: the reference's (logits * multi_hot).max.
 *   PROTO      the label.
 *   FILT       the label where it equals the arg-max, else 255; then a pixel that is the prototype of classes of its own superpixel
 *              takes the highest of them.
 *   diag       [0] valid pixels, [1] table entries with a prototype, [2] valid pixels with best < global, [3] valid pixels that have
 *              a label in PROTO and 255 in FILT (0 in mode PROTO).
 */
#ifndef MULACTSEG_WITHIN_EVAL_H
#define MULACTSEG_WITHIN_EVAL_H

#include "online_plbl.h"

/* the candidate row of a pixel, 0 when it is not valid */
MAS_HD uint32_t mas_we_valid_bits(unsigned char mask_byte, long long id, int S, const uint32_t* bits_row) {
    if (!mask_byte || id < 0 || id >= S) return 0u;
    return bits_row[id];
}

MAS_HD uint32_t mas_we_cands(uint32_t Y, int C) { return C < 32 ? (Y & ((1u << C) - 1u)) : Y; }

/* whether the table word holds a prototype of an H*W picture, and its pixel */
MAS_HD bool mas_we_word_proto(uint64_t word, uint32_t HW, uint32_t* pp) {
    *pp = mas_opl_word_pixel(word);
    return (uint32_t)(word >> 32) != 0u && *pp < HW;
}

/* One channel of the walk over the interpolated logits v_0, v_1, ... of a pixel with row Y: *amax the first arg-max so far (replaced on
 * strict '>'), *glob the maximum so far of (c in Y ? v_c : 0).  Channel 0 starts all three. */
MAS_HD void mas_we_logit_step(int c, float v, uint32_t Y, float* best, int* amax, float* glob) {
    const float t = ((Y >> c) & 1u) ? v : 0.0f;
    if (c == 0) {
        *best = v;
        *amax = 0;
        *glob = t;
        return;
    }
    if (v > *best) { *best = v; *amax = c; }
    *glob = (t > *glob) ? t : *glob;
}

/* the label of a valid pixel: arg = its nearest-prototype class (-1: no candidate has a prototype), amax = the arg-max of its logits,
 * proto_hi = the highest class it is the prototype of (-1: none); *removed = whether the filter took its label away */
MAS_HD int mas_we_label(int mode, int arg, int amax, int proto_hi, int* removed) {
    *removed = 0;
    if (arg < 0) return 255;
    if (mode != MAS_WE_FILT) return arg;
    int lab = (arg == amax) ? arg : 255;
    if (proto_hi >= 0) lab = proto_hi;
    *removed = (lab == 255) ? 1 : 0;
    return lab;
}

#endif /* MULACTSEG_WITHIN_EVAL_H */
