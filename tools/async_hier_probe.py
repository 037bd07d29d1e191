"""Probe of the cross-view hierarchical group terms (csrc/hier_group.h, second section; k_hier_weights, k_whier_fwd / _bwd of
csrc/online_plbl.hip) on the siblings' batch: the strong view is quarter-resolution logits [4,19,192,192] at 768 x 768, the weak view
[4,19,256,512] at 1024 x 2048 against 2048 superpixels and a seeded fine map of 8192 ids; the strong maps are a 768 x 768 window of the
weak ones.  Runs, ``--reps`` times each,

  tables    ``ops.async_hier_tables`` without weights, with 'max' and with 'mean' (memsets, the weak-view group scan, k_hier_pairs,
            k_hier_weights, k_hier_weights_mean)
  plain     ``ops.async_hier_loss_fwd`` / ``_bwd`` without weights (k_hier_fwd / _bwd)
  weighted  the same with the 'max' table (k_whier_fwd / _bwd)

so that one ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/async_hier_probe.py`` run (kernel trace only, a run
of its own) times them side by side (``--summarize <kernel trace csv>`` prints the per-kernel medians), and reports (JSON on stdout)
the pairs, the counted pixels and counts, and the allocator peak of a ``forward_lowres`` step (weighted group term + merged positive)
against the ATen composition of the same two terms on materialised logits of both views."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hier_group_probe import peak_of  # noqa: E402

N, C, h, w, ho, wo, S, SS, T = 4, 19, 192, 192, 256, 512, 2048, 8192, 0.1
H, W, HO, WO = 4 * h, 4 * w, 4 * ho, 4 * wo
Y0, X0 = 128, 640                   # where the strong window lies in the weak view
EPS = 1e-8


def aten_step(torch, zq, zq_weak, tgt, spx, small, msk, spx_w, small_w, msk_w):
    """merged positive + the max-weighted cross-view group term on materialised logits of both views with ATen ops"""
    z = torch.nn.functional.interpolate(zq, size=(H, W), mode='bilinear', align_corners=False)
    with torch.no_grad():
        zw = torch.nn.functional.interpolate(zq_weak, size=(HO, WO), mode='bilinear', align_corners=False)
    total, n = 0, 1
    for i in range(N):
        m = msk[i].reshape(-1)
        ids, fine = spx[i].reshape(-1)[m], small[i].reshape(-1)[m]
        zi = z[i].permute(1, 2, 0).reshape(H * W, C)[m]
        y = tgt[i][ids].float()
        total = total + 16.0 * (-torch.log((torch.softmax(zi / T, dim=1) * y).sum(dim=1) + EPS)).sum()
        mw = msk_w[i].reshape(-1)
        ids_w, fine_w = spx_w[i].reshape(-1)[mw], small_w[i].reshape(-1)[mw]
        pw = torch.softmax(zw[i].permute(1, 2, 0).reshape(HO * WO, C)[mw], dim=1)
        best = torch.zeros((S, C), device=pw.device).scatter_reduce(0, ids_w[:, None].expand(-1, C), pw, 'amax', include_self=True)
        is_arg = (pw == best[ids_w]) & (tgt[i][ids_w] != 0)                    # (ties count twice here: a memory probe, not a reference)
        mult = torch.zeros((SS + 1, C), device=pw.device).index_add_(0, fine_w, is_arg.float())
        top = torch.zeros((SS + 1, C), device=pw.device).scatter_reduce(0, fine_w[:, None].expand(-1, C), pw, 'amax', include_self=True)
        wgt = (mult * top)[fine]
        total = total + (wgt * -torch.log(torch.softmax(zi, dim=1) + EPS)).sum()
        n = n + mult[fine].sum()
    (total / n).backward()


def summarize(path):
    """Per-kernel medians of a kernel-trace csv.  Not ``online_plbl_probe.summarize``: that one keys on the bare kernel name, which would
    merge the 'max' and 'mean' forms of k_hier_weights (<19, true, false> / <19, true, true>); here the template arguments stay in the key."""
    import csv
    import re
    out = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r'\bk_\w+(?:<[^>]*>)?', r['Kernel_Name'])
        name = m.group(0) if m else r['Kernel_Name'].split('(')[0][:48]
        out.setdefault(name, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print(json.dumps({k: {'calls': len(v), 'median_us': round(float(np.median(v)), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)}
                      for k, v in sorted(out.items())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--summarize')
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    from mulactseg_amd import ops, synth
    from mulactseg_amd.utils import loss as L
    zq = torch.from_numpy(synth.logits(3, N, C, h, w)).cuda()
    zw = torch.from_numpy(synth.logits(4, N, C, ho, wo)).cuda()
    crops = [synth.train_crop(50 + i, HO, WO, S, frac_selected=0.08) for i in range(N)]
    spx_h = np.stack([c[0] for c in crops])
    msk_h = np.stack([c[1] for c in crops])
    small_h = np.stack([synth.superpixel_map(90 + i, HO, WO, SS) for i in range(N)])
    small_h[spx_h == S] = SS

    def window(arr):
        return torch.from_numpy(np.ascontiguousarray(arr[:, Y0:Y0 + H, X0:X0 + W][:, :, ::-1])).cuda()
    spx_w, small_w, msk_w = (torch.from_numpy(x).cuda() for x in (spx_h, small_h, msk_h))
    spx, small, msk = window(spx_h), window(small_h), window(msk_h)
    tgt = torch.from_numpy(np.stack([synth.multi_hot_targets(70 + i, S, C + 1, p_counts=(0.40, 0.35, 0.15, 0.10)) for i in range(N)])).cuda()
    tgt[..., -1] = 0
    bits = ops.target_bits(tgt, C)
    one = torch.ones(1, device='cuda')
    out = dict(shape=dict(strong=[N, C, h, w, H, W], weak=[ho, wo, HO, WO], S=S, Ss=SS), selected_weak=int(msk_w.sum()), selected_strong=int(msk.sum()))
    for _ in range(a.reps):
        plain = ops.async_hier_tables(zw, (HO, WO), spx_w, small_w, SS, msk_w, bits)
        tmax = ops.async_hier_tables(zw, (HO, WO), spx_w, small_w, SS, msk_w, bits, weight_reduce='max')
        tmean = ops.async_hier_tables(zw, (HO, WO), spx_w, small_w, SS, msk_w, bits, weight_reduce='mean')
        _, acc = ops.async_hier_loss_fwd(zq, (H, W), small, SS, msk, plain['mult'], plain['any'])
        ops.async_hier_loss_bwd(zq, (H, W), small, SS, msk, plain['mult'], plain['any'], None, acc, one)
        _, acc_w = ops.async_hier_loss_fwd(zq, (H, W), small, SS, msk, tmax['mult'], tmax['any'], tmax['wgt'])
        ops.async_hier_loss_bwd(zq, (H, W), small, SS, msk, tmax['mult'], tmax['any'], tmax['wgt'], acc_w, one)
    any_ = plain['any']
    out['pairs'] = int(plain['mult'].sum())
    out['fine_superpixels_with_a_pair'] = int((any_ != 0).sum())
    out['weak_pixels_in_k_hier_weights'] = int((msk_w & (small_w < SS) & (any_.gather(1, small_w.clamp(max=SS - 1).view(N, -1)).view(N, HO, WO) != 0)).sum())
    out['counted_pixels'] = int((msk & (small < SS) & (any_.gather(1, small.clamp(max=SS - 1).view(N, -1)).view(N, H, W) != 0)).sum())
    out['count_n'], out['count_n_weighted'] = int(acc[1]), int(acc_w[1])
    out['pair_tables_of_max_and_mean_equal'] = bool(torch.equal(tmax['mult'], tmean['mult']) and torch.equal(tmax['any'], tmean['any']))
    crit = L.WeightAsyncHierGroupMultiLabelCE(type('A', (), dict(small_nseg=SS))(), C, S, False, -1)
    crit.sync_normalisers = False

    def fused():
        z = zq.detach().clone().requires_grad_(True)
        group = crit.forward_lowres(z, (H, W), zw, (HO, WO), tgt, msk, msk_w, spx, spx_w, small, small_w)
        (16.0 * crit.merged_positive(z, (H, W), spx, msk, T) + group).backward()

    def aten():
        aten_step(torch, zq.detach().clone().requires_grad_(True), zw, tgt[..., :C], spx, small, msk, spx_w, small_w, msk_w)

    out['peak_bytes_forward_lowres_step'] = peak_of(torch, fused)
    out['peak_bytes_aten_on_materialised_logits'] = peak_of(torch, aten)
    out['one_full_resolution_logit_tensor_bytes'] = dict(strong=N * C * H * W * 4, weak=N * C * HO * WO * 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
