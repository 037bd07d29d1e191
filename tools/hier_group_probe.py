"""Probe of the hierarchical group term (csrc/hier_group.h; k_hier_pairs, k_hier_fwd / _bwd of csrc/online_plbl.hip) on the siblings'
batch: quarter-resolution logits [4,19,192,192] at 768 x 768 against 2048 superpixels and a seeded fine map of 8192 ids.  Runs,
``--reps`` times each,

  soft_ce   ``ops.soft_ce_fwd_lowres`` / ``_bwd_lowres`` (k_soft_ce_fwd / _bwd, the closest relative: the same tile-queue core)
  hier      ``ops.hier_group_loss_fwd`` / ``_bwd`` (memsets, the group scan, k_hier_pairs, k_hier_fwd; k_hier_bwd)

so that one ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/hier_group_probe.py`` run (kernel trace only, a run
of its own) times them side by side (``--summarize <kernel trace csv>`` prints the per-kernel medians), and reports (JSON on stdout)
the counted pixels of both, and the allocator peak of a ``forward_lowres`` step (group term + merged positive) against the ATen
composition of the same two terms on materialised logits."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from online_plbl_probe import summarize  # noqa: E402

N, C, CH, h, w, S, SS, T = 4, 19, 256, 192, 192, 2048, 8192, 0.1
H, W = 4 * h, 4 * w
EPS = 1e-8


def aten_step(torch, zq, tgt, spx, small, msk):
    """merged positive + the hierarchical group term on the materialised logits with ATen ops (scatter_reduce / index_add per picture)"""
    z = torch.nn.functional.interpolate(zq, size=(H, W), mode='bilinear', align_corners=False)
    total, n = 0, 1
    for i in range(N):
        m = msk[i].reshape(-1)
        ids, fine = spx[i].reshape(-1)[m], small[i].reshape(-1)[m]
        zi = z[i].permute(1, 2, 0).reshape(H * W, C)[m]
        y = tgt[i][ids].float()
        total = total + 16.0 * (-torch.log((torch.softmax(zi / T, dim=1) * y).sum(dim=1) + EPS)).sum()
        p = torch.softmax(zi, dim=1)
        index = ids[:, None].expand(-1, C)
        best = torch.zeros((S, C), device=p.device).scatter_reduce(0, index, p.detach(), 'amax', include_self=True)
        is_arg = (p.detach() == best[ids]) & (tgt[i][ids] != 0)                 # (ties count twice here: a memory probe, not a reference)
        mult = torch.zeros((SS, C), device=p.device).index_add_(0, fine, is_arg.float())
        wgt = mult[fine]
        total = total + (wgt * -torch.log(p + EPS)).sum()
        n = n + wgt.sum()
    (total / n).backward()


def peak_of(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


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
    zq_p = torch.from_numpy(synth.logits(4, N, C, h, w)).cuda()
    g = torch.Generator().manual_seed(5)
    featq = torch.nn.functional.normalize(torch.randn((N, CH, h, w), generator=g), dim=1).cuda()
    crops = [synth.train_crop(50 + i, H, W, S, frac_selected=0.08) for i in range(N)]
    spx_h = np.stack([c[0] for c in crops])
    small_h = np.stack([synth.superpixel_map(90 + i, H, W, SS) for i in range(N)])
    small_h[spx_h == S] = SS
    spx, small = torch.from_numpy(spx_h).cuda(), torch.from_numpy(small_h).cuda()
    msk = torch.from_numpy(np.stack([c[1] for c in crops])).cuda()
    tgt = torch.from_numpy(np.stack([synth.multi_hot_targets(70 + i, S, C + 1, p_counts=(0.40, 0.35, 0.15, 0.10)) for i in range(N)])).cuda()
    tgt[..., -1] = 0
    bits = ops.target_bits(tgt, C)
    mask = msk.view(torch.uint8)
    invT, one = ops.inv_temperature(T), torch.ones(1, device='cuda')
    softw, live, _ = ops.online_soft_weights(zq_p, featq, (H, W), spx, msk, bits=bits, invT=invT, inv_tau=invT)
    out = dict(shape=[N, C, h, w, H, W, S, SS], selected=int(msk.sum()))
    for _ in range(a.reps):
        _, acc_soft = ops.soft_ce_fwd_lowres(zq, (H, W), spx, mask, bits, softw, live, invT)
        ops.soft_ce_bwd_lowres(zq, (H, W), spx, mask, bits, softw, live, acc_soft, one, invT)
        f = ops.hier_group_loss_fwd(zq, (H, W), spx, small, SS, msk, bits)
        ops.hier_group_loss_bwd(zq, (H, W), small, SS, msk, f['mult'], f['any'], f['acc'], one)
    out['soft_ce_counted_pixels'] = int(acc_soft[1])
    out['hier_count_n'] = int(f['acc'][1])
    out['hier_pairs'] = int(f['mult'].sum())
    out['hier_counted_pixels'] = int((msk & (small < SS) & (f['any'].view(N, SS).gather(1, small.clamp(max=SS - 1).view(N, -1)).view(N, H, W) != 0)).sum())
    crit = L.HierGroupMultiLabelCE(type('A', (), dict(small_nseg=SS))(), C, S, False, -1)
    crit.sync_normalisers = False

    def fused():
        z = zq.detach().clone().requires_grad_(True)
        group = crit.forward_lowres(z, (H, W), tgt, msk, spx, small)
        (16.0 * crit.merged_positive(z, (H, W), spx, msk, T) + group).backward()

    def aten():
        aten_step(torch, zq.detach().clone().requires_grad_(True), tgt[..., :C], spx, small, msk)

    out['peak_bytes_forward_lowres_step'] = peak_of(torch, fused)
    out['peak_bytes_aten_on_materialised_logits'] = peak_of(torch, aten)
    out['one_full_resolution_logit_tensor_bytes'] = N * C * H * W * 4
    print(json.dumps(out))


if __name__ == "__main__":
    main()
