"""Probe of the teacher-weighted group scans (csrc/teacher_terms.h, wgroup) on the siblings' batch: quarter-resolution logits
[4,20,192,192] scanned at 768 x 768 against 2048 superpixels.  Runs, ``--reps`` times each, the forward and the backward scan of

  top1      merged positive + group + the teacher-gated top-1 term (the scans of profiles/teacher_terms/)
  wgroup    merged positive + the teacher-weighted group term: forward scan, weighted finalize, backward scan

so that one ``rocprofv3 --kernel-trace --stats -- python tools/wgroup_probe.py`` run (kernel trace only, a run of its own) times them
side by side, and reports (JSON on stdout) the allocator peak of a ``FusedWGroupLoss.forward_lowres`` step against the ATen
composition of the same two terms on materialised logits."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mulactseg_amd import ops, synth  # noqa: E402
from mulactseg_amd.utils import loss as L  # noqa: E402

N, C, h, w, S, T = 4, 20, 192, 192, 2048, 0.1
H, W = 4 * h, 4 * w
EPS = 1e-8


def aten_step(zq, tq, tgt, spx, msk):
    """pos + the weighted group term on the materialised logits with ATen ops (scatter_reduce for the two max-pools)"""
    z = torch.nn.functional.interpolate(zq, size=(H, W), mode='bilinear', align_corners=False)
    with torch.no_grad():
        t = torch.nn.functional.interpolate(tq, size=(H, W), mode='bilinear', align_corners=False)
    total = 0
    for i in range(N):
        m = msk[i].reshape(-1)
        ids = spx[i].reshape(-1)[m]
        y = tgt[i][ids].float()
        p = torch.softmax(z[i].permute(1, 2, 0).reshape(H * W, C)[m] / T, dim=1)
        total = total + (-torch.log((p * y).sum(dim=1) + EPS)).sum()
        index = ids[:, None].expand(-1, C)
        pool = torch.zeros((S, C), device=p.device).scatter_reduce(0, index, p, 'amax', include_self=True) * tgt[i].float()
        with torch.no_grad():
            q = torch.softmax(t[i].permute(1, 2, 0).reshape(H * W, C)[m] / T, dim=1)
            wt = torch.zeros((S, C), device=p.device).scatter_reduce(0, index, q, 'amax', include_self=True)
        nz = pool > 0
        total = total + (wt[nz] * -torch.log(pool[nz] + EPS)).sum()
    total.backward()


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    zq = torch.from_numpy(synth.logits(3, N, C, h, w)).cuda()
    tq = torch.from_numpy(synth.logits(4, N, C, h, w)).cuda()
    crops = [synth.train_crop(50 + i, H, W, S, frac_selected=0.08) for i in range(N)]
    spx = torch.from_numpy(np.stack([c[0] for c in crops])).cuda()
    msk = torch.from_numpy(np.stack([c[1] for c in crops])).cuda()
    tgt = torch.from_numpy(np.stack([synth.multi_hot_targets(70 + i, S, C) for i in range(N)])).cuda()
    bits = ops.target_bits(tgt)
    invT, one = ops.inv_temperature(T), ops.inv_temperature(1.0)
    go3, go4 = torch.tensor([16.0, 0.0, 1.0], device='cuda'), torch.tensor([16.0, 0.0, 1.0, 1.0], device='cuda')
    base = ops.LOSS_CE | ops.LOSS_GROUP
    out = dict(shape=[N, C, h, w, H, W, S], selected=int(msk.sum()))
    for _ in range(a.reps):
        _, acc, gmax = ops.teacher_loss_fwd(zq, tq, (H, W), spx, msk, bits, invT, one, 0.05, base | ops.LOSS_TOP1)
        ops.teacher_loss_bwd(zq, tq, (H, W), spx, msk, bits, gmax, acc, go4, invT, one, 0.05, base | ops.LOSS_TOP1)
        _, acc, gmax, tmax = ops.wgroup_loss_fwd(zq, tq, (H, W), spx, msk, bits, invT, base | ops.LOSS_WGROUP)
        ops.wgroup_loss_bwd(zq, tq, (H, W), spx, msk, bits, gmax, tmax, acc, go3, invT, base | ops.LOSS_WGROUP)
        out['group_entries'] = int(acc[6])
    crit = L.FusedWGroupLoss(S, T, T, sync_normalisers=False)

    def fused():
        z = zq.detach().clone().requires_grad_(True)
        pos, group = crit.forward_lowres(z, tq, (H, W), tgt, spx, msk)
        (16.0 * pos + group).backward()

    def aten():
        z = zq.detach().clone().requires_grad_(True)
        aten_step(z, tq, tgt, spx, msk)

    out['peak_bytes_forward_lowres_step'] = peak_of(fused)
    out['peak_bytes_aten_on_materialised_logits'] = peak_of(aten)
    out['one_full_resolution_logit_tensor_bytes'] = N * C * H * W * 4
    print(json.dumps(out))


if __name__ == "__main__":
    main()
