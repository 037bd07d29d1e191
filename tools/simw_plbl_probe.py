"""Time the similarity-weighted online pseudo labels (csrc/online_plbl.hip: k_online_soft, k_soft_ce_fwd / _bwd, the signed label CE)
at the training geometry of tools/online_plbl_probe.py, whose inputs these are: seeded quarter-resolution logits [4,20,192,192] and
features [4,256,192,192] at 768 x 768 against 2048 superpixels, T = 0.1, tau = 0.1.

Default: one JSON line with ``--series`` medians (device events, ``--reps`` calls each after 2 warm-ups) of ``ops.online_soft_weights``,
``ops.soft_ce_fwd_lowres`` / ``_bwd_lowres``, of ``ops.online_pseudo_labels`` with the similarity weight and the signed label CE, and of
the sibling's calls next to them; the counted-pixel numbers; and the peak allocation of one ``forward_lowres`` + backward of
``JointLocalProtoWeightingCE`` and ``LocalsimWProtoCE`` against ``forward`` on materialised full-resolution tensors.

--kernels-only runs every call ``--reps`` times and nothing else; with rocprofv3 this gives the kernel trace, the new kernels and the
sibling's in one run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o simw -- python tools/simw_plbl_probe.py --kernels-only --reps 10
    python tools/simw_plbl_probe.py --summarize OUT/simw_kernel_trace.csv
"""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from online_plbl_probe import H, NSEG, TEMP, W, inputs, summarize, timed  # noqa: E402

TAU = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--series', type=int, default=3)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--summarize')
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch
    from mulactseg_amd import ops
    from mulactseg_amd.utils import loss as L
    zq_p, featq, zq, tgt, spx, msk = inputs()
    invT, inv_tau = ops.inv_temperature(TEMP), ops.inv_temperature(TAU)
    bits = ops.target_bits(tgt)
    mask = msk.view(torch.uint8)
    size = (H, W)
    one = torch.ones(1, device='cuda')
    labels, weight = ops.online_pseudo_labels(zq_p, featq, size, spx, msk, bits=bits, invT=invT)
    labels_s, weight_s = ops.online_pseudo_labels(zq_p, featq, size, spx, msk, bits=bits, invT=invT, weight_sim=True)
    assert torch.equal(labels, labels_s)
    softw, live, _ = ops.online_soft_weights(zq_p, featq, size, spx, msk, bits=bits, invT=invT, inv_tau=inv_tau)
    signed = ops.LCE_WEIGHTED | ops.LCE_SIGNED
    _, acc = ops.label_ce_fwd_lowres(zq, size, labels, weight, invT, ops.LCE_WEIGHTED)
    _, acc_s = ops.label_ce_fwd_lowres(zq, size, labels, weight_s, invT, signed)
    _, acc_soft = ops.soft_ce_fwd_lowres(zq, size, spx, mask, bits, softw, live, invT)
    calls = {
        'pseudo_labels': lambda: ops.online_pseudo_labels(zq_p, featq, size, spx, msk, bits=bits, invT=invT),
        'pseudo_labels_sim': lambda: ops.online_pseudo_labels(zq_p, featq, size, spx, msk, bits=bits, invT=invT, weight_sim=True),
        'soft_weights': lambda: ops.online_soft_weights(zq_p, featq, size, spx, msk, bits=bits, invT=invT, inv_tau=inv_tau),
        'label_ce_fwd': lambda: ops.label_ce_fwd_lowres(zq, size, labels, weight, invT, ops.LCE_WEIGHTED),
        'label_ce_bwd': lambda: ops.label_ce_bwd_lowres(zq, size, labels, weight, acc, one, invT, ops.LCE_WEIGHTED),
        'signed_ce_fwd': lambda: ops.label_ce_fwd_lowres(zq, size, labels, weight_s, invT, signed),
        'signed_ce_bwd': lambda: ops.label_ce_bwd_lowres(zq, size, labels, weight_s, acc_s, one, invT, signed),
        'soft_ce_fwd': lambda: ops.soft_ce_fwd_lowres(zq, size, spx, mask, bits, softw, live, invT),
        'soft_ce_bwd': lambda: ops.soft_ce_bwd_lowres(zq, size, spx, mask, bits, softw, live, acc_soft, one, invT),
    }
    if args.kernels_only:
        for _ in range(args.reps):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        return
    res = {k: [] for k in calls}
    for _ in range(args.series):
        for k, fn in calls.items():
            res[k].append(timed(fn, args.reps) * 1e3)
    out = {k + '_us': round(float(np.median(v)), 1) for k, v in res.items()}
    out.update(labelled_pixels=int((labels != 255).sum()), negative_weights=int((weight_s < 0).sum()), selected_pixels=int(msk.sum()),
               signed_ce_counted=int(acc_s[1]), label_ce_counted=int(acc[1]), soft_ce_counted=int(acc_soft[1]), live=live.tolist(),
               softw_bytes=softw.numel() * 4)
    ns = types.SimpleNamespace(nseg=NSEG, weight_wo_proto=False, th_wplbl=None, ce_temp=TEMP, simw_temp=TAU)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - before)

    for name, cls in (('pwce', L.JointLocalProtoWeightingCE), ('simw', L.LocalsimWProtoCE)):
        crit = cls(ns, NSEG, TEMP)

        def low():
            z = zq.clone().requires_grad_(True)
            crit.forward_lowres(zq_p, featq, z, size, tgt, spx, msk).backward()

        def full():
            z = zq.clone().requires_grad_(True)
            up = lambda t: torch.nn.functional.interpolate(t, size=size, mode='bilinear', align_corners=False)      # noqa: E731
            crit(up(zq_p), up(featq), up(z), tgt, spx, msk).backward()

        out['peak_bytes_%s_forward_lowres' % name] = peak(low)
        out['peak_bytes_%s_forward_materialised' % name] = peak(full)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
