"""Time the evaluation of the local-prototype labels inside the queried superpixels (csrc/within_eval.hip: k_within_eval) at the
evaluation geometry: seeded quarter-resolution logits [4,20,256,512] and features [4,256,256,512] at 1024 x 2048 against 2048
superpixels, 9 % of them selected, rows of 1-4 classes.

Default: one JSON line with ``--series`` medians (device events, ``--reps`` calls each after 2 warm-ups) of ``ops.within_multihot_eval``
in both modes and of ``ops.online_pseudo_labels`` (k_online_assign) on the same inputs; the diagnostics; and the peak allocation of one
fused call against the ``MAS_WITHIN_EVAL=aten`` chain on the materialised full-resolution tensors of ONE picture of the batch (the
chain's [N,256,H,W] features of four pictures are 8.6 GB).

--kernels-only runs every call ``--reps`` times and nothing else; with rocprofv3 this gives the kernel trace, the new kernel and the
sibling's in one run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o within -- python tools/within_eval_probe.py --kernels-only --reps 5
    python tools/within_eval_probe.py --summarize OUT/within_kernel_trace.csv
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from online_plbl_probe import P_COUNTS, summarize, timed  # noqa: E402

N, C, CH, HQ, WQ, H, W, NSEG = 4, 20, 256, 256, 512, 1024, 2048, 2048


def inputs():
    import torch
    from mulactseg_amd import synth
    zq = torch.from_numpy(synth.logits(3, N, C, HQ, WQ)).cuda()
    g = torch.Generator().manual_seed(5)
    featq = torch.nn.functional.normalize(torch.randn((N, CH, HQ, WQ), generator=g), dim=1).cuda()
    sm = [synth.train_crop(60 + i, H, W, NSEG, frac_selected=0.09) for i in range(N)]
    spx = torch.from_numpy(np.stack([a for a, _ in sm])).cuda()
    msk = torch.from_numpy(np.stack([b for _, b in sm])).cuda()
    tgt = torch.from_numpy(np.stack([synth.multi_hot_targets(80 + i, NSEG, C, p_counts=P_COUNTS) for i in range(N)])).cuda()
    rs = np.random.RandomState(9)
    gt = torch.from_numpy(np.stack([synth.class_map(90 + i, H, W, C - 1) for i in range(N)]).astype(np.int64))
    gt[torch.from_numpy(rs.random_sample((N, H, W)) < 0.1)] = 255
    return zq, featq, tgt, spx, msk, gt.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--series', type=int, default=3)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--summarize')
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch
    from mulactseg_amd import ops
    zq, featq, tgt, spx, msk, gt = inputs()
    bits = ops.target_bits(tgt)
    size = (H, W)
    counts = torch.zeros(3 * C + 3, dtype=torch.int64, device='cuda')
    diag = torch.zeros(4, dtype=torch.int64, device='cuda')
    calls = {
        'within_proto': lambda: ops.within_multihot_eval(zq, featq, size, spx, msk, gt, bits=bits, mode='proto', counts=counts, diag=diag),
        'within_filt': lambda: ops.within_multihot_eval(zq, featq, size, spx, msk, gt, bits=bits, mode='filt', counts=counts, diag=diag),
        'online_pseudo_labels': lambda: ops.online_pseudo_labels(zq, featq, size, spx, msk, bits=bits, invT=1.0),
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
    _, d, _ = ops.within_multihot_eval(zq, featq, size, spx, msk, gt, bits=bits, mode='filt')
    out.update(selected_pixels=int(msk.sum()), diag_filt=d.tolist(),
               multi_hot_valid_pixels=int((ops.online_pseudo_labels(zq, featq, size, spx, msk, bits=bits, invT=1.0)[0] != 255).sum()))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - before)

    out['peak_bytes_fused_batch_of_4'] = peak(lambda: ops.within_multihot_eval(zq, featq, size, spx, msk, gt, bits=bits))
    tr = object.__new__(importlib.import_module("mulactseg_amd.trainer.eval_cosplbl_within_multihot").ActiveTrainer)

    def chain():
        up = lambda t: torch.nn.functional.interpolate(t, size=size, mode='bilinear', align_corners=False)      # noqa: E731
        lab = tr.pseudo_label_generation(gt[:1], up(featq[:1]), up(zq[:1]), tgt[:1], msk[:1], spx[:1])
        ops.iou_counts(lab.contiguous(), None, gt[:1].contiguous(), C, 255)

    out['peak_bytes_aten_chain_one_picture'] = peak(chain)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
