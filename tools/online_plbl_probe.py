"""Time the online local-prototype pseudo labels (csrc/online_plbl.hip) at the training geometry: seeded quarter-resolution logits
[4,20,192,192] and features [4,256,192,192] labelled at 768 x 768 against 2048 superpixels, T = 0.1.

Default: one JSON line with ``--series`` medians (device events, ``--reps`` calls each after 2 warm-ups) of ``ops.online_pseudo_labels``,
``ops.label_ce_fwd_lowres`` and ``ops.label_ce_bwd_lowres`` (weighted mode), of the merged-positive scans next to them, and the peak
allocation of one ``LocalWProtoCE.forward_lowres`` + backward against ``forward`` on materialised full-resolution tensors.

--step times whole training steps (device events around ``--reps`` steps after 2 warm-ups, batch 4 x 768 x 768, synthetic pictures) of
``active_onlinewplbl_multi_predignore`` and of ``active_joint_multi_predignore``.

--kernels-only runs ``--reps`` times: merged-positive forward + backward scans, pseudo labels, label CE forward + backward, and nothing
else; with rocprofv3 this gives the kernel trace of the losses of one step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o opl -- python tools/online_plbl_probe.py --kernels-only --reps 10
    python tools/online_plbl_probe.py --summarize OUT/opl_kernel_trace.csv
"""
import argparse
import csv
import json
import logging
import os
import re
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, CH, HQ, WQ, H, W, NSEG = 4, 20, 256, 192, 192, 768, 768, 2048
TEMP = 0.1
P_COUNTS = (0.40, 0.35, 0.15, 0.10)


def timed(fn, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def inputs():
    import torch
    from mulactseg_amd import synth
    zq_p = torch.from_numpy(synth.logits(3, N, C, HQ, WQ)).cuda()
    zq = torch.from_numpy(synth.logits(4, N, C, HQ, WQ)).cuda()
    g = torch.Generator().manual_seed(5)
    featq = torch.nn.functional.normalize(torch.randn((N, CH, HQ, WQ), generator=g), dim=1).cuda()
    sm = [synth.train_crop(60 + i, H, W, NSEG, frac_selected=0.09) for i in range(N)]
    spx = torch.from_numpy(np.stack([a for a, _ in sm])).cuda()
    msk = torch.from_numpy(np.stack([b for _, b in sm])).cuda()
    tgt = torch.from_numpy(np.stack([synth.multi_hot_targets(80 + i, NSEG, C, p_counts=P_COUNTS) for i in range(N)])).cuda()
    return zq_p, featq, zq, tgt, spx, msk


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        m = re.search(r'\bk_\w+', r['Kernel_Name'])
        name = m.group(0) if m else r['Kernel_Name'].split('(')[0][:48]
        out.setdefault(name, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print(json.dumps({k: {'calls': len(v), 'median_us': round(float(np.median(v)), 2)} for k, v in sorted(out.items())}))


class _Train:
    selection_iter = 1

    def __len__(self):
        return N

    def __getitem__(self, i):
        import torch
        from mulactseg_amd import synth
        rs = np.random.RandomState(100 + i)
        spx, msk = synth.train_crop(200 + i, H, W, NSEG, frac_selected=0.09)
        return {'images': torch.from_numpy(rs.standard_normal((3, H, W)).astype(np.float32)),
                'labels': torch.from_numpy(synth.multi_hot_targets(300 + i, NSEG, C, p_counts=P_COUNTS)),
                'spx': torch.from_numpy(spx), 'spmask': torch.from_numpy(msk)}


class _Val:
    def __len__(self):
        return 1

    def __getitem__(self, i):
        import torch
        return {'images': torch.zeros((3, 64, 64)), 'labels': torch.zeros((64, 64), dtype=torch.int64)}


def step_cost(method, reps):
    """median milliseconds of one training step of ``method`` (events on the training stream at the start of consecutive steps)"""
    import importlib
    import torch
    from mulactseg_amd import dataloader
    from mulactseg_amd.utils import common
    a = common.get_parser().parse_args([
        '-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--method', method, '--multi_ce_temp', '0.1', '--group_ce_temp', '0.1',
        '--coeff', '16.0', '--nseg', str(NSEG), '--num_classes', str(C - 1), '--train_batch_size', str(N), '--num_workers', '0',
        '--val_num_workers', '0', '--train_lr', '2e-5', '--finetune_itrs', str(reps + 3), '--val_period', '100000', '--log_period', '100000',
        '-p', tempfile.mkdtemp()])
    a.pretrained_backbone = False
    dataloader.register_dataset_factory(lambda args, name, data_root, datalist, imageset: _Val())
    torch.manual_seed(0)
    tr = importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer(a, logging.getLogger("probe"), 1)
    tr._wandb_log = lambda payload, step: None
    batch, marks = tr._batch, []

    def _batch():
        b = batch()
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append(e)
        return b

    tr._batch = _batch
    tr.train(types.SimpleNamespace(selection_iter=1, get_trainset=lambda: _Train()))
    torch.cuda.synchronize()
    ts = [marks[i].elapsed_time(marks[i + 1]) for i in range(2, len(marks) - 1)]
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--series', type=int, default=3)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--summarize')
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch
    from mulactseg_amd import ops
    from mulactseg_amd.utils import loss as L
    if args.step:
        out = {m: round(step_cost(m, args.reps), 2) for m in ('active_joint_multi_predignore', 'active_onlinewplbl_multi_predignore')}
        print(json.dumps({'step_ms': out, 'batch': [N, 3, H, W], 'reps': args.reps}))
        return
    zq_p, featq, zq, tgt, spx, msk = inputs()
    invT = ops.inv_temperature(TEMP)
    bits = ops.target_bits(tgt)
    size = (H, W)
    one = torch.ones(1, device='cuda')
    labels, weight = ops.online_pseudo_labels(zq_p, featq, size, spx, msk, bits=bits, invT=invT)
    _, acc = ops.label_ce_fwd_lowres(zq, size, labels, weight, invT, ops.LCE_WEIGHTED)
    _, st = ops.partial_loss_fwd_fused(zq, size, spx, msk, invT, ops.LOSS_CE, bits=bits)
    calls = {
        'pos_fwd': lambda: ops.partial_loss_fwd_fused(zq, size, spx, msk, invT, ops.LOSS_CE, bits=bits),
        'pos_bwd': lambda: ops.partial_loss_bwd_fused(zq, size, spx, msk, st, torch.ones(3, device='cuda'), invT),
        'pseudo_labels': lambda: ops.online_pseudo_labels(zq_p, featq, size, spx, msk, bits=bits, invT=invT),
        'label_ce_fwd': lambda: ops.label_ce_fwd_lowres(zq, size, labels, weight, invT, ops.LCE_WEIGHTED),
        'label_ce_bwd': lambda: ops.label_ce_bwd_lowres(zq, size, labels, weight, acc, one, invT, ops.LCE_WEIGHTED),
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
    out['labelled_pixels'] = int((labels != 255).sum())
    out['selected_pixels'] = int(msk.sum())
    crit = L.LocalWProtoCE(types.SimpleNamespace(nseg=NSEG, weight_wo_proto=False, th_wplbl=None), NSEG, TEMP)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - before)

    def low():
        z = zq.clone().requires_grad_(True)
        crit.forward_lowres(zq_p, featq, z, size, tgt, spx, msk).backward()

    def full():
        z = zq.clone().requires_grad_(True)
        up = lambda t: torch.nn.functional.interpolate(t, size=size, mode='bilinear', align_corners=False)      # noqa: E731
        crit(up(zq_p), up(featq), up(z), tgt, spx, msk).backward()

    out['peak_bytes_forward_lowres'] = peak(low)
    out['peak_bytes_forward_materialised'] = peak(full)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
