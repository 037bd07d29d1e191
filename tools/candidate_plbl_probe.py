"""Time the stage-2 label kernel without expansion per 1024 x 2048 picture on a seeded, randomly initialised
deeplabv3pluswn_resnet50deepstem (20 output channels), one seeded picture, 2048 superpixels, 20 % of them selected, seeded multi-hot rows.

Device-event medians of --reps repetitions after 2 warm-ups, the two sides of each pair alternating in one process:
``k_candidate_plbl`` (ops.candidate_pseudo_labels) in candidate mode with the fallback off, and with the fallback on and the counters,
against the ATen chain of the same call (``MAS_CANDIDATE_PLBL=aten``: upsample, gather of the rows, product, max, softmax, the counters);
``ops.stage2_pseudo_labels`` with ``expand=True`` and ``expand=False``.  Kernel and chain must give the same labels away from the
threshold (asserted).  Also the allocator peak of both sides (``torch.cuda.max_memory_allocated`` over one call) and the kernel's byte
floor at the HBM peak.  --kernels-only runs every side --reps times and nothing else (for a rocprofv3 kernel trace).

    python tools/candidate_plbl_probe.py --out profiles/candidate_plbl/candidate_plbl_probe.json
    rocprofv3 --kernel-trace --stats -d OUT -o cpl -- python tools/candidate_plbl_probe.py --kernels-only --reps 20
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, C, NSEG, K = 1024, 2048, 20, 2048, 20
TH, CE_TEMP = 0.1, 0.1
HBM_PEAK = 8.0e12                            # MI355X HBM3E, bytes/s


def timed_pair(fa, fb, reps, warmup=2):
    """Medians (ms) of the two sides, alternating a, b, a, b, ..."""
    import torch
    for _ in range(warmup):
        fa(), fb()
    ts = ([], [])
    for _ in range(reps):
        for side, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[side].append(a.elapsed_time(b))
    return float(np.median(ts[0])), float(np.median(ts[1]))


def peak_of(fn):
    """Bytes the allocator held at most during one call, above what was held before it."""
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from mulactseg_amd import ops, synth
    from mulactseg_amd.models import get_model
    torch.manual_seed(0)
    net = get_model('deeplabv3pluswn_resnet50deepstem', C, 16, True, pretrained_backbone=False).cuda().eval()
    rs = np.random.RandomState(0)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).cuda(), torch.tensor([0.229, 0.224, 0.225]).cuda()
    image = ((torch.from_numpy(rs.randint(0, 256, size=(3, H, W)).astype(np.float32)).cuda() / 255 - mean[:, None, None]) /
             std[:, None, None])[None].contiguous()
    spx = torch.from_numpy(synth.superpixel_map(11, H, W, NSEG).astype(np.int64)).cuda()[None].contiguous()
    rows = torch.from_numpy(np.stack([synth.multi_hot_targets(7, NSEG, C, p_counts=(0.5, 0.3, 0.15, 0.05))])).cuda()
    spmask = torch.from_numpy(rs.uniform(size=NSEG) < 0.2).cuda()[spx].contiguous()
    labels = torch.from_numpy(rs.randint(0, C - 1, size=(1, H, W)).astype(np.int64)).cuda()
    counts = torch.zeros(3 * K + 3, dtype=torch.int64, device='cuda')

    def side(aten, fallback):
        def run():
            os.environ['MAS_CANDIDATE_PLBL'] = 'aten' if aten else 'fused'
            kw = dict(fallback=True, th=TH, ce_temp=CE_TEMP, targets=labels, counts=counts, num_classes=K) if fallback else {}
            return ops.candidate_pseudo_labels(zq, (H, W), spmask, targets_rows=rows, superpixels=spx, **kw)
        return run
    with torch.no_grad():
        feats, zq = net.feat_forward_quarter(image)
        feats, zq = feats.contiguous(), zq.contiguous()
        z_full = ops.upsample_bilinear(zq, (H, W))
        k_off, a_off, k_on, a_on = side(False, False), side(True, False), side(False, True), side(True, True)
        expand = lambda: ops.stage2_pseudo_labels(feats, z_full, rows, spmask, spx, include_onehot=True)                    # noqa: E731
        assign = lambda: ops.stage2_pseudo_labels(feats, z_full, rows, spmask, spx, include_onehot=True, expand=False)      # noqa: E731
        if args.kernels_only:
            for _ in range(args.reps):
                k_off(), a_off(), k_on(), a_on(), expand(), assign()
            torch.cuda.synchronize()
            return
        # the same labels: exactly with the fallback off, away from the threshold with it
        assert torch.equal(k_off(), a_off())
        got, ref = k_on(), a_on()
        p = 1.0 / torch.exp((z_full.double() - z_full.double().amax(dim=1, keepdim=True)) * ops.inv_temperature(CE_TEMP)).sum(dim=1)
        far = spmask | ((p - TH).abs() > 1e-6)
        assert bool((~far).float().mean() <= 1e-3) and torch.equal(got[far], ref[far])
        assert torch.equal(torch.where(spmask, expand(), torch.full_like(got, 255)), assign())
        kept = float(((got != 255) & ~spmask).sum() / (~spmask).sum())
        row = {'picture': '%dx%d' % (W, H), 'C': C, 'nseg': NSEG, 'selected_fraction': float(spmask.float().mean()),
               'th': TH, 'ce_temp': CE_TEMP, 'fallback_kept_fraction_of_unselected': kept,
               'pixels_within_1e-6_of_th': int((~far).sum())}
        row['candidate_kernel_ms'], row['candidate_aten_ms'] = timed_pair(k_off, a_off, args.reps)
        row['candidate_fallback_counts_kernel_ms'], row['candidate_fallback_counts_aten_ms'] = timed_pair(k_on, a_on, args.reps)
        row['stage2_expand_ms'], row['stage2_assign_only_ms'] = timed_pair(expand, assign, args.reps)
        row['peak_alloc_MB'] = {name: peak_of(fn) / 1e6 for name, fn in (('candidate_kernel', k_off), ('candidate_aten', a_off),
                                                                        ('candidate_fallback_counts_kernel', k_on),
                                                                        ('candidate_fallback_counts_aten', a_on))}
        h, w = zq.shape[2:]
        floor_off = 4 * C * h * w + (1 + 1) * H * W + 8 * int(spmask.sum()) + 4 * NSEG       # logits, mask, labels, ids under the mask, rows
        floor_on = floor_off + 8 * H * W                                                    # + the int64 targets of the counters
        row.update({'byte_floor_MB': floor_off / 1e6, 'floor_us_at_peak': 1e6 * floor_off / HBM_PEAK,
                    'byte_floor_fallback_counts_MB': floor_on / 1e6, 'floor_fallback_counts_us_at_peak': 1e6 * floor_on / HBM_PEAK})
    os.environ.pop('MAS_CANDIDATE_PLBL', None)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'rows': [row]}, f, indent=1)


if __name__ == '__main__':
    main()
