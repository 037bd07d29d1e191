"""Time the acquisition scan of the measures beyond BvSB (csrc/uncertainty.hip: k_uncertainty) per pool batch: seeded
quarter-resolution logits [4,20,256,512] scanned at 1024 x 2048 against 2048 superpixels (the benchmark's batch), T = 0.1.

Default: device-event medians of --reps calls after 2 warm-ups of ``ops.uncertainty_accum_lowres`` per measure, of the headline scan
``ops.single_pass_accum_lowres`` on the same tensors, and of both full-resolution forms on the materialised logits; the new scan's
accumulators are checked first (measure = bvsb equals the headline scan's, low-res equals full-res).  One JSON line, --out writes it.

--kernels-only runs, in this order, --reps calls of the headline low-res scan, then --reps low-res calls per measure in the order of
``ops.UNCERTAINTY``, and nothing else; --summarize CSV turns the kernel trace of such a run into per-group medians:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o unc -- python tools/uncertainty_probe.py --kernels-only --reps 20
    python tools/uncertainty_probe.py --summarize OUT/unc_kernel_trace.csv --reps 20
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, HQ, WQ, H, W, NSEG = 4, 20, 256, 512, 1024, 2048, 2048
CE_TEMP = 0.1


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


def key_runs(full, spx, rows=16):
    """Number of (id, arg-max class) runs down the columns of the 16-row tiles: the pairs of global atomics one scan issues."""
    key = spx * 32 + full.argmax(dim=1)
    change = key[:, 1:] != key[:, :-1]
    change[:, rows - 1::rows] = True                 # a tile border ends every run
    return change.sum() + key.shape[0] * key.shape[2]


def summarize(path, reps):
    """Per-group medians (us) of a --kernels-only trace: the headline kernel's dispatches, then k_uncertainty's in measure order."""
    from mulactseg_amd import ops
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = lambda sel: [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if sel(r['Kernel_Name'])]   # noqa: E731
    head, unc = dur(lambda n: 'k_single_pass' in n), dur(lambda n: 'k_uncertainty' in n)
    if len(unc) != reps * len(ops.UNCERTAINTY):
        raise SystemExit("expected %d k_uncertainty dispatches, found %d" % (reps * len(ops.UNCERTAINTY), len(unc)))
    out = {'k_single_pass_lowres_us': float(np.median(head)), 'dispatches_per_group': reps}
    for k, m in enumerate(ops.UNCERTAINTY):
        out['k_uncertainty_%s_us' % m] = float(np.median(unc[k * reps:(k + 1) * reps]))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--summarize', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.summarize is not None:
        return summarize(args.summarize, args.reps)
    import torch
    from mulactseg_amd import ops, synth
    rs = np.random.RandomState(0)
    zq = torch.from_numpy((rs.randn(B, C, HQ, WQ) * 0.5).astype(np.float32)).cuda()
    spx = torch.from_numpy(np.stack([synth.superpixel_map(20 + i, H, W, NSEG) for i in range(B)])).cuda()
    invT = ops.inv_temperature(CE_TEMP)
    bufs = ops.single_pass_accum_lowres(zq, (H, W), spx, NSEG, invT)
    head_low = lambda: ops.single_pass_accum_lowres(zq, (H, W), spx, NSEG, invT, *bufs)                  # noqa: E731
    low = {m: (lambda m=m: ops.uncertainty_accum_lowres(zq, (H, W), spx, NSEG, invT, m, *bufs)) for m in ops.UNCERTAINTY}
    if args.kernels_only:
        for _ in range(args.reps):
            head_low()
        for m in ops.UNCERTAINTY:
            for _ in range(args.reps):
                low[m]()
        torch.cuda.synchronize()
        return
    full = ops.upsample_bilinear(zq, (H, W))
    want = ops.single_pass_accum_lowres(zq, (H, W), spx, NSEG, invT)
    assert all(torch.equal(a, b) for a, b in zip(ops.uncertainty_accum_lowres(zq, (H, W), spx, NSEG, invT, 'bvsb'), want))
    for m in ops.UNCERTAINTY:
        assert all(torch.equal(a, b) for a, b in zip(ops.uncertainty_accum_lowres(zq, (H, W), spx, NSEG, invT, m),
                                                     ops.uncertainty_accum(full, spx, NSEG, invT, m))), m
    row = {'batch': '[%d,%d,%d,%d] -> %dx%d' % (B, C, HQ, WQ, H, W), 'nseg': NSEG, 'ce_temp': CE_TEMP, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0)}
    row['single_pass_lowres_call_ms'] = timed(head_low, args.reps)
    row['single_pass_fullres_call_ms'] = timed(lambda: ops.single_pass_accum(full, spx, NSEG, invT, *bufs), args.reps)
    for m in ops.UNCERTAINTY:
        row['uncertainty_lowres_%s_call_ms' % m] = timed(low[m], args.reps)
        row['uncertainty_fullres_%s_call_ms' % m] = timed(lambda m=m: ops.uncertainty_accum(full, spx, NSEG, invT, m, *bufs), args.reps)
    # the same instruction stream with ONE arg-max class everywhere: a lane's key runs then end at superpixel borders only, so the
    # difference to the row above is the price of the global atomics of the short runs of these random logits
    z1 = zq.clone()
    z1[:, 3] += 8.0
    b1 = ops.uncertainty_accum_lowres(z1, (H, W), spx, NSEG, invT, 'entropy')
    row['uncertainty_lowres_entropy_one_class_call_ms'] = timed(
        lambda: ops.uncertainty_accum_lowres(z1, (H, W), spx, NSEG, invT, 'entropy', *b1), args.reps)
    row['key_runs_per_batch'] = {'random_logits': int(key_runs(ops.upsample_bilinear(zq, (H, W)), spx)),
                                 'one_class': int(key_runs(ops.upsample_bilinear(z1, (H, W)), spx))}
    # the guarded 32-slot instantiation every C outside {19, 20, 21} runs: what a small C pays for it
    for c in (2, 8, 32):
        zc = torch.from_numpy((rs.randn(B, c, HQ, WQ) * 0.5).astype(np.float32)).cuda()
        bc = ops.uncertainty_accum_lowres(zc, (H, W), spx, NSEG, invT, 'entropy')
        row['uncertainty_lowres_entropy_C%d_call_ms' % c] = timed(
            lambda: ops.uncertainty_accum_lowres(zc, (H, W), spx, NSEG, invT, 'entropy', *bc), args.reps)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(row, f, indent=1)


if __name__ == '__main__':
    main()
