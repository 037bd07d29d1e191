"""Time the counters of multi-scale + flip evaluation (--method eval_naive_ms) per picture: ops.ms_iou_counts fused (csrc/ms_naive.hip,
evaluation mode) and as the ATen chain (MAS_MS_EVAL=aten: upsample_bilinear, flip, F.interpolate, adds, / n, then
ops.logits_iou_counts) on the same seeded quarter-resolution logits of the ten default copies (five scales, then the same flipped):
one 1024 x 2048 picture of a 20-channel model (Cityscapes, K = 19) and one 500 x 375 picture of a 22-channel model (VOC, K = 21).

Per picture (device events, median of --reps, each path warmed up first; the two paths alternate): the fused op, the ATen chain, the
peak of the caching allocator above the inputs during one call of each (what the chain materialises and the kernel does not), the
fused kernel's byte floor from the shapes, and whether the two paths count the same.  --forwards also times the ten
quarter-resolution forwards of a seeded, randomly initialised deeplabv3pluswn_resnet50deepstem on a seeded picture.  --kernels-only runs
both paths --reps times and nothing else (for a rocprofv3 kernel trace).

    python tools/ms_eval_probe.py --forwards --out profiles/ms_eval/ms_eval_probe.json
    rocprofv3 --kernel-trace --stats -d OUT -o mse -- python tools/ms_eval_probe.py --kernels-only --reps 20
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PICTURES = ((1024, 2048, 20, 19), (375, 500, 22, 21))       # (H, W, CH, K)
FACTORS = (0.5, 0.75, 1.0, 1.25, 1.5)
HBM_PEAK = 8.0e12                                            # MI355X HBM3E, bytes/s


def quarter(n):
    return ((n - 1) // 2) // 2 + 1


def byte_floor(sizes, CH, H, W):
    """Bytes the fused kernel cannot avoid: every quarter-resolution logit read once and the int64 targets read once (the counters
    are 3K+3 words)."""
    return 4 * sum(CH * quarter(hs) * quarter(ws) for hs, ws in sizes) + 8 * H * W


def chain_bytes(sizes, CH, H, W):
    """Bytes of the tensors the ATen chain materialises per picture: every source at its scaled size, every source at the picture's
    size, the running sum after each add and the mean (flips are views until the resize reads them)."""
    n = len(sizes)
    return 4 * CH * (sum(hs * ws for hs, ws in sizes) + (2 * n) * H * W)


def timed_pair(fa, fb, reps, warmup=2):
    """Medians (ms) of two callables timed alternately with device events."""
    import torch
    for _ in range(warmup):
        fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return float(np.median(ta)), float(np.median(tb)), float(np.min(ta)), float(np.max(ta)), float(np.min(tb)), float(np.max(tb))


def peak_above(fn):
    """Peak of the caching allocator during fn() above what is allocated before it, in bytes."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--forwards', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from mulactseg_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ms_eval_probe measures on the GPU: no ROCm device is visible")
    rows = []
    for H, W, CH, K in PICTURES:
        rs = np.random.RandomState(H * 1000 + W)
        sizes = [(int(f * H), int(f * W)) for _ in (False, True) for f in FACTORS]
        flips = [k >= len(FACTORS) for k in range(2 * len(FACTORS))]
        zs = [torch.from_numpy(rs.randn(1, CH, quarter(hs), quarter(ws)).astype(np.float32)).cuda() for hs, ws in sizes]
        t = rs.randint(0, K, size=(1, H, W))
        t[rs.uniform(size=t.shape) < 0.1] = 255
        targets = torch.from_numpy(t).cuda()
        counts = torch.zeros(3 * K + 3, dtype=torch.int64, device='cuda')

        def fused(c=counts):
            return ops.ms_iou_counts(zs, sizes, flips, (H, W), targets, K, 255, counts=c)

        def aten(c=counts):
            os.environ["MAS_MS_EVAL"] = "aten"
            try:
                return ops.ms_iou_counts(zs, sizes, flips, (H, W), targets, K, 255, counts=c)
            finally:
                os.environ.pop("MAS_MS_EVAL", None)
        if args.kernels_only:
            for _ in range(args.reps):
                fused(), aten()
            torch.cuda.synchronize()
            continue
        cf, ca = fused(torch.zeros_like(counts)), aten(torch.zeros_like(counts))
        f_ms, a_ms, f_lo, f_hi, a_lo, a_hi = timed_pair(fused, aten, args.reps)
        floor = byte_floor(sizes, CH, H, W)
        row = {'picture': '%dx%d' % (W, H), 'channels': CH, 'sources': len(sizes),
               'fused_ms': f_ms, 'fused_ms_min_max': [f_lo, f_hi], 'aten_ms': a_ms, 'aten_ms_min_max': [a_lo, a_hi],
               'aten_over_fused': a_ms / f_ms,
               'counters_equal': bool(torch.equal(cf, ca)), 'counters_abs_diff_sum': int((cf - ca).abs().sum()), 'pixels': H * W,
               'fused_peak_bytes_above_inputs': peak_above(fused), 'aten_peak_bytes_above_inputs': peak_above(aten),
               'aten_chain_materialised_MB_from_shapes': chain_bytes(sizes, CH, H, W) / 1e6,
               'fused_byte_floor_MB': floor / 1e6, 'fused_floor_us_at_peak': 1e6 * floor / HBM_PEAK,
               'fused_share_of_hbm_peak': floor / (f_ms * 1e-3) / HBM_PEAK}
        if args.forwards:
            from mulactseg_amd.dataloader.device_transforms import DeviceMultiScaleFlip
            from mulactseg_amd.models import get_model
            torch.manual_seed(0)
            net = get_model('deeplabv3pluswn_resnet50deepstem', CH, 16, True, pretrained_backbone=False).cuda().eval()
            pic = torch.from_numpy(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda()
            images = DeviceMultiScaleFlip(FACTORS)(pic)
            with torch.no_grad():
                def forwards():
                    return [net(im[None], lowres=True) for im in images]
                f2, _, lo, hi, _, _ = timed_pair(forwards, lambda: None, max(3, args.reps // 4), warmup=1)
            row.update({'forwards_ms': f2, 'forwards_ms_min_max': [lo, hi], 'fused_share_of_picture': f_ms / (f2 + f_ms)})
            del net, images
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
