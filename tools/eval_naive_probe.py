"""Time the evaluation of ``--method eval_naive`` per 1024 x 2048 picture on a seeded, randomly initialised
deeplabv3pluswn_resnet50deepstem with 20 output channels (C + 1, C = 19), a seeded picture and seeded labels (10 % ignore).

Per picture (device events, median of --reps): the quarter-resolution forward, ``k_lowres_iou`` (ops.lowres_iou_counts) against the
chain it replaces (``k_upsample_fwd`` + ``k_logits_iou``: ops.upsample_bilinear + ops.logits_iou_counts), and one step of the
evaluation loop on each path (host clock, synchronised: forward + counters; ``LowresLogitsIoU.step_lowres`` on ``net(x, lowres=True)``
against ``LogitsIoU.step`` on ``net(x)``) with the peak of allocated device memory of each step.  Also the byte floors of both at the
HBM peak.  The counters of the two chains are compared.  --kernels-only runs the two counting chains --reps times and nothing else
(for a rocprofv3 kernel trace).

    python tools/eval_naive_probe.py --out profiles/eval_naive/eval_naive_probe.json
    rocprofv3 --kernel-trace --stats -d OUT -o evn -- python tools/eval_naive_probe.py --kernels-only --reps 20
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, C = 1024, 2048, 19
CH = C + 1
HBM_PEAK = 8.0e12                            # MI355X HBM3E, bytes/s


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


def host_timed(fn, reps, warmup=2):
    """(median ms on the host clock, peak allocated MB above what was allocated before the step)."""
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), (torch.cuda.max_memory_allocated() - base) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from mulactseg_amd import ops
    from mulactseg_amd.models import get_model
    from mulactseg_amd.utils.miou import LogitsIoU, LowresLogitsIoU
    torch.manual_seed(0)
    net = get_model('deeplabv3pluswn_resnet50deepstem', CH, 16, True, pretrained_backbone=False).cuda().eval()
    rs = np.random.RandomState(0)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).cuda(), torch.tensor([0.229, 0.224, 0.225]).cuda()
    image = ((torch.from_numpy(rs.randint(0, 256, size=(3, H, W)).astype(np.float32)).cuda() / 255 - mean[:, None, None]) /
             std[:, None, None])[None].contiguous()
    lab = rs.randint(0, C, size=(1, H, W)).astype(np.int64)
    lab[rs.uniform(size=lab.shape) < 0.1] = 255
    labels = torch.from_numpy(lab).cuda()
    with torch.no_grad():
        zq = net(image, lowres=True).contiguous()
        counts = torch.zeros(3 * C + 3, dtype=torch.int64, device='cuda')
        fused = lambda: ops.lowres_iou_counts(zq, labels, (H, W), C, 255, counts)                                   # noqa: E731
        chain = lambda: ops.logits_iou_counts(ops.upsample_bilinear(zq, (H, W)), labels, C, 255, counts)           # noqa: E731
        if args.kernels_only:
            for _ in range(args.reps):
                fused(), chain()
            torch.cuda.synchronize()
            return
        a = ops.lowres_iou_counts(zq, labels, (H, W), C, 255)
        b = ops.logits_iou_counts(ops.upsample_bilinear(zq, (H, W)), labels, C, 255)
        row = {'picture': '%dx%d' % (W, H), 'channels': CH, 'counters_equal': bool(torch.equal(a, b)),
               'forward_lowres_ms': timed(lambda: net(image, lowres=True), args.reps),
               'forward_full_ms': timed(lambda: net(image), args.reps),
               'k_lowres_iou_ms': timed(fused, args.reps),
               'upsample_plus_logits_iou_ms': timed(chain, args.reps)}
        m_lo, m_full = LowresLogitsIoU(C, 255), LogitsIoU(C, 255)
        row['loop_lowres_ms'], row['loop_lowres_peak_MB'] = host_timed(lambda: m_lo.step_lowres(net(image, lowres=True), labels),
                                                                       args.reps)
        row['loop_full_ms'], row['loop_full_peak_MB'] = host_timed(lambda: m_full.step(net(image), labels), args.reps)
        h, w = zq.shape[2:]
        floor_f = 4 * CH * h * w + 8 * H * W                              # quarter logits and int64 targets once
        floor_c = 4 * CH * h * w + 2 * 4 * CH * H * W + 8 * H * W         # + full logits written and read back
        row.update({'fused_byte_floor_MB': floor_f / 1e6, 'fused_floor_us_at_peak': 1e6 * floor_f / HBM_PEAK,
                    'chain_byte_floor_MB': floor_c / 1e6, 'chain_floor_us_at_peak': 1e6 * floor_c / HBM_PEAK})
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'rows': [row]}, f, indent=1)


if __name__ == '__main__':
    main()
