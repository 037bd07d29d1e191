"""Time the multi-scale + flip stage-2 generator of VOC per picture (trainer/eval_save_cosplbl_prop_includeonehot_voc_ms.py) on a
seeded, randomly initialised deeplabv3pluswn_resnet50deepstem and seeded 500 x 375 / 500 x 500 pictures.

Per picture (device events, median of --reps): the ten pictures of eval_spx_identity_ms, the ten quarter-resolution forwards, the
ensemble fused (ops.ms_ensemble) and as the ATen chain (MAS_MS_ENSEMBLE=aten: feat_forward's upsampling, flip, F.interpolate, adds,
divide, F.normalize on the same quarter maps), K9 (ops.stage2_pseudo_labels), the PNG write (host clock), and the whole generation
step (host clock, synchronised).  Also: the fused kernel's algorithmic byte floor from the shapes, and the largest difference between
the fused and the ATen ensemble.  --ensemble-only runs the two ensembles --reps times and nothing else (for a rocprofv3 kernel trace).

    python tools/ms_ensemble_probe.py --out profiles/ms_ensemble/ms_ensemble_probe.json
    rocprofv3 --kernel-trace --stats -d OUT -o mse -- python tools/ms_ensemble_probe.py --ensemble-only --reps 20
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PICTURES = ((375, 500), (500, 500))          # (H, W): VOC's landscape size and a square one
HBM_PEAK = 8.0e12                            # MI355X HBM3E, bytes/s


def byte_floor(sizes, Ch, C, H, W):
    """Bytes the fused kernel cannot avoid: every quarter-resolution map read once, the two outputs written once."""
    q = sum((Ch + C) * (((hs - 1) // 2) // 2 + 1) * (((ws - 1) // 2) // 2 + 1) for hs, ws in sizes)
    return 4 * (q + (Ch + C) * H * W)


def aten_chain(feats_q, logits_q, sizes, flips, size):
    """The trainer's ATen ensemble on given quarter maps: feat_forward's upsampling (models/deeplab.py:_upsample), flip back,
    F.interpolate to the original size, sum, / n, F.normalize."""
    import torch.nn.functional as F
    from mulactseg_amd.models.deeplab import _upsample
    feats = outs = None
    for f, z, s, fl in zip(feats_q, logits_q, sizes, flips):
        f, z = _upsample(f, s), _upsample(z, s)
        if fl:
            f, z = f.flip(-1), z.flip(-1)
        f = F.interpolate(f, size=size, mode='bilinear', align_corners=False)
        z = F.interpolate(z, size=size, mode='bilinear', align_corners=False)
        feats = f if feats is None else feats + f
        outs = z if outs is None else outs + z
    n = len(feats_q)
    return F.normalize(feats / n, dim=1), outs / n


def timed(fn, reps, warmup=2, spread=False):
    """Median (ms) of fn over reps, by device events; spread: (median, [min, max])."""
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
    return (float(np.median(ts)), [float(np.min(ts)), float(np.max(ts))]) if spread else float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--ensemble-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from PIL import Image
    from mulactseg_amd import ops, synth
    from mulactseg_amd.dataloader.device_transforms import DeviceMultiScaleFlip
    from mulactseg_amd.models import get_model
    torch.manual_seed(0)
    net = get_model('deeplabv3pluswn_resnet50deepstem', 21, 16, True, pretrained_backbone=False).cuda().eval()
    tta = DeviceMultiScaleFlip()
    rows = []
    tmp = tempfile.mkdtemp()
    for H, W in PICTURES:
        rs = np.random.RandomState(H * 1000 + W)
        pic = torch.from_numpy(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda()
        images = tta(pic)
        sizes = [tuple(im.shape[-2:]) for im in images]
        flips = [k >= 5 for k in range(10)]
        with torch.no_grad():
            q = [net.feat_forward_quarter(im[None]) for im in images]
            fq, lq = [f.contiguous() for f, _ in q], [z.contiguous() for _, z in q]
            fused = lambda: ops.ms_ensemble(fq, lq, sizes, flips, (H, W))          # noqa: E731
            aten = lambda: aten_chain(fq, lq, sizes, flips, (H, W))                # noqa: E731
            if args.ensemble_only:
                for _ in range(args.reps):
                    fused(), aten()
                torch.cuda.synchronize()
                continue
            f1, z1 = fused()
            f0, z0 = aten()
            df = float((f1 - f0).abs().max())
            dz = float(((z1 - z0).abs() / z0.abs().clamp(min=1.0)).max())
            S = 32
            spx = torch.from_numpy(synth.superpixel_map(H + W, H, W, S).astype(np.int64) % S).cuda()
            trs = np.random.RandomState(7)
            targets = torch.from_numpy((trs.uniform(size=(S, 22)) < 0.15).astype(np.uint8)).cuda()
            spmask = torch.from_numpy(trs.uniform(size=S) < 0.5).cuda()[spx]
            k9 = lambda: ops.stage2_pseudo_labels(f1, z1.contiguous(), targets[None], spmask[None], spx[None], True)   # noqa: E731
            fused_ms, fused_span = timed(fused, args.reps, spread=True)
            row = {'picture': '%dx%d' % (W, H), 'tta_ms': timed(lambda: tta(pic), args.reps),
                   'forwards_ms': timed(lambda: [net.feat_forward_quarter(im[None]) for im in images], args.reps),
                   'ensemble_fused_ms': fused_ms, 'ensemble_fused_ms_min_max': fused_span, 'ensemble_aten_ms': timed(aten, args.reps), 'k9_ms': timed(k9, args.reps)}
            plbl = k9()
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                Image.fromarray(plbl[0].cpu().numpy().astype('uint8')).save(os.path.join(tmp, 'p.png'))
                t.append(time.perf_counter() - t0)
            row['png_ms'] = 1e3 * float(np.median(t))
            t = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ims = tta(pic)
                qq = [net.feat_forward_quarter(im[None]) for im in ims]
                ff, zz = ops.ms_ensemble([f.contiguous() for f, _ in qq], [z.contiguous() for _, z in qq], sizes, flips, (H, W))
                p = ops.stage2_pseudo_labels(ff, zz.contiguous(), targets[None], spmask[None], spx[None], True)
                Image.fromarray(p[0].cpu().numpy().astype('uint8')).save(os.path.join(tmp, 'p.png'))
                t.append(time.perf_counter() - t0)
            row['generation_step_ms'] = 1e3 * float(np.median(t))
            floor = byte_floor(sizes, fq[0].shape[1], lq[0].shape[1], H, W)
            row.update({'fused_byte_floor_MB': floor / 1e6, 'fused_floor_us_at_peak': 1e6 * floor / HBM_PEAK,
                        'fused_floor_bytes_per_s_TB': floor / (row['ensemble_fused_ms'] * 1e-3) / 1e12,
                        'fused_share_of_hbm_peak': floor / (row['ensemble_fused_ms'] * 1e-3) / HBM_PEAK,
                        'aten_over_fused': row['ensemble_aten_ms'] / row['ensemble_fused_ms'],
                        'fused_vs_aten_feat_max_abs': df, 'fused_vs_aten_logit_max_rel': dz})
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
