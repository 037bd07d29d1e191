"""Time the naive arg-max pseudo labels of VOC per picture (trainer/eval_save_cosplbl_naive_voc_ms.py, the README's Naive Inference with
the multi-scale + flip TTA) on a seeded, randomly initialised 21-class deeplabv3pluswn_resnet50deepstem and seeded 500 x 375 / 500 x 500
pictures.

Per picture (device events, median of --reps): the ten quarter-resolution forwards (net(x, lowres=True)); labels + counters fused
(ops.ms_naive_labels, csrc/ms_naive.hip), as the ATen chain (MAS_MS_NAIVE=aten: upsample_bilinear, flip, F.interpolate, adds, / n,
max, then MeanIoU._after_step's kernel) and as ops.ms_ensemble (a one-channel dummy feature map) + torch.max + MeanIoU._after_step, all
on the same quarter maps; the PNG write (host clock); the whole generation loop of the generator (host clock, synchronised) with
MAS_STAGE2_WORKERS=1 and =4.  Also the fused kernel's byte floor from the shapes, and how many labels the fused and ATen paths give
differently (all of them at a top-2 gap <= 1e-5).  --kernels-only runs the three label paths --reps times and nothing else (for a
rocprofv3 kernel trace).

    python tools/ms_naive_probe.py --out profiles/ms_naive/ms_naive_probe.json
    rocprofv3 --kernel-trace --stats -d OUT -o msn -- python tools/ms_naive_probe.py --kernels-only --reps 20
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PICTURES = ((375, 500), (500, 500))          # (H, W): VOC's landscape size and a square one
HBM_PEAK = 8.0e12                            # MI355X HBM3E, bytes/s
K = 22                                       # MeanIoU(num_classes + 1): the 21 VOC classes and the void class 21


def byte_floor(sizes, C, H, W):
    """Bytes the fused kernel cannot avoid: every quarter-resolution logit read once, the int64 targets read once, the u8 labels
    written once."""
    q = sum(C * (((hs - 1) // 2) // 2 + 1) * (((ws - 1) // 2) // 2 + 1) for hs, ws in sizes)
    return 4 * q + 8 * H * W + H * W


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


class _Loader:
    def __init__(self, samples):
        self.samples, self.k = samples, 0

    def __len__(self):
        return len(self.samples)

    def __next__(self):
        self.k += 1
        return self.samples[self.k - 1]


def loop_ms(net, samples, workers, reps):
    """Per-picture time of the generator's loop (eval_save_cosplbl_prop.inference) over ``samples``, median over reps."""
    import torch
    from mulactseg_amd.trainer import eval_save_cosplbl_naive_voc_ms as G
    tmp = tempfile.mkdtemp(prefix="ms_naive_probe_")
    tr = object.__new__(G.ActiveTrainer)
    tr.args = types.SimpleNamespace(ignore_idx=255, init_checkpoint=os.path.join(tmp, "checkpoint01.tar"), plbl_type=None,
                                    val_batch_size=1, save_vis=False)
    tr.net, tr.device, tr.num_classes, tr.selection_iter, tr.save_dir = net, torch.device('cuda:0'), 21, 1, None
    os.environ["MAS_STAGE2_WORKERS"] = str(workers)
    ts = []
    try:
        import contextlib
        import io
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                tr.inference(_Loader(samples))
            ts.append((time.perf_counter() - t0) / len(samples))
    finally:
        os.environ.pop("MAS_STAGE2_WORKERS", None)
    return 1e3 * float(np.median(ts[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from PIL import Image
    from mulactseg_amd import ops
    from mulactseg_amd.dataloader.device_transforms import DeviceMultiScaleFlip
    from mulactseg_amd.models import get_model
    from mulactseg_amd.utils.miou import MeanIoU
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
        targets = torch.from_numpy(np.where(rs.uniform(size=(1, H, W)) < 0.1, 21, rs.randint(0, 21, size=(1, H, W)))).cuda()
        counts = torch.zeros(3 * K + 3, dtype=torch.int64, device='cuda')
        with torch.no_grad():
            zs = [net(im[None], lowres=True).contiguous() for im in images]
            dummy = [torch.ones((1, 1) + tuple(z.shape[2:]), device='cuda') for z in zs]

            def fused():
                return ops.ms_naive_labels(zs, sizes, flips, (H, W), targets=targets, counts=counts, num_classes=K)

            def aten():
                os.environ["MAS_MS_NAIVE"] = "aten"
                try:
                    return ops.ms_naive_labels(zs, sizes, flips, (H, W), targets=targets, counts=counts, num_classes=K)
                finally:
                    os.environ.pop("MAS_MS_NAIVE", None)

            def ensemble():
                lab = torch.max(ops.ms_ensemble(dummy, zs, sizes, flips, (H, W))[1], 1)[1]
                m = MeanIoU(K, 255)
                m._counts = counts
                m._after_step({'outputs': lab, 'targets': targets})
                return lab
            if args.kernels_only:
                for _ in range(args.reps):
                    fused(), aten(), ensemble()
                torch.cuda.synchronize()
                continue
            l1, l0, le = fused(), aten(), ensemble()
            m = ops.ms_ensemble(dummy, zs, sizes, flips, (H, W))[1]
            top = torch.topk(m, 2, dim=1)[0]
            gap = top[:, 0] - top[:, 1]
            differ = l1 != l0
            fused_ms, fused_span = timed(fused, args.reps, spread=True)
            row = {'picture': '%dx%d' % (W, H),
                   'forwards_ms': timed(lambda: [net(im[None], lowres=True) for im in images], args.reps),
                   'fused_ms': fused_ms, 'fused_ms_min_max': fused_span, 'aten_ms': timed(aten, args.reps), 'ensemble_argmax_count_ms': timed(ensemble, args.reps),
                   'fused_equals_ensemble_argmax': bool(torch.equal(l1, le)),
                   'fused_vs_aten_labels_differ': int(differ.sum()), 'fused_vs_aten_max_gap_where_differ': float(gap[differ].max()) if bool(differ.any()) else 0.0}
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                Image.fromarray(l1[0].cpu().numpy().astype('uint8')).save(os.path.join(tmp, 'p.png'))
                t.append(time.perf_counter() - t0)
            row['png_ms'] = 1e3 * float(np.median(t))
            floor = byte_floor(sizes, zs[0].shape[1], H, W)
            row.update({'fused_byte_floor_MB': floor / 1e6, 'fused_floor_us_at_peak': 1e6 * floor / HBM_PEAK,
                        'fused_share_of_hbm_peak': floor / (row['fused_ms'] * 1e-3) / HBM_PEAK,
                        'aten_over_fused': row['aten_ms'] / row['fused_ms'],
                        'ensemble_over_fused': row['ensemble_argmax_count_ms'] / row['fused_ms']})
            samples = []
            for k in range(8):
                samples.append({'image_list': [images], 'labels': targets, 'imsizes': [(W, H)],
                                'fnames': [('p%d.jpg' % k, 'p%d.png' % k, 's%d.pkl' % k)], 'spx': targets})
            for workers in (1, 4):
                row['step_ms_workers_%d' % workers] = loop_ms(net, samples, workers, max(2, args.reps // 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
