"""Time the two stage-2 ablation generators of paper Fig. 7 per 1024 x 2048 picture on a seeded, randomly initialised
deeplabv3pluswn_resnet50deepstem (20 output channels) and a seeded picture, id map (2048 superpixels) and dominant target map.

Per picture (device events, median of --reps): the network forward, ``k_naive_plbl`` (ops.naive_pseudo_labels, mask and threshold
modes) against the ATen chain it replaces (F.interpolate, softmax / max, masked_fill), ``k_spx_max_onehot`` (ops.spx_max_onehot; int64
target and ids as the loader yields them, and uint8 / int16) against an ATen chain (scatter_reduce amax, one_hot, the != 255 mask),
and the whole generation step of each method (host clock, synchronised: forward, labels, copy to the host, PNG encode).  Also the
byte floors of both kernels at the HBM peak.  --kernels-only runs the kernels and the ATen chains --reps times and nothing else (for
a rocprofv3 kernel trace).

    python tools/naive_plbl_probe.py --out profiles/naive_plbl/naive_plbl_probe.json
    rocprofv3 --kernel-trace --stats -d OUT -o npl -- python tools/naive_plbl_probe.py --kernels-only --reps 20
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

H, W, C, NSEG = 1024, 2048, 20, 2048
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


def host_timed(fn, reps):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def aten_onehot(target, spx, nseg, C):
    import torch
    m = torch.full((nseg,), -1, dtype=torch.int64, device=target.device)
    m.scatter_reduce_(0, spx.reshape(-1), target.reshape(-1).long(), 'amax', include_self=True)
    m = torch.where(m < 0, torch.zeros_like(m), torch.where(m == 255, torch.full_like(m, C - 1), m))
    return torch.nn.functional.one_hot(m, C).to(torch.uint8), target != 255


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from PIL import Image
    from mulactseg_amd import ops, synth
    from mulactseg_amd.models import get_model
    torch.manual_seed(0)
    net = get_model('deeplabv3pluswn_resnet50deepstem', C, 16, True, pretrained_backbone=False).cuda().eval()
    rs = np.random.RandomState(0)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).cuda(), torch.tensor([0.229, 0.224, 0.225]).cuda()
    image = ((torch.from_numpy(rs.randint(0, 256, size=(3, H, W)).astype(np.float32)).cuda() / 255 - mean[:, None, None]) /
             std[:, None, None])[None].contiguous()
    spx = torch.from_numpy(synth.superpixel_map(11, H, W, NSEG).astype(np.int64)).cuda()
    dom = torch.from_numpy(rs.randint(0, C, size=NSEG)).cuda()
    target = torch.where(torch.from_numpy(rs.uniform(size=NSEG) < 0.2).cuda()[spx], dom[spx], torch.full_like(spx, 255))
    spmask = target != 255
    with torch.no_grad():
        zq = net(image, lowres=True).contiguous()
        fused = lambda: ops.naive_pseudo_labels(zq, (H, W), spmask[None], 0.0)              # noqa: E731
        fused_th = lambda: ops.naive_pseudo_labels(zq, (H, W), None, 0.5)                   # noqa: E731
        aten = lambda: ops._naive_plbl_aten(zq, (H, W), spmask[None], 0.0)                  # noqa: E731
        aten_th = lambda: ops._naive_plbl_aten(zq, (H, W), spmask[None], 0.5)               # noqa: E731
        onehot = lambda: ops.spx_max_onehot(target, spx, NSEG, C)                           # noqa: E731
        t8, s16 = target.to(torch.uint8), spx.to(torch.int16)
        onehot_u8 = lambda: ops.spx_max_onehot(t8, s16, NSEG, C)                            # noqa: E731
        onehot_aten = lambda: aten_onehot(target, spx, NSEG, C)                             # noqa: E731
        if args.kernels_only:
            for _ in range(args.reps):
                fused(), fused_th(), aten(), aten_th(), onehot(), onehot_u8(), onehot_aten()
            torch.cuda.synchronize()
            return
        same = bool(torch.equal(fused(), aten()))
        diff_th = int((fused_th() != aten_th()).sum())
        r1, m1 = onehot()
        r0, m0 = onehot_aten()
        assert torch.equal(r1, r0) and torch.equal(m1, m0)
        row = {'picture': '%dx%d' % (W, H), 'C': C, 'nseg': NSEG,
               'forward_lowres_ms': timed(lambda: net(image, lowres=True), args.reps),
               'naive_fused_ms': timed(fused, args.reps), 'naive_fused_th_ms': timed(fused_th, args.reps),
               'naive_aten_ms': timed(aten, args.reps), 'naive_aten_th_ms': timed(aten_th, args.reps),
               'onehot_fused_i64_ms': timed(onehot, args.reps), 'onehot_fused_u8_i16_ms': timed(onehot_u8, args.reps),
               'onehot_aten_ms': timed(onehot_aten, args.reps),
               'naive_equal_to_aten_mask_mode': same, 'naive_th_pixels_differing_from_aten': diff_th}
        tmp = tempfile.mkdtemp()

        def step_naive():
            z = net(image, lowres=True)
            p = ops.naive_pseudo_labels(z.contiguous(), (H, W), spmask[None], 0.0)
            Image.fromarray(p[0].cpu().numpy().astype('uint8')).save(os.path.join(tmp, 'a.png'))

        def step_dom():
            rows, mask = ops.spx_max_onehot(target, spx, NSEG, C)
            f, z = net.feat_forward_lowres(image)
            p = ops.stage2_pseudo_labels(f.contiguous(), z.contiguous(), rows[None], mask[None], spx[None], True)
            Image.fromarray(p[0].cpu().numpy().astype('uint8')).save(os.path.join(tmp, 'b.png'))
        row['step_naive_ms'] = host_timed(step_naive, args.reps)
        row['step_onehotignore_ms'] = host_timed(step_dom, args.reps)
        h, w = zq.shape[2:]
        floor_n = 4 * C * h * w + 2 * H * W                       # quarter logits once, mask and labels once
        floor_o = (8 + 8 + 1) * H * W + NSEG * C                  # int64 target and ids, mask out, rows out
        row.update({'naive_byte_floor_MB': floor_n / 1e6, 'naive_floor_us_at_peak': 1e6 * floor_n / HBM_PEAK,
                    'onehot_byte_floor_MB_i64': floor_o / 1e6, 'onehot_floor_us_at_peak': 1e6 * floor_o / HBM_PEAK})
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'rows': [row]}, f, indent=1)


if __name__ == '__main__':
    main()
