"""Time the photometric path of the training augmentation (csrc/photometric.hip) on one sample at the production shape: a seeded
1024 x 2048 picture with a superpixel map -> a 768 x 768 crop, fixed geometry (scale 1.37, no pad), the whole chain
(brightness, contrast, saturation, hue) and grayscale.

Default: device-event medians of --reps whole calls after 2 warm-ups of ``DeviceTrainAugment`` (the plain sample: one launch) and of
``DeviceTrainAugmentStrong`` with the chain (two launches plus the zeroing of the accumulator), each including the host's table
upload; the jittered picture is checked against the host entry first.  The bytes each kernel must move, from the shapes, and the
expected augmentation cost of a ``[4,3,768,768]`` step at the reference's probabilities (a sample is jittered or grey with
probability 1 - 0.8 * 0.8 = 0.36) are printed beside them; ``--bench-json FILE`` (the result line of ``bench.py`` run on the same
machine) adds the measured train step and the share of it.  One JSON line, --out writes it.

--kernels-only runs --reps plain calls, then --reps jittered calls, then --reps calls of pass 1 alone per entry of PASS1_VARIANTS,
and nothing else; --summarize CSV turns the kernel trace of such a run into per-kernel medians:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o pm -- python tools/photometric_probe.py --kernels-only --reps 20
    python tools/photometric_probe.py --summarize OUT/pm_kernel_trace.csv --reps 20
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, CROP, NSEG = 1024, 2048, 768, 2048
P_JITTER, P_GRAY, BATCH = 0.2, 0.2, 4
CHAIN = dict(order=[3, 0, 1, 2], factors=[1.31, 0.72, 1.18, -0.06], grey=True)
# pass 1 without the sum (the u8 store alone), with the sum of the untouched crop (contrast first), with saturation before contrast
PASS1_VARIANTS = {'grey_only': dict(order=None, factors=[None] * 4, grey=True),
                  'contrast_first': dict(order=[1, 3, 0, 2], factors=[1.31, 0.72, 1.18, -0.06], grey=True),
                  'saturation_then_contrast': dict(order=[2, 1, 3, 0], factors=[1.31, 0.72, 1.18, -0.06], grey=True)}


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


def params():
    th, tw = int(H * 1.37), int(W * 1.37)
    return dict(scale=1.37, th=th, tw=tw, gap_y=0, gap_x=0, i=211, j=1033, flip=True)


def bytes_moved():
    """What each kernel must move per sample, from the shapes (the source picture and the tables are read through L2)."""
    n = CROP * CROP
    src = 3 * n / 1.37 ** 2          # the source pixels under the crop, each read by several taps out of L2
    maps = n * (2 + 8)               # int16 ids in, int64 out
    return {'k_train_augment': {'source_read_L2_resident': src, 'f32_written': 12 * n, 'map_read_written': maps},
            'k_train_augment_u8': {'source_read_L2_resident': src, 'u8_written': 3 * n, 'map_read_written': maps},
            'k_photometric': {'u8_read': 3 * n, 'f32_written': 12 * n}}


def p_active():
    return 1.0 - (1.0 - P_JITTER) * (1.0 - P_GRAY)


def summarize(path, reps):
    """Per-kernel medians (us) of a --kernels-only trace."""
    rows = list(csv.DictReader(open(path)))
    dur = lambda key: [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows       # noqa: E731
                       if key(r['Kernel_Name'])]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    pass1 = dur(lambda n: 'k_train_augment_u8' in n)
    groups = {'k_train_augment': dur(lambda n: 'k_train_augment' in n and 'k_train_augment_u8' not in n),
              'k_train_augment_u8': pass1[:reps], 'k_photometric': dur(lambda n: 'k_photometric' in n)}
    for k, name in enumerate(PASS1_VARIANTS):          # dispatched after the jittered calls, in this order
        groups['k_train_augment_u8_' + name] = pass1[(k + 1) * reps:(k + 2) * reps]
    for name, d in groups.items():
        if len(d) != reps:
            raise SystemExit("expected %d %s dispatches, found %d" % (reps, name, len(d)))
    out = {name + '_us': float(np.median(d)) for name, d in groups.items()}
    out['dispatches_per_kernel'] = reps
    out['jittered_over_plain'] = (out['k_train_augment_u8_us'] + out['k_photometric_us']) / out['k_train_augment_us']
    plain, jit = out['k_train_augment_us'], out['k_train_augment_u8_us'] + out['k_photometric_us']
    out['expected_kernel_us_per_step_of_%d' % BATCH] = BATCH * ((1 - p_active()) * plain + p_active() * jit)
    out['plain_kernel_us_per_step_of_%d' % BATCH] = BATCH * plain
    n = CROP * CROP
    out['k_photometric_GBps'] = 15 * n / (out['k_photometric_us'] * 1e-6) / 1e9
    print(json.dumps(out))


def train_step_ms(path):
    """``ms_per_iter`` of the train-iter leg in a ``bench.py`` result line."""
    def walk(o):
        if isinstance(o, dict):
            if str(o.get('metric', '')).startswith('train-iter') and 'ms_per_iter' in o:
                return o['ms_per_iter']
            o = list(o.values())
        if isinstance(o, list):
            for v in o:
                r = walk(v)
                if r is not None:
                    return r
        return None
    for line in open(path):
        line = line.strip()
        if line.startswith('{'):
            r = walk(json.loads(line))
            if r is not None:
                return float(r)
    raise SystemExit("no train-iter leg in %s" % path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--summarize', default=None)
    ap.add_argument('--bench-json', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.summarize is not None:
        return summarize(args.summarize, args.reps)
    import torch
    from mulactseg_amd.dataloader import device_transforms as dt
    rs = np.random.RandomState(0)
    img = torch.from_numpy(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda()
    spx = torch.from_numpy(rs.randint(0, NSEG, size=(H, W)).astype(np.int16)).cuda()
    plain_t = dt.DeviceTrainAugment(size=(CROP, CROP), pad_values=[NSEG])
    strong_t = dt.DeviceTrainAugmentStrong(size=(CROP, CROP), pad_values=[NSEG])
    p = params()
    ps = dict(p, photometric=CHAIN)
    plain = lambda: plain_t(img, [spx], params=p)           # noqa: E731
    strong = lambda: strong_t(img, [spx], params=ps)        # noqa: E731
    if args.kernels_only:
        for _ in range(args.reps):
            plain()
        for _ in range(args.reps):
            strong()
        for ph in PASS1_VARIANTS.values():          # pass 1 alone: what its extra work costs beside the geometry
            for _ in range(args.reps):
                strong_t.augment_u8(img, [spx], dict(p, photometric=ph))
        torch.cuda.synchronize()
        return
    crop, _, lsum = strong_t.augment_u8(img, [spx], ps)
    _, want, want_sum = dt.photometric_reference(crop.cpu().numpy(), CHAIN)
    assert int(lsum.item()) == want_sum and np.array_equal(strong()[0].cpu().numpy(), want)
    row = {'sample': '%dx%d -> %dx%d, scale 1.37, flip' % (H, W, CROP, CROP), 'chain': CHAIN, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0), 'bytes': bytes_moved(), 'p_jittered_or_grey': p_active()}
    row['plain_call_ms'] = timed(plain, args.reps)
    row['jittered_call_ms'] = timed(strong, args.reps)
    row['pass1_call_ms'] = timed(lambda: strong_t.augment_u8(img, [spx], ps), args.reps)
    row['pass2_call_ms'] = timed(lambda: dt.photometric(crop, CHAIN, lsum), args.reps)
    row['expected_call_ms_per_step_of_%d' % BATCH] = BATCH * ((1 - p_active()) * row['plain_call_ms'] + p_active() * row['jittered_call_ms'])
    row['plain_call_ms_per_step_of_%d' % BATCH] = BATCH * row['plain_call_ms']
    if args.bench_json:
        step = train_step_ms(args.bench_json)
        row['train_step_ms'] = step
        row['added_share_of_train_step'] = (row['expected_call_ms_per_step_of_%d' % BATCH] - row['plain_call_ms_per_step_of_%d' % BATCH]) / step
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(row, f, indent=1)


if __name__ == '__main__':
    main()
