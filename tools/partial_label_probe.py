"""Time the stage-1 loss scans per multi-hot term (csrc/losses.hip; ``choice`` = the merged positive, ``rc``, ``topone``:
csrc/partial_label.h) at the training geometry: seeded quarter-resolution logits [4,20,192,192] scanned at 768 x 768 against 2048
superpixels, production flags (ce + mc + group over multi-hot regions), T = 0.1.

Default: one JSON line with, per mode, ``--series`` medians (device events, ``--reps`` calls each after 2 warm-ups) of the forward call
(``ops.partial_loss_fwd_lowres``) and of the backward call (``ops.partial_loss_bwd_lowres``), the modes interleaved inside every
series; the peak allocation of one ``FusedPartialLabelLoss(group=False)`` step against the ATen composition on materialised logits.

--lib PATH [PATH ...] times ``choice`` only, through the C ABI of each named library (``product`` = the in-tree one), the libraries
interleaved inside every series: the same-box comparison of two builds.  A library built before this probe's entry points were added
is fine: only the entry points both builds have are bound.

--kernels-only runs one forward call per mode (the state of the backward calls), then ``--reps`` forward + backward calls per mode in
the order choice, rc, topone, and nothing else; --summarize CSV
turns the kernel trace of such a run into per-mode medians of k_partial_loss_fwd / k_partial_loss_bwd:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o pl -- python tools/partial_label_probe.py --kernels-only --reps 20
    python tools/partial_label_probe.py --summarize OUT/pl_kernel_trace.csv --reps 20
"""
import argparse
import csv
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, HQ, WQ, H, W, NSEG = 4, 20, 192, 192, 768, 768, 2048
CE_TEMP = 0.1
BASE = 1 | 2 | 4 | 8
MODES = {'choice': 0, 'rc': 32, 'topone': 64}


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


def summarize(path, reps):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = lambda sel: [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if sel in r['Kernel_Name']]   # noqa: E731
    fwd, bwd = dur('k_partial_loss_fwd'), dur('k_partial_loss_bwd')
    fwd = fwd[len(MODES):]           # (one forward call per mode comes first: the state the backward calls read)
    if len(fwd) != reps * len(MODES) or len(bwd) != reps * len(MODES):
        raise SystemExit("expected %d dispatches per direction, found %d / %d" % (reps * len(MODES), len(fwd), len(bwd)))
    out = {'dispatches_per_group': reps}
    for k, m in enumerate(MODES):
        out['k_partial_loss_fwd_%s_us' % m] = float(np.median(fwd[k * reps:(k + 1) * reps]))
        out['k_partial_loss_bwd_%s_us' % m] = float(np.median(bwd[k * reps:(k + 1) * reps]))
    print(json.dumps(out))


def inputs():
    import torch
    from mulactseg_amd import synth
    zq = torch.from_numpy(synth.logits(5, N, C, HQ, WQ)).cuda()
    spx, msk = zip(*[synth.train_crop(70 + i, H, W, NSEG) for i in range(N)])
    tgt = np.stack([synth.multi_hot_targets(90 + i, NSEG, C) for i in range(N)])
    return zq, torch.from_numpy(np.stack(spx)).cuda(), torch.from_numpy(np.stack(msk)).cuda(), torch.from_numpy(tgt).cuda()


def raw_calls(path, zq, spx, msk, bits, invT):
    """(forward, backward) closures on the C ABI of the library at ``path``: the scans plus the launches around them that
    ops.partial_loss_fwd_lowres / _bwd_lowres make (memset, group finalize, loss values; loss scales, memset, fixed point -> float)."""
    import torch
    from mulactseg_amd import _lib
    lib = ctypes.CDLL(path)
    for name in ('mas_partial_loss_fwd_lowres', 'mas_group_finalize', 'mas_loss_values', 'mas_loss_scales', 'mas_partial_loss_bwd_lowres',
                 'mas_fix_to_float'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    buf = torch.zeros(_lib.ACC_WORDS + N * NSEG * C, dtype=torch.int64, device='cuda')
    acc, gmax = buf[:_lib.ACC_WORDS], buf[_lib.ACC_WORDS:]
    losses, scale = torch.empty(3, device='cuda'), torch.empty(3, device='cuda')
    go = torch.tensor([16.0, 8.0, 1.0], device='cuda')
    fix, dz = torch.zeros((N, C, HQ, WQ), dtype=torch.int64, device='cuda'), torch.empty_like(zq)
    st = torch.cuda.current_stream().cuda_stream
    m8 = msk.view(torch.uint8)

    def ok(code):
        if code != 0:
            raise SystemExit("%s: call failed with code %d" % (path, code))

    def fwd():
        buf.zero_()
        ok(lib.mas_partial_loss_fwd_lowres(zq.data_ptr(), HQ, WQ, spx.data_ptr(), _lib.ID_I64, m8.data_ptr(), bits.data_ptr(), N, C, H, W, NSEG,
                                           invT, BASE, gmax.data_ptr(), acc.data_ptr(), st))
        ok(lib.mas_group_finalize(gmax.data_ptr(), gmax.numel(), acc.data_ptr(), st))
        ok(lib.mas_loss_values(acc.data_ptr(), BASE, losses.data_ptr(), st))

    def bwd():
        ok(lib.mas_loss_scales(acc.data_ptr(), go.data_ptr(), BASE, scale.data_ptr(), st))
        fix.zero_()
        ok(lib.mas_partial_loss_bwd_lowres(zq.data_ptr(), HQ, WQ, spx.data_ptr(), _lib.ID_I64, m8.data_ptr(), bits.data_ptr(), gmax.data_ptr(),
                                           scale.data_ptr(), N, C, H, W, NSEG, invT, BASE, fix.data_ptr(), st))
        ok(lib.mas_fix_to_float(fix.data_ptr(), fix.numel(), _lib.GRAD_FRAC, dz.data_ptr(), st))
    return fwd, bwd, (losses, dz)


def peak_of(step):
    import torch
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--series', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--summarize', default=None)
    ap.add_argument('--lib', nargs='+', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.summarize is not None:
        return summarize(args.summarize, args.reps)
    import torch
    from mulactseg_amd import _lib, ops
    zq, spx, msk, tgt = inputs()
    invT = ops.inv_temperature(CE_TEMP)
    bits = ops.target_bits(tgt)
    go = torch.tensor([16.0, 8.0, 1.0], device='cuda')
    row = {'batch': '[%d,%d,%d,%d] -> %dx%d' % (N, C, HQ, WQ, H, W), 'nseg': NSEG, 'ce_temp': CE_TEMP, 'reps': args.reps,
           'series': args.series, 'device': torch.cuda.get_device_name(0), 'selected_pixels': int(msk.sum())}

    if args.lib:
        calls, outs = {}, {}
        for name in args.lib:
            path = _lib.LIB_PATH if name == 'product' else os.path.abspath(name)
            f, b, o = raw_calls(path, zq, spx, msk, bits, invT)
            f(), b()
            torch.cuda.synchronize()
            calls[name], outs[name] = (f, b), (o[0].clone(), o[1].clone())
        first = outs[args.lib[0]]
        row['same_bits'] = all(torch.equal(first[0].view(torch.int32), o[0].view(torch.int32)) and
                               torch.equal(first[1].view(torch.int32), o[1].view(torch.int32)) for o in outs.values())
        row['choice_fwd_call_ms'] = {n: [] for n in args.lib}
        row['choice_bwd_call_ms'] = {n: [] for n in args.lib}
        for _ in range(args.series):
            for n in args.lib:
                row['choice_fwd_call_ms'][n].append(timed(calls[n][0], args.reps))
                row['choice_bwd_call_ms'][n].append(timed(calls[n][1], args.reps))
    else:
        state = {}
        for m, f in MODES.items():
            _, acc, gmax = ops.partial_loss_fwd_lowres(zq, (H, W), spx, msk, bits, invT, BASE | f)
            state[m] = (acc, gmax)
        fwd = {m: (lambda f=f: ops.partial_loss_fwd_lowres(zq, (H, W), spx, msk, bits, invT, BASE | f)) for m, f in MODES.items()}
        bwd = {m: (lambda m=m, f=f: ops.partial_loss_bwd_lowres(zq, (H, W), spx, msk, bits, state[m][1], state[m][0], go, invT, BASE | f))
               for m, f in MODES.items()}
        if args.kernels_only:
            for m in MODES:
                for _ in range(args.reps):
                    fwd[m]()
                    bwd[m]()
            torch.cuda.synchronize()
            return
        row['multi_hot_pixels'] = int(state['choice'][0][3])
        row['fwd_call_ms'] = {m: [] for m in MODES}
        row['bwd_call_ms'] = {m: [] for m in MODES}
        for _ in range(args.series):
            for m in MODES:
                row['fwd_call_ms'][m].append(timed(fwd[m], args.reps))
                row['bwd_call_ms'][m].append(timed(bwd[m], args.reps))
        # peak allocation of one group=False step (quarter-resolution logits in, their gradient out) against the ATen composition of the
        # same objective on materialised logits
        from mulactseg_amd.utils.loss import FusedPartialLabelLoss
        crit = FusedPartialLabelLoss(NSEG, CE_TEMP, CE_TEMP, sync_normalisers=False, multi_hot='rc', group=False)

        def fused_step():
            z = zq.detach().requires_grad_(True)
            crit.weighted_lowres(z, (H, W), tgt, spx, msk, 16.0, 8.0, 0.0)[0].backward()

        def aten_step():
            z = zq.detach().requires_grad_(True)
            up = torch.nn.functional.interpolate(z, size=(H, W), mode='bilinear', align_corners=False)
            p = torch.softmax(up.permute(0, 2, 3, 1).reshape(N, H * W, C) / CE_TEMP, dim=2)
            ce_sum, mc_sum, n_ce, n_mc = 0, 0, 1, 1
            for i in range(N):
                mk = msk[i].reshape(-1)
                q = p[i][mk] * tgt[i][spx[i].reshape(-1)[mk]].to(p.dtype)
                nb = (q > 0).sum(dim=1)
                s = q.sum(dim=1)
                one, multi = nb == 1, nb > 1
                ce_sum = ce_sum + (-torch.log(s[one] + 1e-8)).sum()
                w = (q[multi] / s[multi][:, None]).detach()
                mc_sum = mc_sum + (w * -torch.log(q[multi] + 1e-8)).sum()
                n_ce, n_mc = n_ce + int(one.sum()), n_mc + int(multi.sum())
            (16.0 * ce_sum / n_ce + 8.0 * mc_sum / n_mc).backward()
        row['peak_bytes_fused_group_false_step'] = peak_of(fused_step)
        row['peak_bytes_aten_step'] = peak_of(aten_step)
        row['bytes_of_one_full_resolution_logit_tensor'] = N * C * H * W * 4
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(row, f, indent=1)


if __name__ == '__main__':
    main()
