"""Time the data-generation step (csrc/labels.hip, mulactseg_amd/label_assignment.py) on a synthetic Cityscapes-sized pool.

Three numbers: kernel time per picture (HIP events around the counts + finalize [+ paint] launches of one resident picture), the
command line over an on-disk pool (labelIds PNGs + {'labels': int16} pickles, 1024 x 2048, nseg 2048; --distinct different maps
written under --pictures names), and, for context, the restated per-id loop (tests/label_assign_restated.py, the reference's steps
in numpy -- a restatement, not the reference tool) on one picture on the host.

    python tools/label_assign_probe.py --pictures 256 --out profiles/label_assign/label_assign_probe.json
"""
import argparse
import json
import os
import pickle
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def build_pool(root, n, distinct, H, W, nseg):
    from PIL import Image
    import label_assign_restated as R
    from mulactseg_amd.dataloader import constant
    raw_of_train = np.zeros(256, dtype=np.uint8)
    for raw in range(constant.N_RAW_IDS):
        t = int(constant.id_to_train_id[raw])
        if t != 255:
            raw_of_train[t] = raw
    maps = []
    for j in range(distinct):
        spx = R.voronoi(1000 + j, H, W, nseg)
        maps.append((spx, R.labels_for(2000 + j, spx, 19)))
    lines, region = [], {}
    os.makedirs(os.path.join(root, 'gtFine'), exist_ok=True)
    os.makedirs(os.path.join(root, 'spx'), exist_ok=True)
    for i in range(n):
        spx, lab = maps[i % distinct]
        stem = 'synth_%06d_000019' % i
        lbl, sp = 'gtFine/%s_gtFine_labelIds.png' % stem, 'spx/%s.pkl' % stem
        Image.fromarray(raw_of_train[lab]).save(os.path.join(root, lbl))
        with open(os.path.join(root, sp), 'wb') as f:
            pickle.dump({'labels': spx.astype(np.int16)}, f)
        lines.append('leftImg8bit/%s_leftImg8bit.png\t%s\t%s' % (stem, lbl, sp))
        region[sp] = [nseg, []]
    with open(os.path.join(root, 'list.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    with open(os.path.join(root, 'list.dict'), 'w') as f:
        json.dump(region, f)
    return maps


def kernel_times(maps, nseg, reps):
    import torch
    from mulactseg_amd import ops
    spx, lab = maps[0]
    s = torch.from_numpy(spx.astype(np.int16)).cuda()
    lb = torch.from_numpy(lab).cuda()
    ids = list(range(nseg))
    listed = ops.listed_ids(ids, nseg, 'cuda')
    out = {}
    for name, fn in (('counts_k0', lambda: ops._label_counts(lb, s, nseg, 19, 0)),
                     ('counts_k5', lambda: ops._label_counts(lb, s, nseg, 19, 5)),
                     ('multi_hot_k5', lambda: ops.region_multi_hot(lb, s, listed, nseg, 19, 5)),
                     ('dominant', lambda: ops.region_dominant(lb, s, listed, nseg, 19, True))):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name + '_us'] = round(e0.elapsed_time(e1) * 1000.0 / reps, 2)
    out['note'] = ('counts_k*: the counts kernel alone (+ its memsets); multi_hot_k5 and dominant include the label-check read-back '
                   '(one synchronisation) of the ops wrapper, so they are upper bounds on kernel time')
    return out


def cli_times(root, nseg, threads):
    from mulactseg_amd import label_assignment as la
    common = ['--nseg', str(nseg), '--trg_data_dir', root, '--trg_datalist', os.path.join(root, 'list.txt'),
              '--region_dict', os.path.join(root, 'list.dict'), '--num_worker', str(threads)]
    out = {}
    a = la.resolve(la.get_parser().parse_args(['multi_hot'] + common + ['--trim_multihot_boundary', '--trim_kernel_size', '5',
                                                                           '--save_data_dir', os.path.join(root, 'mh')]))
    out['multi_hot_k5'] = la.run(a)
    a = la.resolve(la.get_parser().parse_args(['dominant'] + common + ['--generate_ignore', '--loader',
                                                                          'region_cityscapes_dominant_all_sample', '--nvis_color', '0']))
    out['dominant_ignore_sample'] = la.run(a)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pictures', type=int, default=256)
    p.add_argument('--distinct', type=int, default=8)
    p.add_argument('--nseg', type=int, default=2048)
    p.add_argument('--reps', type=int, default=50)
    p.add_argument('--threads', type=int, default=8)
    p.add_argument('--no-cli', action='store_true')
    p.add_argument('--no-host-loop', action='store_true')
    p.add_argument('--out', default=None)
    a = p.parse_args()
    H, W = 1024, 2048
    res = {'shape': [H, W], 'nseg': a.nseg, 'pictures': a.pictures, 'k': 5,
           'byte_floor_per_picture': H * W * (1 + 2), 'byte_floor_note': 'u8 labels + u16 ids read once'}
    tmp = tempfile.mkdtemp(prefix='label_assign_probe_')
    try:
        t = time.perf_counter()
        n, distinct = (1, 1) if a.no_cli else (a.pictures, a.distinct)
        maps = build_pool(tmp, n, distinct, H, W, a.nseg)
        res['pool_build_s'] = round(time.perf_counter() - t, 1)
        res['kernel'] = kernel_times(maps, a.nseg, a.reps)
        if not a.no_cli:
            res['cli'] = cli_times(tmp, a.nseg, a.threads)
        if not a.no_host_loop:
            import label_assign_restated as R
            spx, lab = maps[0]
            t = time.perf_counter()
            R.multi_hot_loop(lab, spx, list(range(a.nseg)), a.nseg, 19, 5)
            res['restated_per_id_loop_host_s'] = round(time.perf_counter() - t, 2)
            res['restated_note'] = 'numpy restatement of the reference per-id loop (np.unique per id), one picture, host; not the reference tool'
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
