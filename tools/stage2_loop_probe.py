#!/usr/bin/env python
"""Wall time per picture of the stage-2 pseudo-label generation LOOP (trainer/eval_save_cosplbl_prop*.py: forward at batch 1, K9 kernels,
IoU counters, one PNG per picture) on synthetic resident 1024 x 2048 pictures -- the loop, not only the kernels bench.py's stage2 leg times.

    python tools/stage2_loop_probe.py [--pictures 48] [--save_vis]
    python tools/stage2_loop_probe.py --threshold_ab --selected 0.15 --workers 1 4 --repeats 5 --json out.json

--threshold_ab: the prototype-threshold step (ops.stage2_thresholds) on the kernels and on the torch chain (MAS_STAGE2_THRESHOLD=aten, what
the step was before the kernels), interleaved in one process: the step alone on the assignment of a real picture, then the loop."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=48)
    ap.add_argument("--workers", type=int, nargs="+", default=[1, 2, 3, 4])
    ap.add_argument("--save_vis", action="store_true", help="also render and write the --save_vis picture of every label map")
    ap.add_argument("--selected", type=float, default=0.3, help="share of the superpixels that carry labels")
    ap.add_argument("--method", default="median", choices=["median", "min"], help="--cosprop_threshold_method of the loop")
    ap.add_argument("--threshold_ab", action="store_true", help="A/B of the threshold step: kernels against MAS_STAGE2_THRESHOLD=aten")
    ap.add_argument("--step_only", action="store_true", help="--threshold_ab: stop after the step alone (for a kernel trace)")
    ap.add_argument("--repeats", type=int, default=5, help="--threshold_ab: timed loops per (path, worker count)")
    ap.add_argument("--json", default=None, help="--threshold_ab: write the figures here")
    a = ap.parse_args()
    from mulactseg_amd import synth
    from mulactseg_amd.models import get_model
    from mulactseg_amd.trainer import eval_save_cosplbl_prop_includeonehot as G
    dev = torch.device('cuda:0')
    C, H, W, S = 19, 1024, 2048, 2048
    torch.manual_seed(2)
    net = get_model('deeplabv3pluswn_resnet50deepstem', C + 1, 16, True, pretrained_backbone=False).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(4)
    nbuf = 4
    pics = torch.randn((nbuf, 1, 3, H, W), generator=g, device=dev)
    spx = [torch.from_numpy(synth.superpixel_map(70 + i, H, W, S)[None]).to(dev) for i in range(nbuf)]
    rs = np.random.RandomState(5)
    samples = []
    for i in range(nbuf):
        lab = torch.from_numpy(rs.randint(0, C, size=(1, H, W))).to(dev)
        trg = torch.from_numpy((rs.rand(1, S, C + 1) < 0.1).astype(np.uint8))
        trg[..., C] = 0
        sel = torch.from_numpy(rs.rand(S) < a.selected)
        trg[0, ~sel] = 0
        trg = trg.to(dev)
        msk = (trg.sum(-1) > 0)[0][spx[i][0].long()][None]
        samples.append((lab, trg, msk))
    tmp = tempfile.mkdtemp(prefix="mas_s2_")

    class Loader:
        def __init__(self, n):
            self.n, self.k = n, 0

        def __len__(self):
            return self.n

        def __next__(self):
            i = self.k % nbuf
            self.k += 1
            lab, trg, msk = samples[i]
            return {'images': pics[i], 'labels': lab, 'spx': spx[i], 'spmask': msk, 'target': trg,
                    'fnames': [["i/p%05d.png" % self.k, "l/p%05d.png" % self.k, "s/p%05d.pkl" % self.k]]}
    import hashlib

    def loop(workers, pictures, tag):
        """(seconds, digest of the PNGs, IoU table) of one timed loop after a 6-picture warm-up."""
        os.environ["MAS_STAGE2_WORKERS"] = str(workers)
        run = tempfile.mkdtemp(prefix="%s_w%d_" % (tag, workers), dir=tmp)
        tr = object.__new__(G.ActiveTrainer)
        tr.args = types.SimpleNamespace(ignore_idx=255, init_checkpoint=os.path.join(run, "checkpoint01.tar"), plbl_type=None, val_batch_size=1,
                                        save_vis=a.save_vis, cosprop_threshold_method=a.method)
        tr.net, tr.device, tr.num_classes, tr.selection_iter, tr.save_dir = net, dev, C, 1, None
        tr.inference(Loader(6))                     # warm-up (first launches of the process, the threads' streams)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        miou, table = tr.inference(Loader(pictures))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        files = sorted(f for f in os.listdir(tr._save_dir()) if f.endswith(".png"))
        h = hashlib.sha256()
        for f in files:
            h.update(f.encode())
            h.update(open(os.path.join(tr._save_dir(), f), "rb").read())
        return dt, h.hexdigest(), table, len(files)

    if a.threshold_ab:
        return threshold_ab(a, loop, samples, spx, pics, net)
    results = {}
    for workers in a.workers:
        dt, digest, table, nfiles = loop(workers, a.pictures, "run")
        results[workers] = (digest, table)
        print(("--save_vis " if a.save_vis else "") + "MAS_STAGE2_WORKERS=%d: %d pictures in %.2f s = %.1f ms per picture; %d PNGs, sha256 over names and bytes %s"
              % (workers, a.pictures, dt, dt / a.pictures * 1e3, nfiles, digest[:16]), flush=True)
    same = len(set(results.values())) == 1
    print("PNG files and IoU table identical for every worker count" if same else "MISMATCH between worker counts")
    return 0 if same else 1


def threshold_ab(a, loop, samples, spx, pics, net):
    from mulactseg_amd import ops
    paths = ("aten", "kernel")
    out = {"shape": "1024x2048, 2048 superpixels, %.0f %% selected" % (100 * a.selected), "method": a.method, "pictures": a.pictures,
           "repeats": a.repeats, "step": {}, "loop_ms_per_picture": {}}
    # the step alone, on the assignment (nn, nn_sim) of the first picture
    seen = []
    real = ops.stage2_thresholds

    def record(nn, nn_sim, n_proto, method='median'):
        seen.append((nn.clone(), nn_sim.clone(), n_proto))
        return real(nn, nn_sim, n_proto, method)
    ops.stage2_thresholds = record
    try:
        with torch.no_grad():
            lab, trg, msk = samples[0]
            feats, logits = net.feat_forward_lowres(pics[0])
            ops.stage2_pseudo_labels(feats.contiguous(), logits.contiguous(), trg, msk, spx[0], True, threshold_method=a.method)
    finally:
        ops.stage2_thresholds = real
    nn, nn_sim, n_proto = seen[0]
    out["n_proto"], out["assigned_pixels"], out["HW"] = n_proto, int((nn >= 0).sum()), nn.numel()
    out["byte_floor_per_pass_MB"] = nn.numel() * 8 / 1e6
    calls = 50
    for method in ("median", "min"):
        for rep in range(3):
            for path in paths:
                os.environ["MAS_STAGE2_THRESHOLD"] = path
                for _ in range(3):
                    ops.stage2_thresholds(nn, nn_sim, n_proto, method)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(calls):
                    ops.stage2_thresholds(nn, nn_sim, n_proto, method)
                e1.record()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / calls * 1e6
                out["step"].setdefault("%s/%s" % (method, path), []).append({"device_us": e0.elapsed_time(e1) / calls * 1e3, "wall_us": wall})
        os.environ["MAS_STAGE2_THRESHOLD"] = "aten"
        want = ops.stage2_thresholds(nn, nn_sim, n_proto, method)
        os.environ["MAS_STAGE2_THRESHOLD"] = "kernel"
        assert torch.equal(want, ops.stage2_thresholds(nn, nn_sim, n_proto, method)), method
    for key, runs in out["step"].items():
        print("threshold step %-14s device %s us, wall %s us per call" % (key, ["%.1f" % r["device_us"] for r in runs], ["%.1f" % r["wall_us"] for r in runs]),
              flush=True)
    if a.step_only:
        return 0
    # the loop, interleaved
    digests = set()
    for workers in a.workers:
        for rep in range(a.repeats):
            for path in paths:
                os.environ["MAS_STAGE2_THRESHOLD"] = path
                dt, digest, table, _ = loop(workers, a.pictures, path)
                digests.add((digest, table))
                out["loop_ms_per_picture"].setdefault("%s/workers=%d" % (path, workers), []).append(dt / a.pictures * 1e3)
    os.environ.pop("MAS_STAGE2_THRESHOLD", None)
    for key, v in out["loop_ms_per_picture"].items():
        print("loop %-18s %s ms per picture (min %.2f, max %.2f)" % (key, ["%.2f" % x for x in v], min(v), max(v)), flush=True)
    out["same_files"] = len(digests) == 1
    print("PNG files and IoU table identical on both paths and every worker count" if out["same_files"] else "MISMATCH")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if out["same_files"] else 1


if __name__ == "__main__":
    sys.exit(main())
