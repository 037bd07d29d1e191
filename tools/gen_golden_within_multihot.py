"""Generate ``tests/golden/g21_within_multihot.npz`` by EXECUTING THE REFERENCE'S OWN ``inference()`` LOOPS of the four evaluators of the
local-prototype labels inside the queried superpixels (build container only; needs the reference tree, see ``oracle/refshim/install.py``):

    trainer/eval_cosplbl_within_multihot.py        nearest local prototype; IoU, precision and recall tables
    trainer/eval_cosplbl_filt_within_multihot.py   ... kept where it equals the model's arg-max, prototype pixels restored; one table
    trainer/eval_maxcosplbl_within_multihot.py     the labels of the first; prints per picture how many winning similarities lie
                                                   below max_c (logit_c * Y_c); one table
    trainer/eval_ensemble_plbl_within_multihot.py  the labels of the first; one table

Run:  ``python tools/gen_golden_within_multihot.py``.  Nothing of the reference is copied: its ``ActiveTrainer`` classes are imported from
where they lie and run against stubs (a ``net`` whose ``feat_forward`` returns the seeded features and logits of the current picture --
the bilinear upsampling of the seeded quarter-resolution maps, which is what the reference's ``feat_forward`` returns --, a loader that
deals the seeded pictures one per batch, an ``args`` namespace); the label maps are taken from ``pseudo_label_generation``'s return
value and everything the loops print is captured.  Inputs: ``tests/within_eval_restated.inputs()`` (the geometry of g15, three
pictures, the third with nothing selected).  The fixture holds the seed, the input digest, the two label maps, the captured output and
the returned table string of each evaluator, the counts ``maxcos`` printed and the float64 margin of that count, ``sim_err_ref`` (the largest |float32 - float64| inner
product of the reference's own ``torch.mm`` on these inputs) and, per mode, the float64 margin of every valid pixel
(``tests/within_eval_restated.generate``).  Conditions the tests rely on are asserted here; if one fails, change the seed, not the
bound.  The archive is written with fixed member dates, so a rerun reproduces it byte for byte.
"""
import contextlib
import importlib
import io
import os
import re
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.refshim import install as refshim  # noqa: E402
from oracle.gen_golden import digest  # noqa: E402
from tools.gen_golden_stage2_variants import save_fixed  # noqa: E402
import online_plbl_restated as O  # noqa: E402
import within_eval_restated as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g21_within_multihot.npz")
EVALUATORS = (('cosplbl', 'trainer.eval_cosplbl_within_multihot'), ('filt', 'trainer.eval_cosplbl_filt_within_multihot'),
              ('maxcos', 'trainer.eval_maxcosplbl_within_multihot'), ('ensemble', 'trainer.eval_ensemble_plbl_within_multihot'))


class Net:
    """``feat_forward`` of the current picture: the loader tells which one it dealt last."""

    def __init__(self, feats, logits, loader):
        self.feats, self.logits, self.loader = feats, logits, loader

    def eval(self):
        return self

    def set_return_feat(self):
        pass

    def feat_forward(self, images):
        i = self.loader.current
        return self.feats[i:i + 1], self.logits[i:i + 1]


class Loader:
    def __init__(self, labels, spx, msk, tgt):
        self.labels, self.spx, self.msk, self.tgt = labels, spx, msk, tgt
        self.current = -1

    def __len__(self):
        return self.labels.shape[0]

    def __next__(self):
        self.current = i = (self.current + 1) % len(self)
        return {'images': torch.zeros((1, 3, R.H, R.W)), 'labels': self.labels[i:i + 1], 'spx': self.spx[i:i + 1],
                'spmask': self.msk[i:i + 1], 'target': self.tgt[i:i + 1]}


def run(modname, tensors):
    """-> (label maps uint8 [N,H,W] as ``pseudo_label_generation`` returned them, the returned table string, the captured output)"""
    feats, z, tgt, spx, msk, labels = tensors
    T = importlib.import_module(modname).ActiveTrainer
    loader = Loader(labels, spx, msk, tgt)
    tr = T.__new__(T)
    tr.args = types.SimpleNamespace(nseg=R.S, ignore_idx=R.IGNORE)
    tr.net, tr.num_classes, tr.device, tr.selection_iter = Net(feats, z, loader), R.C - 1, 'cpu', 0
    maps = []
    generate = tr.pseudo_label_generation

    def recording(*a, **k):
        out = generate(*a, **k)
        maps.append(out.clone())
        return out
    tr.pseudo_label_generation = recording
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        _, table = tr.inference(loader, prefix='evaluation')
    maps = torch.cat(maps).numpy()
    assert maps.shape == (R.N, R.H, R.W) and maps.min() >= 0 and maps.max() <= 255
    return maps.astype(np.uint8), table, buf.getvalue()


def main():
    torch.set_num_threads(1)
    refshim.install()
    zq, featq, tgt, spx, msk, gt = R.inputs()
    size = (R.H, R.W)
    logits, feats = O.upsample(zq, size), O.upsample(featq, size)
    tensors = (feats, logits) + tuple(torch.from_numpy(a) for a in (tgt, spx, msk, gt))
    out = dict(seed=R.SEED, N=R.N, C=R.C, Ch=R.CH, H=R.H, W=R.W, hq=R.HQ, wq=R.WQ, S=R.S, input_digest=digest(zq, featq, tgt, spx, msk, gt))

    # what the issue of this fixture asks of the inputs
    assert not msk[2].any() and msk[0].any() and msk[1].any()
    n_rows = tgt.sum(axis=2)
    assert n_rows.min() >= 1, "a superpixel with an empty row: the reference raises on it when it is selected"
    selected = [np.unique(spx[i][msk[i]]) for i in range(R.N)]
    assert all(u.size == 0 or (u.min() >= 0 and u.max() < R.S) for u in selected)
    hot = np.concatenate([n_rows[i][u] for i, u in enumerate(selected)])
    assert (hot == 1).any() and (hot >= 2).any() and hot.max() <= 4, "one-hot and 2-4-hot rows must both be selected"
    assert any(len(u) < R.S for u in selected[:2]), "no row is set for a superpixel without a valid pixel"

    maps = {}
    for name, modname in EVALUATORS:
        maps[name], table, printed = run(modname, tensors)
        out['table_' + name], out['stdout_' + name] = np.str_(table), np.str_(printed)
        print("g21 %-8s %s" % (name, table[:40]))
    assert np.array_equal(maps['cosplbl'], maps['maxcos']) and np.array_equal(maps['cosplbl'], maps['ensemble'])
    out['plbl_proto'], out['plbl_filt'] = maps['cosplbl'], maps['filt']
    out['maxcos_counts'] = np.asarray([int(v) for v in re.findall(r"tensor\((\d+)\)", str(out['stdout_maxcos']))], dtype=np.int64)
    assert out['maxcos_counts'].size == 2                     # one line per picture with a selected pixel

    err = R.sim_err_f32(feats, torch.from_numpy(msk))
    out['sim_err_ref'] = np.float64(err)
    valid = msk & (n_rows[np.arange(R.N)[:, None, None], np.minimum(spx, R.S - 1)] > 0) & (spx < R.S)
    assert np.array_equal(maps['cosplbl'] != 255, valid)
    n_valid = int(valid.sum())
    for mode, key in (('proto', 'gap64'), ('filt', 'gap64_filt')):
        r = R.generate(logits, feats, tgt, spx, msk, mode)
        assert np.array_equal(r['valid'], valid)
        close = int((r['gap'][valid] <= 8 * err).sum())
        assert n_valid >= 500 and 200 * close <= n_valid, "%d of %d valid pixels lie within 8 * sim_err_ref of a tie" % (close, n_valid)
        decided = valid & (r['gap'] > 8 * err)
        assert np.array_equal(r['labels'][decided], maps['cosplbl' if mode == 'proto' else 'filt'][decided].astype(np.int64))
        out[key] = r['gap']
        print("g21 %-5s valid %d, near ties %d, float64 agreement on the rest, kept by the mode %d"
              % (mode, n_valid, close, int((maps['cosplbl' if mode == 'proto' else 'filt'][valid] != 255).sum())))
        if mode == 'proto':
            out['maxcos_margin64'] = np.float64(r['below_margin'])
            assert r['below_margin'] > 8 * err and np.array_equal(r['below'][:2], out['maxcos_counts']), \
                "a winning similarity lies within 8 * sim_err_ref of max_c (logit_c * Y_c): the printed count depends on rounding"
            print("g21 maxcos printed %s, float64 restatement %s" % (out['maxcos_counts'].tolist(), r['below'].tolist()))
    save_fixed(OUT, out)
    print("g21: sim_err_ref %.3e; wrote %s (%d bytes)" % (err, OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
