"""Generate ``tests/golden/g12_stage2_variants.npz`` by EXECUTING THE REFERENCE'S OWN ``inference()`` LOOPS of the four stage-2
generators without expansion (build container only; needs the reference tree, see ``oracle/refshim/install.py``):

    trainer/eval_save_cosplbl.py            prototype assignment, no expansion                        (Table 2, second row)
    trainer/eval_save_cosplbl_naiveprop.py  ... plus top-1 with softmax(z / ce_temp).max > plbl_th outside the selected superpixels
    trainer/eval_save_candidateplbl.py      arg-max within the superpixel's candidate set
    trainer/eval_save_candidateplbl_prop.py ... plus the same thresholded fallback

Run:  ``python tools/gen_golden_stage2_variants.py``.  Nothing of the reference is copied: its ``ActiveTrainer`` classes are imported
from where they lie and run against stubs (a ``net`` whose ``feat_forward`` returns the seeded features and logits of the current
picture, a loader that deals the seeded pictures, an ``args`` namespace), and the PNGs they save are read back.  Inputs: the G6 inputs,
``stage2_inputs(61, 3, 20, 16, 40, 56, 36)`` (the third picture has nothing selected).  The fixture holds the seed, the input digest,
the saved label maps (uint8) and the returned IoU table strings; for the two generators with the fallback per
``(plbl_th, ce_temp)`` of ``SETTINGS``.  The archive is written with fixed member dates, so a rerun reproduces it byte for byte.
"""
import importlib
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.refshim import install as refshim  # noqa: E402
from oracle.gen_golden import digest, stage2_inputs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g12_stage2_variants.npz")
SEED, N, C, CH, H, W, S = 61, 3, 20, 16, 40, 56, 36
SETTINGS = ((0.0, 1.0), (0.1, 1.0), (0.9, 0.1))         # (plbl_th, ce_temp): keep 100 %, 43 % and 29 % of the unqueried pixels
GENERATORS = (('cosplbl', 'trainer.eval_save_cosplbl', False), ('naiveprop', 'trainer.eval_save_cosplbl_naiveprop', True),
              ('candidate', 'trainer.eval_save_candidateplbl', False), ('candprop', 'trainer.eval_save_candidateplbl_prop', True))


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
        self.dataset = types.SimpleNamespace(decode_target=lambda t: np.zeros(tuple(t.shape) + (3,), dtype=np.uint8))
        self.current = -1

    def __len__(self):
        return self.labels.shape[0]

    def __next__(self):
        self.current = i = (self.current + 1) % len(self)
        return {'images': torch.zeros((1, 3, H, W)), 'labels': self.labels[i:i + 1], 'spx': self.spx[i:i + 1],
                'spmask': self.msk[i:i + 1], 'target': self.tgt[i:i + 1],
                'fnames': [('leftImg8bit/pic_%d.png' % i, 'gtFine/pic_%d.png' % i, 'superpixel/pic_%d.pkl' % i)]}


def run(modname, tensors, plbl_type, plbl_th, ce_temp):
    """-> (label maps uint8 [N,H,W] read back from the PNGs the reference saved, its IoU table string, the directory's name)."""
    from PIL import Image
    feats, z, tgt, spx, msk, labels = tensors
    T = importlib.import_module(modname).ActiveTrainer
    with tempfile.TemporaryDirectory() as tmp:
        loader = Loader(labels, spx, msk, tgt)
        tr = T.__new__(T)
        tr.args = types.SimpleNamespace(nseg=S, ignore_idx=255, init_checkpoint=os.path.join(tmp, 'checkpoint01.tar'), plbl_type=plbl_type,
                                        save_vis=False, plbl_th=plbl_th, ce_temp=ce_temp)
        tr.net, tr.num_classes, tr.device, tr.selection_iter = Net(feats, z, loader), C - 1, 'cpu', 0
        _, table = tr.inference(loader, prefix='evaluation')
        (sub,) = [d for d in os.listdir(tmp) if d.startswith('plbl_gen')]
        d = os.path.join(tmp, sub, 'round_01')
        maps = np.stack([np.array(Image.open(os.path.join(d, 'pic_%d.png' % i))) for i in range(N)])
    assert maps.dtype == np.uint8 and maps.shape == (N, H, W)
    return maps, table, sub


def save_fixed(path, arrays):
    """``np.savez_compressed`` with fixed member dates (numpy stamps the members with the clock)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(1)
    refshim.install()
    feats, z, tgt, spx, msk, labels = stage2_inputs(SEED, N, C, CH, H, W, S)
    tensors = tuple(torch.from_numpy(a) for a in (feats, z, tgt, spx, msk, labels))
    out = dict(seed=SEED, N=N, C=C, Ch=CH, H=H, W=W, S=S, input_digest=digest(feats, z, tgt, spx, msk), labels_digest=digest(labels),
               settings=np.asarray(SETTINGS, dtype=np.float64))
    unq = ~msk
    for tag, modname, has_fallback in GENERATORS:
        for k, (th, temp) in enumerate(SETTINGS if has_fallback else ((0.0, 1.0),)):
            key = '%s_%d' % (tag, k) if has_fallback else tag
            maps, table, sub = run(modname, tensors, None, th, temp)
            out['plbl_' + key], out['table_' + key], out['dir_' + key] = maps, np.str_(table), np.str_(sub)
            print("g12 %-12s th %.1f T %.1f -> %s: %5.1f %% of the unqueried pixels labelled, %5.1f %% of the selected; %s"
                  % (key, th, temp, sub, 100.0 * (maps[unq] != 255).mean(), 100.0 * (maps[msk] != 255).mean(), table[:24]))
    # the quirk of top_pseudo_label_generation: selected pixels whose candidate logits are all negative take an excluded channel
    rows = tgt[np.arange(N)[:, None, None], spx]
    lab = out['plbl_candidate'].astype(np.int64)
    excluded = msk & (np.take_along_axis(rows, np.minimum(lab, C - 1)[..., None], axis=3)[..., 0] == 0)
    print("g12: %.0f %% of the selected pixels carry a label outside their candidate set" % (100.0 * excluded.sum() / msk.sum()))
    save_fixed(OUT, out)
    print("g12: wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
