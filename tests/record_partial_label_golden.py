"""Records tests/golden/g14_partial_label.npz by EXECUTING the reference's partial-label baselines on the CPU (not collected; the only
file of the partial-label tests that reads the reference tree).  Run:  ``python tests/record_partial_label_golden.py``.

  rc_*       ``utils/loss.py:653-707`` RCMultiChoiceCE (C logits against C + 1 target columns, the last one dropped)
  topone_*   ``trainer/active_joint_multi_lossdecomp_topone.py:14-71`` OnehotCEMultihotTopone -> (ce, mc)

and, for each, the gradient of the weighted objective (16 * loss; 16 * ce + 8 * mc).  ``OnehotCEMultihotRC``
(``trainer/active_joint_multi_lossdecomp_rc.py``) is executed too and the exception it raises is recorded as text: it cannot run as
written.  Inputs are recorded by seed (``tests/test_losses_gpu.py:_inputs``), as g3_losses.npz does; the packages the reference
imports and never calls here come from ``oracle/refshim`` (torch_scatter, wandb, the data layer) and a ``tqdm`` stand-in."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import install as refshim  # noqa: E402
from mulactseg_amd import synth  # noqa: E402

SEED, N, C, H, W, S, T = 41, 2, 20, 40, 44, 48, 0.1


def inputs(seed, N, C, H, W, S, frac=0.25):
    z = synth.logits(seed, N, C, H, W)
    spx, msk = [], []
    for i in range(N):
        s, m = synth.train_crop(seed * 17 + i, H, W, S, frac_selected=frac)
        spx.append(s)
        msk.append(m)
    tgt = np.stack([synth.multi_hot_targets(seed * 19 + i, S, C) for i in range(N)])
    return z, tgt, np.stack(spx), np.stack(msk)


def main():
    refshim.install()
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules['tqdm'] = types.ModuleType('tqdm')
            sys.modules['tqdm'].tqdm = lambda it, **k: it
    import utils.loss as L
    z, tgt, spx, msk = inputs(SEED, N, C, H, W, S)
    tt, ts, tm = torch.from_numpy(tgt), torch.from_numpy(spx), torch.from_numpy(msk)
    ttb = torch.from_numpy(np.concatenate([tgt, np.zeros((N, S, 1), np.uint8)], axis=2))
    out = dict(seed=SEED, N=N, C=C, H=H, W=W, S=S, temp=T, w_ce=16.0, w_mc=8.0)

    zt = torch.from_numpy(z).clone().requires_grad_(True)
    loss = L.RCMultiChoiceCE(num_class=C, temperature=T)(zt, ttb, ts, tm)
    (g,) = torch.autograd.grad(16.0 * loss, zt)
    out['rc_loss'], out['rc_grad'] = np.float32(float(loss)), g.numpy()

    try:
        from trainer.active_joint_multi_lossdecomp_topone import OnehotCEMultihotTopone
        zt = torch.from_numpy(z).clone().requires_grad_(True)
        ce, mc = OnehotCEMultihotTopone(num_class=C, temperature=T)(zt, tt, ts, tm)
        (g,) = torch.autograd.grad(16.0 * ce + 8.0 * mc, zt)
        out['topone_ce'], out['topone_mc'], out['topone_grad'] = np.float32(float(ce)), np.float32(float(mc)), g.numpy()
        out['topone_recorded'] = True
    except ImportError as e:
        print("OnehotCEMultihotTopone not importable:", e)
        out['topone_recorded'] = False

    try:
        from trainer.active_joint_multi_lossdecomp_rc import OnehotCEMultihotRC
        zt = torch.from_numpy(z).clone().requires_grad_(True)
        OnehotCEMultihotRC(num_class=C, temperature=T)(zt, tt, ts, tm)
        out['rc_decomp_error'] = ''
    except Exception as e:      # noqa: BLE001 -- the finding is that it raises
        out['rc_decomp_error'] = '%s: %s' % (type(e).__name__, e)
    path = os.path.join(ROOT, "tests", "golden", "g14_partial_label.npz")
    np.savez_compressed(path, **out)
    print({k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
