"""Records tests/golden/g15_online_plbl.npz by EXECUTING the reference's online pseudo-label losses on the CPU (not collected; the only
file of the online-plbl tests that reads the reference tree).  Run:  ``python tests/record_online_plbl_golden.py``.

  LocalProtoCE        ``trainer/active_onlineplbl_multi_predignore.py:14-141``        -> plain_loss, plain_grad
  LocalWProtoCE       ``trainer/active_onlinewplbl_multi_predignore.py:15-148``       -> labels, weight, w_loss, w_grad; with
                      ``--weight_wo_proto``: weight_wo, wo_loss, wo_grad; with ``--th_wplbl``: th_loss, th_grad
  JointLocalProtoCE   ``trainer/active_onlinewplblonly_multi_predignore.py:15-137``   -> joint_loss

Inputs are recorded by seed (``online_plbl_restated.inputs``, which the tests call too): quarter-resolution logits of the pseudo-label forward and of
the training forward, normalised quarter-resolution features; the reference sees their ``F.interpolate(bilinear)`` to the picture
size, which is what its ``net(x)`` / ``feat_forward`` return.  Gradients are with respect to the full-resolution training logits.
Also recorded: ``gap64`` (the float64 best-vs-second similarity gap of every valid pixel, tests/online_plbl_restated.py) and
``sim_err_ref``, the largest |float32 - float64| similarity of the reference's own ``torch.mm`` on these inputs.  Two conditions the
tests rely on are asserted here; if one fails, change the seed, not the bound."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from online_plbl_restated import SEED, N, C, CH, H, W, HQ, WQ, S, T, TH, inputs, upsample  # noqa: E402


def main():
    import install as refshim
    import online_plbl_restated as R
    refshim.install()
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules['tqdm'] = types.ModuleType('tqdm')
            sys.modules['tqdm'].tqdm = lambda it, **k: it
    from trainer.active_onlineplbl_multi_predignore import LocalProtoCE
    from trainer.active_onlinewplbl_multi_predignore import LocalWProtoCE
    from trainer.active_onlinewplblonly_multi_predignore import JointLocalProtoCE

    zq_p, featq, zq, tgt, spx, msk = inputs()
    logits_p, feats, logits = upsample(zq_p, (H, W)), upsample(featq, (H, W)), upsample(zq, (H, W))
    tt, ts, tm = torch.from_numpy(tgt), torch.from_numpy(spx), torch.from_numpy(msk)

    selected = [np.unique(spx[i][msk[i]]) for i in range(N)]
    n_sel = sum(len(u) for u in selected)
    n_multi = sum(int((tgt[i][u].sum(1) > 1).sum()) for i, u in enumerate(selected))
    assert 3 * n_multi >= n_sel, "fewer than a third of the selected superpixels are multi-hot: %d of %d" % (n_multi, n_sel)

    def args(**kw):
        return types.SimpleNamespace(nseg=S, weight_wo_proto=kw.get('wo', False), th_wplbl=kw.get('th'))

    def run(cls, **kw):
        crit = cls(args=args(**kw), num_superpixel=S, temperature=T)
        z = logits.clone().requires_grad_(True)
        loss = crit(logits_p, feats, z, tt, ts, tm)
        (g,) = torch.autograd.grad(loss, z)
        return np.float32(float(loss)), g.numpy()

    out = dict(seed=SEED, N=N, C=C, Ch=CH, H=H, W=W, hq=HQ, wq=WQ, S=S, temp=T, th=TH)
    out['plain_loss'], out['plain_grad'] = run(LocalProtoCE)
    out['w_loss'], out['w_grad'] = run(LocalWProtoCE)
    out['wo_loss'], out['wo_grad'] = run(LocalWProtoCE, wo=True)
    out['th_loss'], out['th_grad'] = run(LocalWProtoCE, th=TH)
    out['joint_loss'], _ = run(JointLocalProtoCE)
    with torch.no_grad():
        w, lab = LocalWProtoCE(args=args(), num_superpixel=S, temperature=T).generate_plbl(logits_p, feats, tt, ts, tm)
        w_wo, lab_wo = LocalWProtoCE(args=args(wo=True), num_superpixel=S, temperature=T).generate_plbl(logits_p, feats, tt, ts, tm)
        lab_plain = LocalProtoCE(args=args(), num_superpixel=S, temperature=T).generate_plbl(logits_p, feats, tt, ts, tm)
    assert torch.equal(lab, lab_wo) and torch.equal(lab, lab_plain)
    out['labels'], out['weight'], out['weight_wo'] = lab.numpy().astype(np.uint8), w.numpy(), w_wo.numpy()

    # the reference's own float32 similarity error on these inputs, and the float64 margins of the labels
    err = 0.0
    for i in range(N):
        vf = feats[i].permute(1, 2, 0).reshape(-1, CH)[tm[i].reshape(-1)]
        err = max(err, float((torch.mm(vf, vf.T).double() - torch.mm(vf.double(), vf.double().T)).abs().max()))
    out['sim_err_ref'] = np.float64(err)
    lab64, _, gap64 = R.generate(logits_p, feats, tgt, spx, msk, T)
    valid = lab64 != 255
    n_valid = int(valid.sum())
    close = int((gap64[valid] <= 8 * err).sum())
    assert 200 * close < n_valid, "%d of %d valid pixels lie within 8 * sim_err_ref of a tie" % (close, n_valid)
    out['gap64'] = gap64.numpy()
    ce = F.cross_entropy(logits.double() / T, lab.long(), ignore_index=255, reduction='none')
    assert float(ce[lab != 255].min()) >= 1e-6, "a labelled pixel has ce < 1e-6: the non-zero count would be ambiguous"
    agree = float((lab64[valid] == lab.long()[valid]).double().mean())
    path = os.path.join(ROOT, "tests", "golden", "g15_online_plbl.npz")
    np.savez_compressed(path, **out)
    print({k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in out.items()})
    print("valid pixels %d, near ties %d, float64 agreement %.6f, multi-hot superpixels %d of %d, bytes %d"
          % (n_valid, close, agree, n_multi, n_sel, os.path.getsize(path)))


if __name__ == "__main__":
    main()
