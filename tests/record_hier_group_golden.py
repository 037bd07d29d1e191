"""Records tests/golden/g19_hier_group.npz by EXECUTING the reference's hierarchical group losses on the CPU (not collected; the only
file of the hier-group tests that reads the reference tree).  Run:  ``python tests/record_hier_group_golden.py``.

  hier_*  ``utils/loss.py:143-235`` HierGroupMultiLabelCE          aug_*  ``utils/loss.py:439-533`` AugHierGroupMultiLabelCE (--nocropsp)
  *_all_<Ss> / *_single_<Ss>: ``only_single`` False / True with a fine map of Ss = 192 and of Ss = 12 superpixels

each with the counted ``n`` (``reduction='none'`` returns ``num_valid = 1 + n``), the loss and the gradient of 16 * loss, at N = 2,
C = 20 logits against 21 target columns (the last one zero).  Inputs are those of g14 / g18 by seed
(``record_partial_label_golden.inputs``); the fine map is ``synth.superpixel_map(seed * 23 + i, H, W, Ss)`` with the pad pixels set to
Ss (``test_hier_group_cpu.small_map``).  For ``aug`` the merged-positive loss (``MultiChoiceCE`` at temperature 0.1) and its count are
recorded on the labels the reference has modified in place, beside the count on the untouched labels and the number of rows that changed.

The arg-pixel is a discrete decision.  The recorder asserts in float64 (``test_hier_group_cpu.restated``) that for every counted pair
the best selected pixel lying in a DIFFERENT fine superpixel is more than 1e-5 relative below the maximum: no entry has to be left out
of any comparison.  It also asserts that Ss = 12 holds a pair of multiplicity 2 and Ss = 192 none, and prints how far the executed
reference lies from the float64 restatement."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import install as refshim  # noqa: E402
from record_partial_label_golden import inputs  # noqa: E402
from test_hier_group_cpu import cleared_rows, restated, restated_pos, small_map, with_last_column  # noqa: E402

SEED, N, C, H, W, S, WEIGHT, POS_TEMP = 41, 2, 20, 40, 44, 48, 16.0, 0.1


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
    tgt = with_last_column(tgt)
    ts, tm = torch.from_numpy(spx), torch.from_numpy(msk)
    out = dict(seed=SEED, N=N, C=C, H=H, W=W, S=S, weight=WEIGHT, pos_temp=POS_TEMP)
    worst_loss = worst_grad = 0.0
    for Ss in (192, 12):
        small = small_map(SEED, spx, S, Ss)
        tf = torch.from_numpy(small)
        args = types.SimpleNamespace(small_nseg=Ss)
        for name, cls, aug in (('hier', L.HierGroupMultiLabelCE, False), ('aug', L.AugHierGroupMultiLabelCE, True)):
            for sub, single in (('all', False), ('single', True)):
                key = "%s_%s_%d" % (name, sub, Ss)
                r = restated(z, tgt, spx, small, msk, Ss, single, aug, upstream=WEIGHT)
                assert r['gap'] > 1e-5, (key, r['gap'])
                zt = torch.from_numpy(z).clone().requires_grad_(True)
                labels = torch.from_numpy(tgt.copy())
                loss = cls(args, C, S, single, -1, temperature=0.1)(zt, labels, tm, ts, tf)
                (gr,) = torch.autograd.grad(WEIGHT * loss, zt)
                with torch.no_grad():
                    _, num_valid = cls(args, C, S, single, -1, reduction='none')(torch.from_numpy(z), torch.from_numpy(tgt.copy()), tm, ts, tf)
                n = int(num_valid) - 1
                assert n == r['n'], (key, n, r['n'])
                dl = abs(float(loss) - r['loss']) / abs(r['loss'])
                dg = float(np.max(np.abs(gr.numpy() - r['grad']))) / float(np.max(np.abs(r['grad'])))
                worst_loss, worst_grad = max(worst_loss, dl), max(worst_grad, dg)
                out[key + '_loss'], out[key + '_n'], out[key + '_grad'] = np.float32(float(loss)), n, gr.numpy()
                print(key, 'counted', n, 'loss', float(loss), 'restated', r['loss'], 'min gap', r['gap'], 'max mult', int(r['mult'].max()),
                      'reference vs float64: loss %.3e grad %.3e' % (dl, dg))
                if aug and not single and Ss == 12:
                    changed = int((labels.numpy() != tgt).any(axis=2).sum())
                    assert np.array_equal(labels.numpy(), cleared_rows(tgt, spx, S))
                    with torch.no_grad():
                        pos = L.MultiChoiceCE(C, temperature=POS_TEMP)(torch.from_numpy(z), labels, ts, tm)
                        _, pn = L.MultiChoiceCE(C, temperature=POS_TEMP, reduction='none')(torch.from_numpy(z), labels, ts, tm)
                        _, pn0 = L.MultiChoiceCE(C, temperature=POS_TEMP, reduction='none')(torch.from_numpy(z), torch.from_numpy(tgt), ts, tm)
                    rl, rn = restated_pos(z, labels.numpy()[..., :C], spx, msk, POS_TEMP)
                    assert rn == int(pn) - 1
                    out.update(rows_changed=changed, aug_pos_loss=np.float32(float(pos)), aug_pos_n=int(pn) - 1, pos_n=int(pn0) - 1)
                    print('nocropsp: rows changed', changed, 'of', N * S, 'merged-positive count', int(pn0) - 1, '->', int(pn) - 1,
                          'loss', float(pos), 'restated', rl)
        out['max_mult_%d' % Ss] = int(restated(z, tgt, spx, small, msk, Ss, False)['mult'].max())
    assert out['max_mult_12'] >= 2 and out['max_mult_192'] == 1
    print('executed reference against the float64 restatement, worst of the eight cases: loss %.3e relative, gradient %.3e of max|grad|'
          % (worst_loss, worst_grad))
    path = os.path.join(ROOT, "tests", "golden", "g19_hier_group.npz")
    np.savez_compressed(path, **out)
    print({k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
