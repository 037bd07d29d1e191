"""Records tests/golden/g20_async_hier.npz by EXECUTING the reference's cross-view hierarchical group losses on the CPU (not collected;
the only file of the async-hier tests that reads the reference tree).  Run:  ``python tests/record_async_hier_golden.py``.

  async_*  ``utils/loss.py:341-437`` AsyncHierGroupMultiLabelCE
  wmax_* / wmean_*  ``utils/loss.py:237-339`` WeightAsyncHierGroupMultiLabelCE with ``weight_reduce`` 'max' / 'mean'
  *_<Ss>: a fine map of Ss = 192 and of Ss = 12 superpixels

each with the counted ``n`` (``reduction='none'`` returns ``num_valid = 1 + n``), the ``reduction='none'`` sum, the loss and the
gradient of 16 * loss, at N = 2, C = 20 logits against 21 target columns (the last one zero).

The WEAK view is exactly g19's input: ``record_partial_label_golden.inputs(41, 2, 20, 40, 44, 48)`` with
``test_hier_group_cpu.small_map`` and ``with_last_column``.  The STRONG view is rows 5..29 and columns 8..40 of the weak maps and mask,
flipped left-right, with the logits ``synth.logits(7, 2, 20, 24, 32)`` (``test_async_hier_cpu.views``).

The arg-pixel is a discrete decision.  The recorder asserts in float64 (``test_hier_group_cpu.restated``) that for every pair the best
selected weak pixel lying in a DIFFERENT fine superpixel is more than 1e-5 relative below the maximum: no entry has to be left out of
any comparison.  It also asserts the counts of the issue, that no pair over a non-empty fine superpixel has value or weight 0 (where
the reference's ``size[value.nonzero()]`` and this project's ``wgt != 0`` would part), that Ss = 12 holds a pair of multiplicity >= 2,
and that at least one pair's fine superpixel is absent from the strong window; and prints how far the executed reference lies from the
float64 restatement (``test_async_hier_cpu.restated_async``)."""
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
from test_async_hier_cpu import C, HO, ISSUE, KEYS, N, S, SEED, WO, restated_async, views  # noqa: E402

WEIGHT = 16.0


def main():
    refshim.install()
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules['tqdm'] = types.ModuleType('tqdm')
            sys.modules['tqdm'].tqdm = lambda it, **k: it
    import utils.loss as L
    out = dict(seed=SEED, N=N, C=C, H=HO, W=WO, S=S, weight=WEIGHT)
    worst_loss = worst_grad = 0.0
    for Ss in (192, 12):
        v = views(Ss)
        zw = inputs(SEED, N, C, HO, WO, S)[0]
        assert np.array_equal(zw, v['zw'])                    # the weak view is g19's input
        t = {k: torch.from_numpy(a) for k, a in v.items()}
        args = types.SimpleNamespace(small_nseg=Ss)
        for key, reduce in KEYS.items():
            k = "%s_%d" % (key, Ss)
            r = restated_async(v, Ss, reduce, upstream=WEIGHT)
            assert r['gap'] > 1e-5, (k, r['gap'])
            pairs = r['mult'] > 0
            present = pairs & (r['size'] > 0)[..., None]
            assert np.all(r['value'][present] != 0)           # no pair over a non-empty fine superpixel has value 0 ...
            if r['wgt'] is not None:
                assert np.all(r['wgt'][pairs] != 0)           # ... or weight 0
            kw = {} if reduce is None else dict(weight_reduce=reduce)
            cls = L.AsyncHierGroupMultiLabelCE if reduce is None else L.WeightAsyncHierGroupMultiLabelCE

            def run(z, reduction):
                crit = cls(args, C, S, False, -1, reduction=reduction, temperature=0.1, **kw)
                return crit(z, t['zw'], t['tgt'].clone(), t['msk'], t['msk_w'], t['spx'], t['spx_w'], t['small'], t['small_w'])
            zt = t['z'].clone().requires_grad_(True)
            loss = run(zt, 'mean')
            (gr,) = torch.autograd.grad(WEIGHT * loss, zt)
            with torch.no_grad():
                total, num_valid = run(t['z'], 'none')
            n = int(num_valid) - 1
            assert n == r['n'] == ISSUE[Ss][0], (k, n, r['n'])
            want = ISSUE[Ss][1 + list(KEYS).index(key)]
            assert abs(float(total) - want) <= 5e-4, (k, float(total), want)
            dl = abs(float(loss) - r['loss']) / abs(r['loss'])
            dg = float(np.max(np.abs(gr.numpy() - r['grad']))) / float(np.max(np.abs(r['grad'])))
            worst_loss, worst_grad = max(worst_loss, dl), max(worst_grad, dg)
            out[k + '_n'], out[k + '_sum'], out[k + '_loss'], out[k + '_grad'] = n, np.float32(float(total)), np.float32(float(loss)), gr.numpy()
            print(k, 'counted', n, 'sum', float(total), 'loss', float(loss), 'restated', r['loss'], 'min gap', r['gap'],
                  'reference vs float64: loss %.3e grad %.3e' % (dl, dg))
        r = restated_async(v, Ss)
        out['max_mult_%d' % Ss] = int(r['mult'].max())
        out['absent_pairs_%d' % Ss] = int(((r['mult'] > 0).any(axis=2) & (r['size'] == 0)).sum())
        print('Ss', Ss, 'pairs', int((r['mult'] > 0).sum()), 'max mult', out['max_mult_%d' % Ss], 'fine superpixels with a pair and no '
              'selected strong pixel', out['absent_pairs_%d' % Ss])
    assert out['max_mult_12'] >= 2 and out['absent_pairs_192'] > 0
    out['worst_loss'], out['worst_grad'] = worst_loss, worst_grad
    print('executed reference against the float64 restatement, worst of the six cases: loss %.3e relative, gradient %.3e of max|grad|'
          % (worst_loss, worst_grad))
    path = os.path.join(ROOT, "tests", "golden", "g20_async_hier.npz")
    np.savez_compressed(path, **out)
    print({k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
