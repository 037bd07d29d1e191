"""Records tests/golden/g18_wgroup.npz by EXECUTING the reference's teacher-weighted group loss on the CPU (not collected; the only
file of the wgroup tests that reads the reference tree).  Run:  ``python tests/record_wgroup_golden.py``.

  all_*     ``trainer/active_joint_multi_predignore_wgroup.py:12-82`` WeightedGroupMultiLabelCE at temperature 0.1, ``group_only_single`` False
  single_*  the same with ``group_only_single`` True (only superpixels with more than one target bit)

each with the counted ``n`` (``reduction='none'`` returns ``num_valid = 1 + n``), the loss and the gradient of the weighted objective
(16 * loss).  Inputs are those of g17, recorded by seed (``tests/test_losses_gpu.py:_inputs`` for the student, ``synth.logits`` of a
second seed for the teacher).  The student's arg-pixel is a discrete decision, so the recorder asserts in float64
(tests/test_wgroup_cpu.py:restated) that, for these seeds, no counted (superpixel, class) has its two largest student probabilities
within 1e-5 relative: no entry has to be left out of any comparison."""
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
from mulactseg_amd import synth  # noqa: E402
from record_partial_label_golden import inputs  # noqa: E402
from test_wgroup_cpu import restated  # noqa: E402

SEED, SEED_TEACHER, N, C, H, W, S, TEMP, WEIGHT = 41, 97, 2, 20, 40, 44, 48, 0.1, 16.0


def main():
    refshim.install()
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules['tqdm'] = types.ModuleType('tqdm')
            sys.modules['tqdm'].tqdm = lambda it, **k: it
    from trainer.active_joint_multi_predignore_wgroup import WeightedGroupMultiLabelCE
    z, tgt, spx, msk = inputs(SEED, N, C, H, W, S)
    zteach = synth.logits(SEED_TEACHER, N, C, H, W)
    tt, ts, tm = torch.from_numpy(tgt), torch.from_numpy(spx), torch.from_numpy(msk)
    out = dict(seed=SEED, seed_teacher=SEED_TEACHER, N=N, C=C, H=H, W=W, S=S, temp=TEMP, weight=WEIGHT)
    for key, single in (('all', False), ('single', True)):
        rl, rn, gap, (wlo, whi) = restated(z, zteach, tgt, spx, msk, TEMP, single)
        assert gap > 1e-5, (key, gap)
        args = types.SimpleNamespace(group_only_single=single)
        student = torch.from_numpy(z).clone().requires_grad_(True)
        loss = WeightedGroupMultiLabelCE(args, num_class=C, num_superpixel=S, temperature=TEMP)(student, torch.from_numpy(zteach), tt, ts, tm)
        (gr,) = torch.autograd.grad(WEIGHT * loss, student)
        with torch.no_grad():
            _, num_valid = WeightedGroupMultiLabelCE(args, num_class=C, num_superpixel=S, temperature=TEMP, reduction='none')(
                torch.from_numpy(z), torch.from_numpy(zteach), tt, ts, tm)
        n = int(num_valid) - 1
        assert n == rn, (key, n, rn)
        out[key + '_loss'], out[key + '_n'], out[key + '_grad'] = np.float32(float(loss)), n, gr.numpy()
        print(key, 'counted', n, 'loss', float(loss), 'restated', rl, 'min relative gap', gap, 'weights', wlo, whi)
    assert out['single_n'] < out['all_n']
    path = os.path.join(ROOT, "tests", "golden", "g18_wgroup.npz")
    np.savez_compressed(path, **out)
    print({k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
