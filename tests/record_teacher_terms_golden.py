"""Records tests/golden/g17_teacher_terms.npz by EXECUTING the reference's teacher-gated candidate terms on the CPU (not collected; the
only file of the teacher-term tests that reads the reference tree).  Run:  ``python tests/record_teacher_terms_golden.py``.

  top1_*   ``trainer/active_joint_multi_predignore_top1plbl.py:13-82`` TopOnePlbl at temperature 1.0 (as its trainer builds it), for
           both ``within_filtering`` values, each at ``plbl_th`` 0.0 and at a threshold that rejects roughly half of the multi-hot
           pixels (the median gate value, rounded to three decimals)
  ent_*    ``trainer/active_joint_multi_predignore_multient.py:12-70`` MultiChoiceEnt_ at temperature 0.1

and, for each, the gradient of the weighted objective (16 * loss).  Inputs are recorded by seed (``tests/test_losses_gpu.py:_inputs``
for the student, ``synth.logits`` of a second seed for the teacher) at the shape of g14.  The gate and the arg-max are discrete
decisions, so the recorder asserts in float64 (tests/teacher_terms_restated.py) that, for these seeds, no multi-hot pixel has its gate
value within 1e-5 relative of the threshold and none has its two largest student candidate probabilities within 1e-5 relative: no
pixel has to be left out of any comparison."""
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
import teacher_terms_restated as R  # noqa: E402
from record_partial_label_golden import inputs  # noqa: E402

SEED, SEED_TEACHER, N, C, H, W, S, T_TOP1, T_ENT, WEIGHT = 41, 97, 2, 20, 40, 44, 48, 1.0, 0.1, 16.0


def main():
    refshim.install()
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules['tqdm'] = types.ModuleType('tqdm')
            sys.modules['tqdm'].tqdm = lambda it, **k: it
    from trainer.active_joint_multi_predignore_multient import MultiChoiceEnt_
    from trainer.active_joint_multi_predignore_top1plbl import TopOnePlbl
    z, tgt, spx, msk = inputs(SEED, N, C, H, W, S)
    zteach = synth.logits(SEED_TEACHER, N, C, H, W)
    tt, ts, tm = torch.from_numpy(tgt), torch.from_numpy(spx), torch.from_numpy(msk)
    out = dict(seed=SEED, seed_teacher=SEED_TEACHER, N=N, C=C, H=H, W=W, S=S, temp_top1=T_TOP1, temp_ent=T_ENT, weight=WEIGHT)
    for within in (False, True):
        # the gate values in float64, through a threshold nothing passes
        zs = torch.from_numpy(zteach).double()
        (lt,), y = R._multi_hot_pixels(tgt, spx, msk, zs)
        t = torch.softmax(lt / T_TOP1, dim=1) * y
        g = t.max(dim=1)[0] / (t.sum(dim=1) if within else 1.0)
        half = round(float(g.median()), 3)
        for name, th in (('th0', 0.0), ('half', half)):
            key = 'top1%s_%s' % ('w' if within else '', name)
            _, n, _, margin, gap = R.top1(z, zteach, tgt, spx, msk, T_TOP1, th, within)
            assert margin.min() > 1e-5, (key, margin.min())
            assert gap.min() > 1e-5, (key, gap.min())
            student = torch.from_numpy(z).clone().requires_grad_(True)
            loss = TopOnePlbl(num_class=C, within_filtering=within, filtering_threshold=th, temperature=T_TOP1)(
                student, torch.from_numpy(zteach), tt, ts, tm)
            (gr,) = torch.autograd.grad(WEIGHT * loss, student)
            out[key + '_th'], out[key + '_loss'], out[key + '_n'], out[key + '_grad'] = th, np.float32(float(loss)), n, gr.numpy()
            print(key, 'th', th, 'counted', n, 'of', int(g.shape[0]), 'loss', float(loss), 'margins', margin.min(), gap.min())
    student = torch.from_numpy(z).clone().requires_grad_(True)
    loss = MultiChoiceEnt_(num_class=C, temperature=T_ENT)(student, tt, ts, tm)
    (gr,) = torch.autograd.grad(WEIGHT * loss, student)
    out['ent_loss'], out['ent_grad'] = np.float32(float(loss)), gr.numpy()
    path = os.path.join(ROOT, "tests", "golden", "g17_teacher_terms.npz")
    np.savez_compressed(path, **out)
    print({k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
