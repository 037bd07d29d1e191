"""The teacher-weighted group term without a GPU: the `wgroup` section of csrc/teacher_terms.h through the library's host loop
(``ops.wgroup_loss_reference``) against a float64 numpy restatement written here from the formula, against the scans' host loops
without the new bit, and against the executed reference (tests/golden/g18_wgroup.npz) at the tolerance of the partial-label tests --
1e-4 * max(1, |ref|) for loss values, 1e-4 * max|ref| for gradients, counted entries exactly -- plus the flag rules, the parser flag
and the trainer module."""
import os

import numpy as np
import pytest
import torch

from test_losses_gpu import _inputs
from test_partial_label_cpu import SHAPES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CE, GROUP, ONLY_MULTI, DECOMP, TOP1, WGROUP = 1, 2, 4, 8, 128, 1024
T = 0.1
EPS = 1e-8
ERR_RANGE = -6                  # MAS_ERR_RANGE (csrc/common.h), "argument out of range"
BASE = ['-m', 'deeplabv3pluswn_resnet50deepstem', '--nseg', '64', '-p', '/tmp/x']


def _ops():
    from mulactseg_amd import ops
    return ops


def _bits(tgt):
    from oracle import exact
    return torch.from_numpy(exact.target_bits(np.ascontiguousarray(tgt)).view(np.int32))


def restated(z, zt, tgt, spx, msk, temp, only_multi):
    """The term in float64, from the formula: over the selected pixels of every superpixel s with a non-empty target row (more than
    one bit with ``only_multi``) and every class c of the row, P = max softmax(z / T)_c, Wt = max softmax(z_teacher / T)_c;
    loss = sum Wt * -log(P + eps) / (1 + n) over the n entries with P > 0.  Returns (loss, n, the smallest relative gap between the
    two largest student probabilities of a counted entry, (min Wt, max Wt))."""
    N, C, H, W = z.shape
    S = tgt.shape[1]

    def softmax(x):
        x = x.astype(np.float64) / temp
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    p, t = softmax(z), softmax(zt)
    total, n, gaps, ws = 0.0, 0, [np.inf], []
    for i in range(N):
        sel = np.asarray(msk[i]).astype(bool).reshape(-1)
        ids = np.asarray(spx[i]).reshape(-1)[sel]
        pi, ti = p[i].reshape(C, -1).T[sel], t[i].reshape(C, -1).T[sel]
        for s in np.unique(ids):
            if s < 0 or s >= S:
                continue
            y = tgt[i, s]
            if int(y.sum()) <= (1 if only_multi else 0):
                continue
            rows = ids == s
            for c in np.nonzero(y)[0]:
                col = np.sort(pi[rows, c])
                if col[-1] > 0:
                    w = ti[rows, c].max()
                    total += w * -np.log(col[-1] + EPS)
                    n += 1
                    ws.append(w)
                    if col.shape[0] > 1:
                        gaps.append((col[-1] - col[-2]) / col[-1])
    return total / (1 + n), n, min(gaps), ((min(ws), max(ws)) if ws else (0.0, 0.0))


def _ref(z, zt, tgt, spx, msk, flags, temp=T, go=(0.0, 0.0, 1.0)):
    ops = _ops()
    return ops.wgroup_loss_reference(torch.from_numpy(z), torch.from_numpy(zt), torch.from_numpy(spx), torch.from_numpy(msk), _bits(tgt),
                                     ops.inv_temperature(temp), flags, grad_out=torch.tensor(go, dtype=torch.float32))


def _case(shape):
    from mulactseg_amd import synth
    N, C, H, W, S = shape
    z, tgt, spx, msk = _inputs(300 + W + C, N, C, H, W, S)
    return z, synth.logits(500 + W + C, N, C, H, W), tgt, spx, msk


def _golden():
    from mulactseg_amd import synth
    g = np.load(os.path.join(GOLDEN, "g18_wgroup.npz"))
    N, C, H, W, S = (int(g[k]) for k in 'NCHWS')
    z, tgt, spx, msk = _inputs(int(g['seed']), N, C, H, W, S)
    return g, z, synth.logits(int(g['seed_teacher']), N, C, H, W), tgt, spx, msk


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("only_multi", [False, True])
def test_the_host_loop_matches_the_float64_restatement(shape, only_multi):
    z, zt, tgt, spx, msk = _case(shape)
    rl, rn, _, _ = restated(z, zt, tgt, spx, msk, T, only_multi)
    losses, acc, gmax, tmax, _ = _ref(z, zt, tgt, spx, msk, GROUP | WGROUP | (ONLY_MULTI if only_multi else 0))
    err = abs(float(losses[2]) - rl)
    print("wgroup %s only_multi %s: loss %.7g, restated %.7g, n %d, error %.3e, bound %.3e" % (shape, only_multi, float(losses[2]), rl, rn, err,
                                                                                             1e-5 * abs(rl)))
    assert int(acc[6]) == rn > 0
    assert err <= 1e-5 * abs(rl)
    assert float(losses[0]) == 0.0 and float(losses[1]) == 0.0


@pytest.mark.parametrize("shape", SHAPES)
def test_a_teacher_equal_to_the_student_gives_the_students_table(shape):
    z, _, tgt, spx, msk = _case(shape)
    _, _, gmax, tmax, _ = _ref(z, z.copy(), tgt, spx, msk, GROUP | WGROUP)
    assert bool((gmax != 0).any())
    assert torch.equal(tmax, (gmax >> 32).to(torch.int32))
    assert bool((tmax[gmax == 0] == 0).all())


@pytest.mark.parametrize("company", [CE | GROUP, CE | DECOMP | GROUP, CE | DECOMP | GROUP | ONLY_MULTI])
def test_the_co_resident_terms_are_those_of_the_scans_without_the_bit(company):
    """ce / mc sums, the student's table and n_group == ops.teacher_loss_reference (and ops.partial_loss_reference) without the new bit"""
    ops = _ops()
    z, zt, tgt, spx, msk = _case(SHAPES[2])
    losses, acc, gmax, tmax, dz = _ref(z, zt, tgt, spx, msk, company | WGROUP, go=(16.0, 8.0, 0.0))
    t = (torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(msk), _bits(tgt))
    tl, tacc, tgmax = ops.teacher_loss_reference(t[0], torch.from_numpy(zt), *t[1:], ops.inv_temperature(T), 1.0, 0.0, company | TOP1)
    assert torch.equal(acc[:5], tacc[:5]) and int(acc[6]) == int(tacc[6]) > 0 and torch.equal(gmax, tgmax)
    assert torch.equal(losses[:2], tl[:2])
    assert int(acc[5]) != int(tacc[5])                      # the group sum is the weighted one
    bl, bacc, bdz = ops.partial_loss_reference(*t, ops.inv_temperature(T), company & (CE | DECOMP), grad_out=torch.tensor([16.0, 8.0, 0.0]))
    assert torch.equal(acc[:5], bacc[:5]) and torch.equal(losses[:2], bl[:2])
    assert torch.equal(dz, bdz)                             # a zero upstream gradient of the group term adds exact zeros


@pytest.mark.parametrize("only_single", [False, True])
def test_the_host_loop_matches_the_executed_reference(only_single):
    g, z, zt, tgt, spx, msk = _golden()
    key, w = 'single' if only_single else 'all', float(g['weight'])
    rl, rn, gap, (wlo, whi) = restated(z, zt, tgt, spx, msk, float(g['temp']), only_single)
    assert gap > 1e-5                                       # no arg-pixel decision is near its edge: nothing is left out
    losses, acc, _, _, dz = _ref(z, zt, tgt, spx, msk, GROUP | WGROUP | (ONLY_MULTI if only_single else 0), float(g['temp']), go=(0.0, 0.0, w))
    ref, gref = float(g[key + '_loss']), g[key + '_grad']
    print("g18 %s: n %d (golden %d, restated %d), loss %.7g golden %.7g restated %.7g, gap %.3e, weights %.4g..%.4g"
          % (key, int(acc[6]), int(g[key + '_n']), rn, float(losses[2]), ref, rl, gap, wlo, whi))
    assert int(acc[6]) == int(g[key + '_n']) == rn > 0
    assert abs(float(losses[2]) - ref) <= 1e-4 * max(1.0, abs(ref))
    err, scale = float(np.max(np.abs(dz.numpy() - gref))), float(np.max(np.abs(gref)))
    print("g18 %s gradient: max error %.3e of max|ref| %.3e" % (key, err, scale))
    assert scale > 0 and err <= 1e-4 * scale


def test_the_two_counts_of_the_golden_differ():
    g = np.load(os.path.join(GOLDEN, "g18_wgroup.npz"))
    assert int(g['single_n']) < int(g['all_n'])


def test_the_flag_needs_the_group_term_and_a_teacher():
    from mulactseg_amd import _lib
    ops = _ops()
    lib = _lib.load()
    z, zt, tgt, spx, msk = _case(SHAPES[3])
    N, C, H, W = z.shape
    S = tgt.shape[1]
    zc, tc, sc, mc, bits = torch.from_numpy(z), torch.from_numpy(zt), torch.from_numpy(spx), torch.from_numpy(msk).view(torch.uint8), _bits(tgt)
    acc, gmax, tmax = torch.zeros(8, dtype=torch.int64), torch.zeros((N, S, C), dtype=torch.int64), torch.zeros((N, S, C), dtype=torch.int32)

    def call(teacher, flags):
        return lib.mas_wgroup_loss_reference(zc.data_ptr(), teacher, sc.data_ptr(), 0, mc.data_ptr(), bits.data_ptr(), N, C, H, W, S,
                                             ops.inv_temperature(T), flags, None, acc.data_ptr(), gmax.data_ptr(), tmax.data_ptr(), None, None)

    assert call(tc.data_ptr(), GROUP | WGROUP) == 0
    assert call(tc.data_ptr(), WGROUP) == ERR_RANGE
    assert call(tc.data_ptr(), CE | WGROUP) == ERR_RANGE
    assert call(None, GROUP | WGROUP) == ERR_RANGE
    assert call(tc.data_ptr(), GROUP | WGROUP | TOP1) == ERR_RANGE
    assert call(tc.data_ptr(), GROUP) == ERR_RANGE             # (the entry point is for the new bit)
    # the earlier host loops refuse the bit, as they refuse unknown ones
    with pytest.raises(_lib.MulActSegHipError):
        ops.teacher_loss_reference(zc, tc, sc, mc, bits, ops.inv_temperature(T), 1.0, 0.0, GROUP | TOP1 | WGROUP)
    with pytest.raises(_lib.MulActSegHipError):
        ops.partial_loss_reference(zc, sc, mc, bits, ops.inv_temperature(T), CE | WGROUP)


def test_group_only_single_belongs_to_the_wgroup_trainer():
    from mulactseg_amd.utils import common
    p = common.get_parser()
    assert p.parse_args(BASE).group_only_single is False

    def check(method, extra):
        a = p.parse_args(BASE + ['--method', method] + extra)
        a.init_checkpoint, a.trg_datalist, a.region_dict = 'x', 'train_seed64.txt', 'train_seed64.dict'
        common.arg_assert(a)
        return a

    assert check('active_joint_multi_predignore_wgroup', ['--group_only_single']).group_only_single is True
    check('active_joint_multi_predignore_wgroup', [])
    for method in ('active_joint_multi_predignore', 'active_joint_multi_predignore_top1plbl', 'active_joint_multi_predignore_multient',
                   'active_joint_multi_predignore_lossdecomp'):
        check(method, [])
        with pytest.raises(NotImplementedError, match="group_only_single"):
            check(method, ['--group_only_single'])


def test_the_trainer_imports_and_builds_its_criterion():
    import types
    from mulactseg_amd.trainer import active_joint_multi_predignore_wgroup as mod
    from mulactseg_amd.utils import loss as L
    assert "frozen BatchNorm stays frozen" in mod.__doc__
    for single in (False, True):
        tr = types.SimpleNamespace(args=types.SimpleNamespace(nseg=64, group_ce_temp=0.1, multi_ce_temp=0.1, group_only_single=single),
                                   num_classes=19)
        mod.ActiveTrainer.get_criterion(tr)
        assert isinstance(tr.group_multi_loss, L.WeightedGroupMultiLabelCE) and tr.group_multi_loss.ignore_only_single is single
        assert isinstance(tr.multi_pos_loss, L.MultiChoiceCE_) and isinstance(tr.fused_loss, L.FusedWGroupLoss)
        assert bool(tr.fused_loss.flags & ONLY_MULTI) is single and tr.fused_loss.flags & WGROUP and tr.fused_loss.flags & CE
        assert bool(tr.group_multi_loss._f() & ONLY_MULTI) is single
    assert L.WeightedGroupMultiLabelCE(None, 19, 64, 0.1).ignore_only_single is False
