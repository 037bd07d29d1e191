"""The partial-label baselines (risk-consistent weighting, top-1 candidate) without a GPU: csrc/partial_label.h through the library's
host loop (``ops.partial_loss_reference``) against
  * oracle/exact.c, bit for bit, for the unchanged merged-positive term ('choice');
  * the float64 restatement (tests/partial_label_restated.py) and the executed reference (tests/golden/g14_partial_label.npz) at the
    tolerance of tests/test_losses_gpu.py: 1e-4 * max(1, |ref|) for loss values, 1e-4 * max|ref| for gradients
    (observed: profiles/partial_label/README.md).
Plus the argument check of the new flag bits and the ``--partial_loss`` option."""
import os

import numpy as np
import pytest
import torch

import partial_label_restated as R
from test_losses_gpu import _inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(2, 20, 19, 301, 9), (2, 21, 33, 37, 150), (2, 19, 40, 44, 48), (1, 7, 24, 36, 16), (1, 32, 24, 36, 16)]
T = 0.1
CE, DECOMP, TCE, RC, TOPONE = 1, 8, 16, 32, 64
MODE_FLAG = {'choice': 0, 'rc': RC, 'topone': TOPONE}
GO = np.array([16.0, 8.0, 0.0], dtype=np.float32)


def _ops():
    from mulactseg_amd import ops
    return ops


_CACHE = {}


def case(shape):
    """inputs of one shape (seeded as tests/test_losses_gpu.py seeds them) and the host reference of every mode, computed once"""
    if shape in _CACHE:
        return _CACHE[shape]
    from oracle import exact
    ops = _ops()
    N, C, H, W, S = shape
    z, tgt, spx, msk = _inputs(300 + W + C, N, C, H, W, S)
    bits = exact.target_bits(tgt)
    c = dict(z=z, tgt=tgt, spx=spx, msk=msk, bits=bits, invT=ops.inv_temperature(T))
    t = (torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(msk), torch.from_numpy(bits.view(np.int32)))
    for mode, f in MODE_FLAG.items():
        losses, acc, dz = ops.partial_loss_reference(*t, c['invT'], CE | DECOMP | f, grad_out=torch.from_numpy(GO))
        c[mode] = (losses.numpy(), acc.numpy().view(np.uint64), dz.numpy())
    _CACHE[shape] = c
    return c


def _report(what, got, ref, bound):
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))))
    print("%s: max error %.3e, bound %.3e" % (what, err, bound))
    return err


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("flags", [CE | DECOMP, CE])
def test_choice_equals_the_frozen_oracle_bit_for_bit(shape, flags):
    from oracle import exact
    ops = _ops()
    c = case(shape)
    eacc, egmax, eloss = exact.partial_loss_fwd(c['z'], c['spx'], c['msk'], c['bits'], np.float32(c['invT']), flags)
    go = np.array([16.0, 8.0, 1.0], dtype=np.float32)
    _, edz = exact.partial_loss_bwd(c['z'], c['spx'], c['msk'], c['bits'], egmax, eacc, go, np.float32(c['invT']), flags)
    losses, acc, dz = ops.partial_loss_reference(torch.from_numpy(c['z']), torch.from_numpy(c['spx']), torch.from_numpy(c['msk']),
                                                 torch.from_numpy(c['bits'].view(np.int32)), c['invT'], flags, grad_out=torch.from_numpy(go))
    assert np.array_equal(acc.numpy().view(np.uint64), eacc)
    assert np.array_equal(losses.numpy(), eloss)
    assert np.array_equal(dz.numpy(), edz)
    assert eacc[3] > 0          # multi-hot pixels are present
    # int32 and 16-bit ids give the same bits
    for dt in (torch.int32, torch.int16):
        l2, a2 = ops.partial_loss_reference(torch.from_numpy(c['z']), torch.from_numpy(c['spx']).to(dt), torch.from_numpy(c['msk']),
                                            torch.from_numpy(c['bits'].view(np.int32)), c['invT'], flags)
        assert torch.equal(a2, acc) and torch.equal(l2, losses)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ['rc', 'topone'])
def test_modes_match_the_float64_restatement(shape, mode):
    c = case(shape)
    losses, _, dz = c[mode]
    ce, mc, grad = R.decomp(mode, c['z'], c['tgt'], c['spx'], c['msk'], T)
    for name, got, ref in (('ce', losses[0], ce), ('mc', losses[1], mc)):
        bound = 1e-4 * max(1.0, abs(ref))
        assert _report("%s %s %s" % (mode, shape, name), got, ref, bound) <= bound
    bound = 1e-4 * float(np.max(np.abs(grad)))
    assert _report("%s %s grad (max|ref| %.3e)" % (mode, shape, np.max(np.abs(grad))), dz, grad, bound) <= bound
    assert losses[2] == 0.0


def _golden():
    g = np.load(os.path.join(GOLDEN, "g14_partial_label.npz"))
    z, tgt, spx, msk = _inputs(int(g['seed']), int(g['N']), int(g['C']), int(g['H']), int(g['W']), int(g['S']))
    return g, z, tgt, spx, msk


def test_modes_match_the_executed_reference():
    """RCMultiChoiceCE (one merged sum, last target column dropped) and OnehotCEMultihotTopone as the reference computed them."""
    from oracle import exact
    ops = _ops()
    g, z, tgt, spx, msk = _golden()
    assert bool(g['topone_recorded'])
    assert str(g['rc_decomp_error']).startswith('IndexError')          # the reference's OnehotCEMultihotRC cannot run as written
    N, S, C = int(g['N']), int(g['S']), int(g['C'])
    invT = ops.inv_temperature(float(g['temp']))
    t = (torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(msk))
    tgt_b = np.concatenate([tgt, np.zeros((N, S, 1), np.uint8)], axis=2)
    bits_b = torch.from_numpy(exact.target_bits(tgt_b, cols_used=C).view(np.int32))
    losses, _, dz = ops.partial_loss_reference(*t, bits_b, invT, CE | RC, grad_out=torch.tensor([16.0, 0.0, 0.0]))
    ref = float(g['rc_loss'])
    assert _report("golden rc loss", float(losses[0]), ref, 1e-4 * max(1.0, abs(ref))) <= 1e-4 * max(1.0, abs(ref))
    assert float(losses[1]) == 0.0
    bound = 1e-4 * float(np.max(np.abs(g['rc_grad'])))
    assert _report("golden rc grad", dz.numpy(), g['rc_grad'], bound) <= bound
    # ... and the restatement of the same class agrees with the reference
    rl, _, rg = R.rc_merged(z, tgt_b, spx, msk, float(g['temp']))
    assert abs(rl - ref) <= 1e-4 * max(1.0, abs(ref)) and np.max(np.abs(rg - g['rc_grad'])) <= bound

    bits = torch.from_numpy(exact.target_bits(tgt).view(np.int32))
    losses, _, dz = ops.partial_loss_reference(*t, bits, invT, CE | DECOMP | TOPONE, grad_out=torch.from_numpy(GO))
    for name, got, key in (('ce', losses[0], 'topone_ce'), ('mc', losses[1], 'topone_mc')):
        ref = float(g[key])
        assert _report("golden topone " + name, float(got), ref, 1e-4 * max(1.0, abs(ref))) <= 1e-4 * max(1.0, abs(ref))
    bound = 1e-4 * float(np.max(np.abs(g['topone_grad'])))
    assert _report("golden topone grad", dz.numpy(), g['topone_grad'], bound) <= bound
    assert R.tie_count(z, tgt, spx, msk, float(g['temp']))[0] == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_no_near_tie_among_the_candidates_of_the_test_inputs(shape):
    """Top-1 is discontinuous in the gradient at ties: the comparisons with float64 above hold because no multi-hot pixel of these
    inputs has its two largest candidate probabilities within 1e-5 relative."""
    c = case(shape)
    ties, multi = R.tie_count(c['z'], c['tgt'], c['spx'], c['msk'], T)
    print("%s: %d of %d multi-hot pixels near a tie" % (shape, ties, multi))
    assert multi > 0 and ties == 0


def test_a_tie_sends_the_gradient_to_the_lower_class_index():
    ops = _ops()
    z = np.zeros((1, 4, 1, 2), dtype=np.float32)
    z[0, :, 0, 0] = [0.3, 1.0, 1.0, -0.5]          # candidates 1 and 2 with equal logits
    z[0, :, 0, 1] = [0.3, 0.2, 1.0, 1.0]           # candidates 2 and 3, equal
    bits = torch.tensor([[0b0110, 0b1100]], dtype=torch.int32)
    spx = torch.tensor([[[0, 1]]], dtype=torch.int64)
    msk = torch.ones((1, 1, 2), dtype=torch.bool)
    losses, acc, dz = ops.partial_loss_reference(torch.from_numpy(z), spx, msk, bits, 1.0, CE | DECOMP | TOPONE,
                                                 grad_out=torch.tensor([1.0, 1.0, 0.0]))
    dz = dz.numpy()[0, :, 0, :]
    assert int(acc[3]) == 2
    for px, m in enumerate([1, 2]):
        p = np.exp(z[0, :, 0, px].astype(np.float64))
        p /= p.sum()
        assert dz[m, px] < 0 and all(dz[k, px] > 0 for k in range(4) if k != m)
        # d_c = a * p_m / (p_m + eps) * (p_c - [c = m]), a = 1 / (1 + 2)
        want = (p - (np.arange(4) == m)) * (p[m] / (p[m] + 1e-8)) / 3.0
        assert np.max(np.abs(dz[:, px] - want)) <= 1e-6
    # the tied candidates carry the same probability bits, so apart from the winner's -k the two gradients are the same value
    assert dz[1, 0] < 0 < dz[2, 0] and dz[2, 1] < 0 < dz[3, 1]


@pytest.mark.parametrize("shape", SHAPES)
def test_only_the_multi_hot_sum_depends_on_the_mode_and_the_values_are_ordered(shape):
    c = case(shape)
    acc0 = c['choice'][1]
    for mode in ('rc', 'topone'):
        acc = c[mode][1]
        diff = np.nonzero(acc != acc0)[0]
        assert list(diff) == [1], (mode, diff)               # ACC_SUM_MC
        assert c[mode][0][0] == c['choice'][0][0]            # ce
    assert c['choice'][0][1] <= c['topone'][0][1] <= c['rc'][0][1]
    assert acc0[1] < c['topone'][1][1] < c['rc'][1][1]
    # the restatement obeys the per-pixel inequality: a maximum is at most the sum, a weighted mean of -log p_c at least -log max p_c
    ch, to, rc = R.per_pixel(c['z'], c['tgt'], c['spx'], c['msk'], T)
    assert ch.size == int(acc0[3]) and np.all(ch <= to) and np.all(to <= rc + 1e-12)


def test_one_hot_pixels_keep_their_bits_in_every_mode():
    """nb == 1: the three modes agree -- the gradient of a one-hot pixel is the same float in all three."""
    c = case(SHAPES[2])
    onehot = (c['tgt'].sum(axis=2) == 1)
    sel = np.zeros_like(c['msk'])
    for n in range(c['msk'].shape[0]):
        ids = np.minimum(c['spx'][n], onehot.shape[1] - 1)
        sel[n] = c['msk'][n] & onehot[n][ids] & (c['spx'][n] < onehot.shape[1])
    assert sel.any()
    sel = np.broadcast_to(sel[:, None], c['choice'][2].shape)
    for mode in ('rc', 'topone'):
        assert np.array_equal(c[mode][2][sel], c['choice'][2][sel])


def test_underflowed_candidates_give_a_finite_result():
    """every candidate far below the winner: p_c saturates at exp(-86) * rinv -- finite loss, finite gradient in both modes"""
    ops = _ops()
    z = np.zeros((1, 4, 1, 1), dtype=np.float32)
    z[0, :, 0, 0] = [200.0, -200.0, -200.0, 0.0]
    for f in (RC, TOPONE):
        losses, _, dz = ops.partial_loss_reference(torch.from_numpy(z), torch.zeros((1, 1, 1), dtype=torch.int64), torch.ones((1, 1, 1), dtype=torch.bool),
                                                   torch.tensor([[0b0110]], dtype=torch.int32), 1.0, CE | DECOMP | f,
                                                   grad_out=torch.tensor([1.0, 1.0, 0.0]))
        assert torch.isfinite(losses).all() and torch.isfinite(dz).all()
        assert abs(float(losses[1]) - 0.5 * -np.log(1e-8)) < 1e-3


@pytest.mark.parametrize("flags", [CE | RC | TOPONE, RC, TOPONE | DECOMP, CE | TCE | RC, CE | TCE | TOPONE])
def test_invalid_flag_combinations_are_refused_before_anything_runs(flags):
    from mulactseg_amd import _lib
    ops = _ops()
    lib = _lib.load()
    c = case(SHAPES[3])
    N, C, H, W, S = SHAPES[3]
    z, spx, msk = torch.from_numpy(c['z']), torch.from_numpy(c['spx']), torch.from_numpy(c['msk']).view(torch.uint8)
    bits = torch.from_numpy(c['bits'].view(np.int32))
    with pytest.raises(_lib.MulActSegHipError, match="out of range"):
        ops.partial_loss_reference(z, spx, msk, bits, c['invT'], flags)
    sentinel = 0x5a5a5a5a
    acc = torch.full((8,), sentinel, dtype=torch.int64)
    work = torch.full((int(lib.mas_partial_loss_work_bytes(N, S, C, flags)) // 8 + 1,), sentinel, dtype=torch.int64)
    dz = torch.full_like(z, 7.0)
    losses = torch.full((3,), 7.0)
    go = torch.ones(3)
    # the argument check answers before any launch, so host pointers are never dereferenced and no device is needed
    args = (z.data_ptr(), spx.data_ptr(), 0, msk.data_ptr(), bits.data_ptr())
    assert lib.mas_partial_loss_reference(*args, N, C, H, W, S, c['invT'], flags, None, acc.data_ptr(), None, None) == -6
    assert lib.mas_partial_loss_fwd(*args, N, C, H, W, S, c['invT'], flags, None, acc.data_ptr(), None) == -6
    assert lib.mas_partial_loss_bwd(*args, None, go.data_ptr(), N, C, H, W, S, c['invT'], flags, dz.data_ptr(), None) == -6
    assert lib.mas_partial_loss_fwd_fused(z.data_ptr(), 0, 0, spx.data_ptr(), 0, msk.data_ptr(), None, 0, 0, bits.data_ptr(), N, C, H, W, S,
                                          c['invT'], flags, None, work.data_ptr(), work.numel() * 8, losses.data_ptr(), None) == -6
    assert lib.mas_partial_loss_bwd_fused(z.data_ptr(), 0, 0, spx.data_ptr(), 0, msk.data_ptr(), bits.data_ptr(), work.data_ptr(),
                                          go.data_ptr(), None, N, C, H, W, S, c['invT'], flags, dz.data_ptr(), None, None) == -6
    assert bool((acc == sentinel).all()) and bool((work == sentinel).all()) and bool((dz == 7.0).all()) and bool((losses == 7.0).all())
    assert lib.mas_error_string(-6).decode() == "argument out of range"


def test_reference_entry_takes_the_ce_family_only():
    from mulactseg_amd import _lib
    ops = _ops()
    c = case(SHAPES[3])
    t = (torch.from_numpy(c['z']), torch.from_numpy(c['spx']), torch.from_numpy(c['msk']), torch.from_numpy(c['bits'].view(np.int32)))
    for flags in (2, CE | 2, CE | TCE, 0):
        with pytest.raises(_lib.MulActSegHipError):
            ops.partial_loss_reference(*t, c['invT'], flags)
    assert (ops.LOSS_RC, ops.LOSS_TOPONE) == (32, 64) == (_lib.LOSS_RC, _lib.LOSS_TOPONE)
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "mulactseg_hip.h")).read()
    assert "#define MAS_LOSS_RC 32" in header and "#define MAS_LOSS_TOPONE 64" in header


def test_partial_loss_option_defaults_and_refusal():
    import importlib
    from mulactseg_amd.utils import common
    for module in ("common", "common_voc"):
        p = importlib.import_module("mulactseg_amd.utils." + module).get_parser()
        assert p.parse_args([]).partial_loss == 'choice'
        assert p.parse_args(['--partial_loss', 'rc']).partial_loss == 'rc'
        with pytest.raises(SystemExit):
            p.parse_args(['--partial_loss', 'entropy'])
    args = common.get_parser().parse_args(['--partial_loss', 'rc', '--nseg', '2048', '--method', 'active'])
    args.trg_datalist, args.region_dict = 'train_seed2048.txt', 'train_seed2048.dict'
    with pytest.raises(NotImplementedError, match="partial_loss"):
        common.arg_assert(args)
    for method in common.PARTIAL_LOSS_METHODS:
        args.method = method
        common.arg_assert(args)
    args.method, args.partial_loss = 'active', 'choice'
    common.arg_assert(args)


def test_modules_and_trainers_carry_the_mode():
    import importlib
    from mulactseg_amd import _lib
    from mulactseg_amd.utils import loss as L
    assert L.RCMultiChoiceCE._flags == CE | RC and L.RCMultiChoiceCE._drop_last
    assert L.OnehotCEMultihotRC._flags == CE | DECOMP | RC and not L.OnehotCEMultihotRC._drop_last
    assert L.OnehotCEMultihotTopone._flags == CE | DECOMP | TOPONE and not L.OnehotCEMultihotTopone._drop_last
    assert L.FusedPartialLabelLoss(16).flags == 1 | 2 | 4 | 8                      # the default is the parent's flag set
    assert L.FusedPartialLabelLoss(16, multi_hot='rc').flags == 1 | 2 | 4 | 8 | RC
    assert L.FusedPartialLabelLoss(16, multi_hot='topone', group=False).flags == CE | DECOMP | TOPONE
    with pytest.raises(ValueError):
        L.FusedPartialLabelLoss(16, multi_hot='entropy')
    assert _lib.load().mas_partial_loss_work_bytes(2, 16, 20, CE | DECOMP | RC) == 64 + 2 * 16 * 4          # no [N,S,C] table
    for name in ('rc', 'topone'):
        mod = importlib.import_module("mulactseg_amd.trainer.active_joint_multi_lossdecomp_" + name)
        assert mod.ActiveTrainer.multi_hot == name and not mod.ActiveTrainer.predicts_ignore
