"""The partial-label baselines on the GPU: the PLX instantiations of the loss scans (csrc/losses.hip) against the library's host loop
through csrc/partial_label.h (``ops.partial_loss_reference``) bit for bit -- full resolution and quarter resolution, vector and scalar
path, the three id types -- the unchanged default against oracle/exact.c, the modules against the executed reference
(tests/golden/g14_partial_label.npz) and the float64 restatement, and the trainers end to end."""
import logging
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from mulactseg_amd import synth

import partial_label_restated as R
from test_losses_gpu import _inputs
from test_partial_label_cpu import CE, DECOMP, RC, TOPONE, SHAPES, T, case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = {'rc': RC, 'topone': TOPONE}
GO3 = np.array([16.0, 8.0, 1.0], dtype=np.float32)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _against_reference(ops, z, spx, msk, bits, invT, id_types=(torch.int64, torch.int32, torch.int16)):
    """acc, loss values and dz of the kernels == the host loop, for both modes, with and without DECOMP, for every id type"""
    zc, sc, mc, bc = torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(msk), torch.from_numpy(bits.view(np.int32))
    zt, mt, bt, got = zc.cuda(), mc.cuda(), bc.cuda(), torch.from_numpy(GO3).cuda()
    for mode, f in MODES.items():
        for decomp in (DECOMP, 0):
            flags = CE | decomp | f
            rl, racc, rdz = ops.partial_loss_reference(zc, sc, mc, bc, invT, flags, grad_out=torch.from_numpy(GO3))
            assert int(racc[3]) > 0
            for dt in id_types:
                st = sc.to(dt).cuda()
                losses, acc, gmax = ops.partial_loss_fwd(zt, st, mt, bt, invT, flags)
                assert gmax is None
                assert torch.equal(acc.cpu(), racc), (mode, decomp, dt)
                assert torch.equal(losses.cpu().view(torch.int32), rl.view(torch.int32)), (mode, decomp, dt)
                dz = ops.partial_loss_bwd(zt, st, mt, bt, None, acc, got, invT, flags)
                assert torch.equal(dz.cpu().view(torch.int32), rdz.view(torch.int32)), (mode, decomp, dt)


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_host_reference_bit_for_bit(shape):
    ops = _gpu()
    c = case(shape)
    _against_reference(ops, c['z'], c['spx'], c['msk'], c['bits'], c['invT'])


def test_bit_31_of_the_target_mask():
    """C = 32 with class 31 a candidate of every superpixel (the seeded targets of that shape never draw it)"""
    ops = _gpu()
    from oracle import exact
    c = case(SHAPES[4])
    tgt = c['tgt'].copy()
    tgt[:, :, 31] = 1
    bits = exact.target_bits(tgt)
    assert np.all(bits >> 31 == 1)
    _against_reference(ops, c['z'], c['spx'], c['msk'], bits, c['invT'], id_types=(torch.int64,))


@pytest.mark.parametrize("fname,flags", [('production', 1 | 2 | 4 | 8), ('decomp', 1 | 8), ('mc_predignore', 1), ('onlymulti', 2 | 4)])
def test_flag_sets_without_a_new_bit_keep_the_oracle_bits(fname, flags):
    ops = _gpu()
    from oracle import exact
    c = case(SHAPES[2])
    N, C, H, W, S = SHAPES[2]
    eacc, egmax, eloss = exact.partial_loss_fwd(c['z'], c['spx'], c['msk'], c['bits'], np.float32(c['invT']), flags)
    _, edz = exact.partial_loss_bwd(c['z'], c['spx'], c['msk'], c['bits'], egmax, eacc, GO3, np.float32(c['invT']), flags)
    zt, st, mt = torch.from_numpy(c['z']).cuda(), torch.from_numpy(c['spx']).cuda(), torch.from_numpy(c['msk']).cuda()
    bt = torch.from_numpy(c['bits'].view(np.int32)).cuda()
    losses, acc, gmax = ops.partial_loss_fwd(zt, st, mt, bt, c['invT'], flags)
    assert np.array_equal(acc.cpu().numpy().view(np.uint64), eacc)
    if gmax is not None:
        assert np.array_equal(gmax.cpu().numpy().view(np.uint64), egmax)
    assert np.array_equal(losses.cpu().numpy(), eloss)
    dz = ops.partial_loss_bwd(zt, st, mt, bt, gmax, acc, torch.from_numpy(GO3).cuda(), c['invT'], flags)
    assert np.array_equal(dz.cpu().numpy(), edz)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_group_term_is_untouched_by_the_mode(mode):
    """production flags + a mode: ce and mc are the reference's, the group value, its table and its gradient are the default's"""
    ops = _gpu()
    c = case(SHAPES[2])
    zt, st, mt = torch.from_numpy(c['z']).cuda(), torch.from_numpy(c['spx']).cuda(), torch.from_numpy(c['msk']).cuda()
    bt = torch.from_numpy(c['bits'].view(np.int32)).cuda()
    base = 1 | 2 | 4 | 8
    l0, a0, g0 = ops.partial_loss_fwd(zt, st, mt, bt, c['invT'], base)
    l1, a1, g1 = ops.partial_loss_fwd(zt, st, mt, bt, c['invT'], base | MODES[mode])
    assert torch.equal(g0, g1) and float(l0[2]) == float(l1[2]) and float(l0[0]) == float(l1[0])
    assert float(l1[1]) == float(c[mode][0][1]) and np.array_equal(a1.cpu().numpy().view(np.uint64)[:5], c[mode][1][:5])
    only_group = torch.tensor([0.0, 0.0, 1.0], device='cuda')
    d0 = ops.partial_loss_bwd(zt, st, mt, bt, g0, a0, only_group, c['invT'], base)
    d1 = ops.partial_loss_bwd(zt, st, mt, bt, g1, a1, only_group, c['invT'], base | MODES[mode])
    assert torch.equal(d0, d1) and float(d0.abs().max()) > 0
    # the full gradient is the CE-family gradient (the host loop's) plus the group gradient, to rounding
    go = torch.from_numpy(GO3).cuda()
    d = ops.partial_loss_bwd(zt, st, mt, bt, g1, a1, go, c['invT'], base | MODES[mode])
    want = torch.from_numpy(c[mode][2]).cuda() + d1
    assert float((d - want).abs().max()) <= 1e-6 * float(want.abs().max())


LOW = [(2, 20, 13, 11, 52, 44, 48), (2, 21, 9, 10, 33, 37, 150), (2, 19, 16, 48, 64, 192, 128)]


@pytest.mark.parametrize("N,C,h,w,H,W,S", LOW)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_lowres_scans_equal_the_materialised_path(N, C, h, w, H, W, S, mode):
    ops = _gpu()
    from mulactseg_amd import _lib
    _, tgt, spx, msk = _inputs(900 + W + C, N, C, H, W, S)
    zq = torch.from_numpy(synth.logits(77 + h, N, C, h, w)).cuda()
    invT = ops.inv_temperature(T)
    st, mt = torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda()
    bits = ops.target_bits(torch.from_numpy(tgt).cuda())
    zfull = ops.upsample_bilinear(zq, (H, W))
    got = torch.from_numpy(GO3).cuda()
    for flags in (CE | DECOMP | MODES[mode], CE | MODES[mode], 1 | 2 | 4 | 8 | MODES[mode]):
        l_full, a_full, g_full = ops.partial_loss_fwd(zfull, st, mt, bits, invT, flags)
        l_low, a_low, g_low = ops.partial_loss_fwd_lowres(zq, (H, W), st, mt, bits, invT, flags)
        assert int(a_full[3]) > 0
        assert torch.equal(a_low, a_full) and torch.equal(l_low.view(torch.int32), l_full.view(torch.int32))
        if g_full is not None:
            assert torch.equal(g_low, g_full)
        dzq = ops.partial_loss_bwd_lowres(zq, (H, W), st, mt, bits, g_low, a_low, got, invT, flags)
        dz = ops.partial_loss_bwd(zfull, st, mt, bits, g_full, a_full, got, invT, flags)
        ref = torch.empty_like(zq)
        _lib.check(_lib.load().mas_upsample_bilinear_bwd(dz.data_ptr(), N * C, h, w, H, W, ref.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "mas_upsample_bilinear_bwd")
        scale = float(ref.abs().max())
        err = float((dzq - ref).abs().max())
        print("lowres %s flags %d: max error %.3e of max|ref| %.3e" % (mode, flags, err, scale))
        assert scale > 0 and err <= 2e-6 * scale
        assert torch.equal(dzq, ops.partial_loss_bwd_lowres(zq, (H, W), st, mt, bits, g_low, a_low, got, invT, flags))
    # the id types take the same path at low resolution
    for dt in (torch.int32, torch.int16):
        _, a2, _ = ops.partial_loss_fwd_lowres(zq, (H, W), st.to(dt), mt, bits, invT, flags)
        assert torch.equal(a2, a_low)
        assert torch.equal(dzq, ops.partial_loss_bwd_lowres(zq, (H, W), st.to(dt), mt, bits, g_low, a_low, got, invT, flags))


def _close(got, ref, tol=1e-4):
    return abs(float(got) - float(ref)) <= tol * max(1.0, abs(float(ref)))


def test_modules_match_the_executed_reference_and_the_restatement():
    _gpu()
    from mulactseg_amd.utils import loss as L
    g = np.load(os.path.join(GOLDEN, "g14_partial_label.npz"))
    N, C, H, W, S, temp = int(g['N']), int(g['C']), int(g['H']), int(g['W']), int(g['S']), float(g['temp'])
    z, tgt, spx, msk = _inputs(int(g['seed']), N, C, H, W, S)
    tt, ts, tm = torch.from_numpy(tgt).cuda(), torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda()
    tb = torch.from_numpy(np.concatenate([tgt, np.zeros((N, S, 1), np.uint8)], axis=2)).cuda()

    def grad_close(zt, ref):
        err = float(np.max(np.abs(zt.grad.cpu().numpy() - ref)))
        print("module gradient: max error %.3e of max|ref| %.3e" % (err, np.max(np.abs(ref))))
        return err <= 1e-4 * float(np.max(np.abs(ref)))

    zt = torch.from_numpy(z).cuda().requires_grad_(True)
    loss = L.RCMultiChoiceCE(num_class=C, temperature=temp)(zt, tb, ts, tm)
    (16.0 * loss).backward()
    assert _close(loss, g['rc_loss']) and grad_close(zt, g['rc_grad'])

    zt = torch.from_numpy(z).cuda().requires_grad_(True)
    ce, mc = L.OnehotCEMultihotTopone(num_class=C, temperature=temp)(zt, tt, ts, tm)
    (16.0 * ce + 8.0 * mc).backward()
    assert _close(ce, g['topone_ce']) and _close(mc, g['topone_mc']) and grad_close(zt, g['topone_grad'])

    # the reference's OnehotCEMultihotRC raises (recorded); the class here against the float64 restatement of what it means
    assert str(g['rc_decomp_error']).startswith('IndexError')
    rce, rmc, rgrad = R.decomp('rc', z, tgt, spx, msk, temp)
    zt = torch.from_numpy(z).cuda().requires_grad_(True)
    ce, mc = L.OnehotCEMultihotRC(num_class=C, temperature=temp)(zt, tt, ts, tm)
    (16.0 * ce + 8.0 * mc).backward()
    assert _close(ce, rce) and _close(mc, rmc) and grad_close(zt, rgrad)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("group", [True, False])
def test_fused_module_carries_the_mode(mode, group):
    """weighted_lowres == the torch composition of forward_lowres bit for bit (value and gradient); forward == forward_lowres of the
    materialised logits in value; group=False allocates no [N,S,C] table and reports a zero group value"""
    ops = _gpu()
    from mulactseg_amd.utils.loss import FusedPartialLabelLoss
    N, C, h, w, S = 2, 20, 12, 20, 64
    H, W = 4 * h, 4 * w
    _, tgt, spx, msk = _inputs(43, N, C, H, W, S)
    crit = FusedPartialLabelLoss(S, T, T, sync_normalisers=False, multi_hot=mode, group=group)
    tg, sp, mk = torch.from_numpy(tgt).cuda(), torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda()
    z1 = torch.from_numpy(synth.logits(6, N, C, h, w)).cuda().requires_grad_(True)
    z2 = z1.detach().clone().requires_grad_(True)
    w_gm = 1.0 if group else 0.0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    total, g1, c1, m1 = crit.weighted_lowres(z1, (H, W), tg, sp, mk, 16.0, 8.0, w_gm)
    total.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    g2, c2, m2 = crit.forward_lowres(z2, (H, W), tg, sp, mk)
    ref = (16.0 * c2) + (8.0 * m2) + (w_gm * g2)
    ref.backward()
    assert float(total) == float(ref) and float(g1) == float(g2) and float(c1) == float(c2) and float(m1) == float(m2)
    assert torch.equal(z1.grad, z2.grad) and float(z1.grad.abs().max()) > 0 and float(m1) > 0
    g3, c3, m3 = crit(ops.upsample_bilinear(z1.detach(), (H, W)), tg, sp, mk)
    assert float(g3) == float(g1) and float(c3) == float(c1) and float(m3) == float(m1)
    plain = FusedPartialLabelLoss(S, T, T, sync_normalisers=False, group=group).forward_lowres(z1.detach(), (H, W), tg, sp, mk)
    assert float(plain[1]) == float(c1) and float(plain[0]) == float(g1) and float(plain[2]) < float(m1)       # choice < the mode
    if group:
        assert float(g1) > 0
    else:
        assert float(g1) == 0.0
        assert int(_lib_work_bytes(N, S, C, crit.flags)) == 64 + N * S * 4          # accumulators + bit masks: no [N,S,C] table
        print("peak allocation of a group=False step: %d bytes; one [N,C,H,W] f32 tensor: %d bytes" % (peak, N * C * H * W * 4))
        assert peak < N * C * H * W * 4                                             # no [N,C,H,W] tensor in either direction


def _lib_work_bytes(N, S, C, flags):
    from mulactseg_amd import _lib
    return _lib.load().mas_partial_loss_work_bytes(N, S, C, flags)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_empty_mask_gives_zero_loss_and_zero_gradient(mode):
    _gpu()
    from mulactseg_amd.utils import loss as L
    N, C, H, W, S = 2, 20, 24, 36, 16
    z, tgt, spx, msk = _inputs(11, N, C, H, W, S)
    tt, ts = torch.from_numpy(tgt).cuda(), torch.from_numpy(spx).cuda()
    tm = torch.zeros((N, H, W), dtype=torch.bool, device='cuda')
    cls = {'rc': L.OnehotCEMultihotRC, 'topone': L.OnehotCEMultihotTopone}[mode]
    zt = torch.from_numpy(z).cuda().requires_grad_(True)
    ce, mc = cls(num_class=C, temperature=T)(zt, tt, ts, tm)
    (ce + mc).backward()
    assert float(ce) == 0.0 and float(mc) == 0.0 and float(zt.grad.abs().max()) == 0.0
    crit = L.FusedPartialLabelLoss(S, T, T, sync_normalisers=False, multi_hot=mode, group=False)
    zq = torch.from_numpy(synth.logits(3, N, C, H // 4, W // 4)).cuda().requires_grad_(True)
    total, _, _, _ = crit.weighted_lowres(zq, (H, W), tt, ts, tm, 16.0, 8.0, 0.0)
    total.backward()
    assert float(total) == 0.0 and float(zq.grad.abs().max()) == 0.0


# ---- trainers ---------------------------------------------------------------------------------------------------------------------
N_CLS, TS, TH, TW = 19, 64, 128, 160


class _Train(torch.utils.data.Dataset):
    def __init__(self, cols):
        self.cols = cols
        self.selection_iter = 1

    def __len__(self):
        return 2

    def __getitem__(self, i):
        rs = np.random.RandomState(100 + i)
        spx, msk = synth.train_crop(200 + i, TH, TW, TS, frac_selected=0.3)
        return {'images': torch.from_numpy(rs.standard_normal((3, TH, TW)).astype(np.float32)),
                'labels': torch.from_numpy(synth.multi_hot_targets(300 + i, TS, self.cols)),
                'spx': torch.from_numpy(spx), 'spmask': torch.from_numpy(msk)}


class _Val(torch.utils.data.Dataset):
    def __len__(self):
        return 1

    def __getitem__(self, i):
        return {'images': torch.zeros((3, TH, TW)), 'labels': torch.zeros((TH, TW), dtype=torch.int64)}


@pytest.mark.parametrize("method,extra,cols,module", [
    ('active_joint_multi_lossdecomp_rc', [], N_CLS, 'OnehotCEMultihotRC'),
    ('active_joint_multi_predignore_lossdecomp', ['--partial_loss', 'topone'], N_CLS + 1, 'OnehotCEMultihotTopone'),
    ('active_joint_multi_lossdecomp_topone', [], N_CLS, 'OnehotCEMultihotTopone'),
    ('active_joint_multi_lossdecomp', ['--partial_loss', 'rc'], N_CLS, 'OnehotCEMultihotRC')])
def test_trainers_run_the_quarter_resolution_step(method, extra, cols, module):
    _gpu()
    import importlib
    from mulactseg_amd import dataloader, ops
    from mulactseg_amd.utils import common, loss as L
    tmp = tempfile.mkdtemp()
    a = common.get_parser().parse_args([
        '-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--method', method, '--ce_temp', '0.1', '--multi_ce_temp', '0.1',
        '--group_ce_temp', '0.1', '--coeff', '16.0', '--coeff_mc', '8.0', '--coeff_gm', '1.0', '--or_labeling', '--fair_counting',
        '--nseg', str(TS), '--train_batch_size', '2', '--val_batch_size', '1', '--num_workers', '0', '--val_num_workers', '0',
        '--train_lr', '2e-5', '--finetune_itrs', '3', '--val_period', '1000', '--log_period', '1', '-p', tmp] + extra)
    a.pretrained_backbone = False
    dataloader.register_dataset_factory(lambda args, name, data_root, datalist, imageset: _Val())
    torch.manual_seed(0)
    tr = importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer(a, logging.getLogger("test"), 1)
    seen = dict(lowres=[], batch=[], meters=[], logged=[])
    fwd, batch, meter = tr.forward_train, tr._batch, tr.update_average_meter

    def forward_train(images, **kw):
        out = fwd(images, **kw)
        seen['lowres'].append((kw.get('lowres', False), out.detach().clone()))
        return out

    def _batch():
        b = batch()
        seen['batch'].append(b)
        return b

    def update_average_meter(values):
        seen['meters'].append({k: v.detach().clone() for k, v in values.items()})
        return meter(values)

    tr.forward_train, tr._batch, tr.update_average_meter = forward_train, _batch, update_average_meter
    tr._wandb_log = lambda payload, step: seen['logged'].append(dict(payload))
    before = [p.detach().clone() for p in tr.net.parameters()]
    tr.train(types.SimpleNamespace(selection_iter=1, get_trainset=lambda: _Train(cols)))
    assert len(seen['lowres']) == 3 and all(low for low, _ in seen['lowres'])
    zq = seen['lowres'][0][1]
    assert tuple(zq.shape) == (2, cols, TH // 4, TW // 4)                       # no full-resolution logits left the model
    names = {'train-loss', 'ce-loss', 'pos-loss'} | ({'group-loss'} if extra else set())       # (--partial_loss keeps the group term)
    for m in seen['meters']:
        assert set(m) == names and all(bool(torch.isfinite(v)) for v in m.values())
    assert names <= set().union(*[set(p) for p in seen['logged']])
    moved = sum(float((p.detach() - q).abs().sum()) for p, q in zip(tr.net.parameters(), before))
    assert moved > 0 and np.isfinite(moved)
    # the first step's (ce, mc): the drop-in module on the materialised logits of the same forward
    images, labels, spx, msk = seen['batch'][0]
    ce, mc = getattr(L, module)(num_class=N_CLS, temperature=0.1)(ops.upsample_bilinear(zq, (TH, TW)), labels, spx, msk)
    first = seen['meters'][0]
    assert float(first['ce-loss']) == float(ce) and float(first['pos-loss']) == float(mc) and float(mc) > 0
    assert isinstance(tr.multi_pos_loss, getattr(L, module))
    want = 16.0 * float(ce) + 8.0 * float(mc) + (float(first['group-loss']) if 'group-loss' in first else 0.0)
    assert abs(float(first['train-loss']) - want) <= 1e-5 * abs(want)
