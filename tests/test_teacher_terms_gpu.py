"""The teacher-gated candidate terms on the GPU: the TT instantiations of the loss scans (csrc/losses.hip) against the library's host
loop through csrc/teacher_terms.h (``ops.teacher_loss_reference``) bit for bit -- vector and scalar path, the three id types, both
gates, with and without the co-resident pos / group terms --, the quarter-resolution scans against the materialised upsample, the
co-resident terms against the scans without the new slot, the modules against the executed reference
(tests/golden/g17_teacher_terms.npz), and the two trainers end to end."""
import logging
import os
import tempfile
import types

import numpy as np
import pytest
import torch

from mulactseg_amd import synth

from test_losses_gpu import _inputs
from test_partial_label_cpu import SHAPES
from test_partial_label_gpu import LOW, N_CLS, TH, TS, TW, _Train, _Val
from test_teacher_terms_cpu import CE, DECOMP, ENT, GROUP, ONLY_MULTI, T, TOP1, WITHIN, _bits, _golden

pytestmark = pytest.mark.gpu
GO4 = np.array([16.0, 8.0, 1.0, 4.0], dtype=np.float32)
TERMS = {'top1': (TOP1, 1.0, 0.0), 'top1_within': (TOP1 | WITHIN, 1.0, 0.5), 'ent': (ENT, T, 0.0)}      # flags, temperature, plbl_th
COMPANY = (0, CE | GROUP, CE | DECOMP | GROUP | ONLY_MULTI)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _case(shape, force_bit31=False):
    N, C, H, W, S = shape
    z, tgt, spx, msk = _inputs(300 + W + C, N, C, H, W, S)
    if force_bit31:
        tgt = tgt.copy()
        tgt[:, :, 31] = 1
    return z, synth.logits(500 + W + C, N, C, H, W), tgt, spx, msk


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("term", sorted(TERMS))
def test_kernels_equal_the_host_reference_bit_for_bit(shape, term):
    ops = _gpu()
    z, zt, tgt, spx, msk = _case(shape, force_bit31=shape[1] == 32)
    f, temp, th = TERMS[term]
    invT, invT_x = ops.inv_temperature(T), ops.inv_temperature(temp)
    bits = _bits(tgt)
    if shape[1] == 32:
        assert bool((bits.view(torch.int32) < 0).all())                      # bit 31 in every candidate set
    zc, tc, sc, mc = torch.from_numpy(z), (torch.from_numpy(zt) if f & TOP1 else None), torch.from_numpy(spx), torch.from_numpy(msk)
    zg, tg, mg, bg, gog = zc.cuda(), (None if tc is None else tc.cuda()), mc.cuda(), bits.cuda(), torch.from_numpy(GO4).cuda()
    for company in COMPANY:
        flags = f | company
        rl, racc, rgmax, rdz = ops.teacher_loss_reference(zc, tc, sc, mc, bits, invT, invT_x, th, flags, grad_out=torch.from_numpy(GO4))
        assert int(racc[9]) > 0
        for dt in (torch.int64, torch.int32, torch.int16):
            sg = sc.to(dt).cuda()
            losses, acc, gmax = ops.teacher_loss_fwd(zg, tg, None, sg, mg, bg, invT, invT_x, th, flags)
            assert torch.equal(acc.cpu(), racc), (term, company, dt)
            assert (gmax is None) == (rgmax is None) and (gmax is None or torch.equal(gmax.cpu(), rgmax))
            assert torch.equal(losses.cpu().view(torch.int32), rl.view(torch.int32)), (term, company, dt)
            dz = ops.teacher_loss_bwd(zg, tg, None, sg, mg, bg, gmax, acc, gog, invT, invT_x, th, flags)
            assert torch.equal(dz.cpu().view(torch.int32), rdz.view(torch.int32)), (term, company, dt)
            # two launches give identical bytes
            assert torch.equal(dz, ops.teacher_loss_bwd(zg, tg, None, sg, mg, bg, gmax, acc, gog, invT, invT_x, th, flags))


@pytest.mark.parametrize("N,C,h,w,H,W,S", LOW)
@pytest.mark.parametrize("term", sorted(TERMS))
def test_lowres_scans_equal_the_materialised_path(N, C, h, w, H, W, S, term):
    ops = _gpu()
    from mulactseg_amd import _lib
    _, tgt, spx, msk = _inputs(900 + W + C, N, C, H, W, S)
    f, temp, th = TERMS[term]
    zq = torch.from_numpy(synth.logits(77 + h, N, C, h, w)).cuda()
    tq = torch.from_numpy(synth.logits(78 + h, N, C, h, w)).cuda() if f & TOP1 else None
    invT, invT_x = ops.inv_temperature(T), ops.inv_temperature(temp)
    st, mt = torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda()
    bits = ops.target_bits(torch.from_numpy(tgt).cuda())
    zfull = ops.upsample_bilinear(zq, (H, W))
    tfull = None if tq is None else ops.upsample_bilinear(tq, (H, W))
    got = torch.from_numpy(GO4).cuda()
    for flags in (f, f | CE | GROUP):
        l_full, a_full, g_full = ops.teacher_loss_fwd(zfull, tfull, None, st, mt, bits, invT, invT_x, th, flags)
        l_low, a_low, g_low = ops.teacher_loss_fwd(zq, tq, (H, W), st, mt, bits, invT, invT_x, th, flags)
        assert int(a_full[9]) > 0
        assert torch.equal(a_low, a_full) and torch.equal(l_low.view(torch.int32), l_full.view(torch.int32))
        if g_full is not None:
            assert torch.equal(g_low, g_full)
        dzq = ops.teacher_loss_bwd(zq, tq, (H, W), st, mt, bits, g_low, a_low, got, invT, invT_x, th, flags)
        dz = ops.teacher_loss_bwd(zfull, tfull, None, st, mt, bits, g_full, a_full, got, invT, invT_x, th, flags)
        ref = torch.empty_like(zq)
        _lib.check(_lib.load().mas_upsample_bilinear_bwd(dz.data_ptr(), N * C, h, w, H, W, ref.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "mas_upsample_bilinear_bwd")
        scale, err = float(ref.abs().max()), float((dzq - ref).abs().max())
        print("lowres %s flags %d: max error %.3e of max|ref| %.3e" % (term, flags, err, scale))
        assert scale > 0 and err <= 2e-6 * scale                    # (the bound of tests/test_partial_label_gpu.py: f32 sum against fixed point)
        assert torch.equal(dzq, ops.teacher_loss_bwd(zq, tq, (H, W), st, mt, bits, g_low, a_low, got, invT, invT_x, th, flags))
    for dt in (torch.int32, torch.int16):                           # the id types take the same path at low resolution
        _, a2, _ = ops.teacher_loss_fwd(zq, tq, (H, W), st.to(dt), mt, bits, invT, invT_x, th, flags)
        assert torch.equal(a2, a_low)
        assert torch.equal(dzq, ops.teacher_loss_bwd(zq, tq, (H, W), st.to(dt), mt, bits, g_low, a_low, got, invT, invT_x, th, flags))


@pytest.mark.parametrize("term", sorted(TERMS))
def test_the_co_resident_terms_are_untouched_by_the_new_slot(term):
    """pos and group values, the group table and the group gradient == the scan without the new term, bit for bit"""
    ops = _gpu()
    z, zt, tgt, spx, msk = _case(SHAPES[2])
    f, temp, th = TERMS[term]
    invT, invT_x = ops.inv_temperature(T), ops.inv_temperature(temp)
    zg, sg, mg, bg = torch.from_numpy(z).cuda(), torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda(), _bits(tgt).cuda()
    tg = torch.from_numpy(zt).cuda() if f & TOP1 else None
    base = CE | GROUP
    l0, a0, g0 = ops.partial_loss_fwd(zg, sg, mg, bg, invT, base)
    l1, a1, g1 = ops.teacher_loss_fwd(zg, tg, None, sg, mg, bg, invT, invT_x, th, base | f)
    assert torch.equal(g0, g1) and torch.equal(a0[:7], a1[:7]) and torch.equal(l0.view(torch.int32), l1[:3].view(torch.int32))
    assert float(l1[0]) > 0 and float(l1[2]) > 0 and float(l1[3]) > 0
    for go in ([0.0, 0.0, 1.0], [16.0, 0.0, 1.0]):
        d0 = ops.partial_loss_bwd(zg, sg, mg, bg, g0, a0, torch.tensor(go, device='cuda'), invT, base)
        d1 = ops.teacher_loss_bwd(zg, tg, None, sg, mg, bg, g1, a1, torch.tensor(go + [0.0], device='cuda'), invT, invT_x, th, base | f)
        assert torch.equal(d0, d1) and float(d0.abs().max()) > 0


def _close(got, ref, tol=1e-4):
    return abs(float(got) - float(ref)) <= tol * max(1.0, abs(float(ref)))


def test_modules_match_the_executed_reference():
    ops = _gpu()
    from mulactseg_amd.utils import loss as L
    g, z, zt, tgt, spx, msk = _golden()
    C, S, w = int(g['C']), int(g['S']), float(g['weight'])
    tt, ts, tm, teach = torch.from_numpy(tgt).cuda(), torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda(), torch.from_numpy(zt).cuda()

    def grad_close(zs, ref):
        err = float(np.max(np.abs(zs.grad.cpu().numpy() - ref)))
        print("module gradient: max error %.3e of max|ref| %.3e" % (err, np.max(np.abs(ref))))
        return err <= 1e-4 * float(np.max(np.abs(ref)))

    for key, within in (('top1_th0', False), ('top1_half', False), ('top1w_th0', True), ('top1w_half', True)):
        zs = torch.from_numpy(z).cuda().requires_grad_(True)
        crit = L.TopOnePlbl(num_class=C, within_filtering=within, filtering_threshold=float(g[key + '_th']), temperature=float(g['temp_top1']))
        loss = crit(zs, teach, tt, ts, tm)
        (w * loss).backward()
        assert int(crit.last_acc[9]) == int(g[key + '_n'])
        assert _close(loss, g[key + '_loss']) and grad_close(zs, g[key + '_grad']), key
    zs = torch.from_numpy(z).cuda().requires_grad_(True)
    loss = L.MultiChoiceEnt_(num_class=C, temperature=float(g['temp_ent']))(zs, tt, ts, tm)
    (w * loss).backward()
    assert _close(loss, g['ent_loss']) and grad_close(zs, g['ent_grad'])
    # the fused module: each value is the stand-alone module's, bit for bit
    for term, alone in (('top1', L.TopOnePlbl(num_class=C, temperature=1.0)), ('ent', L.MultiChoiceEnt_(num_class=C, temperature=T))):
        fused = L.FusedTeacherTermLoss(S, term, T, T, 1.0 if term == 'top1' else T)
        pos, group, x = fused(torch.from_numpy(z).cuda(), teach if term == 'top1' else None, tt, ts, tm)
        zd = torch.from_numpy(z).cuda()
        assert float(pos) == float(L.MultiChoiceCE_(num_class=C, temperature=T)(zd, tt, ts, tm))
        assert float(group) == float(L.GroupMultiLabelCE_(args=None, num_class=C, num_superpixel=S, temperature=T)(zd, tt, ts, tm))
        assert float(x) == float(alone(zd, teach, tt, ts, tm) if term == 'top1' else alone(zd, tt, ts, tm)) and float(x) > 0


def test_forward_lowres_builds_no_full_resolution_tensor():
    _gpu()
    from mulactseg_amd.utils import loss as L
    N, C, h, w, S = 2, 20, 24, 40, 64
    H, W = 4 * h, 4 * w
    _, tgt, spx, msk = _inputs(43, N, C, H, W, S)
    tg, sp, mk = torch.from_numpy(tgt).cuda(), torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda()
    zq = torch.from_numpy(synth.logits(6, N, C, h, w)).cuda().requires_grad_(True)
    tq = torch.from_numpy(synth.logits(7, N, C, h, w)).cuda()
    crit = L.FusedTeacherTermLoss(S, 'top1', T, T, 1.0, sync_normalisers=False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pos, group, x = crit.forward_lowres(zq, tq, (H, W), tg, sp, mk)
    (16.0 * pos + group + 0.5 * x).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak allocation of a forward_lowres step: %d bytes; one [N,C,H,W] f32 tensor: %d bytes" % (peak, N * C * H * W * 4))
    assert peak < N * C * H * W * 4 and float(x) > 0 and float(zq.grad.abs().max()) > 0


# ---- trainers ---------------------------------------------------------------------------------------------------------------------
def _trainer(method, extra, itrs, lowres=True, freeze=False, seed=0):
    import importlib
    from mulactseg_amd import dataloader
    from mulactseg_amd.utils import common
    a = common.get_parser().parse_args([
        '-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--method', method, '--ce_temp', '0.1', '--multi_ce_temp', '0.1',
        '--group_ce_temp', '0.1', '--coeff', '16.0', '--or_labeling', '--fair_counting', '--nseg', str(TS), '--train_batch_size', '2',
        '--val_batch_size', '1', '--num_workers', '0', '--val_num_workers', '0', '--train_lr', '2e-5', '--finetune_itrs', str(itrs),
        '--val_period', '1000', '--log_period', '1', '-p', tempfile.mkdtemp()] + extra)
    a.pretrained_backbone = False
    a.lowres_loss = lowres
    if freeze:
        a.freeze_bn = True
    dataloader.register_dataset_factory(lambda args, name, data_root, datalist, imageset: _Val())
    torch.manual_seed(seed)
    tr = importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer(a, logging.getLogger("test"), 1)
    tr._wandb_log = lambda payload, step: None
    return tr


def _run(tr):
    tr.train(types.SimpleNamespace(selection_iter=1, get_trainset=lambda: _Train(N_CLS + 1)))


@pytest.mark.parametrize("method,extra,meter", [
    ('active_joint_multi_predignore_top1plbl', ['--dorampup', '--lamscale', '2.0', '--plbl_th', '0.05', '--within_filtering'], 'top1-loss'),
    ('active_joint_multi_predignore_multient', ['--entcoeff', '0.5'], 'ent-loss')])
@pytest.mark.parametrize("freeze", [False, True])
def test_trainers_run_the_quarter_resolution_step(method, extra, meter, freeze):
    _gpu()
    tr = _trainer(method, extra, 3, freeze=freeze)
    seen = dict(lowres=[], meters=[], modes=[])
    fwd, meter_fn, step = tr.forward_train, tr.update_average_meter, tr.step_losses

    def forward_train(images, **kw):
        seen['lowres'].append(kw.get('lowres', False))
        return fwd(images, **kw)

    def update_average_meter(values):
        seen['meters'].append({k: v.detach().clone() for k, v in values.items()})
        return meter_fn(values)

    def step_losses(*args):
        before = [m.training for m in tr.net.modules()]
        out = step(*args)
        seen['modes'].append((before, [m.training for m in tr.net.modules()]))
        return out

    tr.forward_train, tr.update_average_meter, tr.step_losses = forward_train, update_average_meter, step_losses
    start = [p.detach().clone() for p in tr.net.parameters()]
    _run(tr)
    assert seen['lowres'] == [True] * 3
    names = {'train-loss', 'pos-loss', 'group-loss', meter}
    for m in seen['meters']:
        assert set(m) == names and all(bool(torch.isfinite(v)) for v in m.values())
    assert float(seen['meters'][-1][meter]) > 0
    for before, after in seen['modes']:                             # every module is back in the mode it had
        assert before == after
        bn = [t for m, t in zip(tr.net.modules(), before) if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        assert bn and all(t is (not freeze) for t in bn)
    assert tr.net.training
    moved = sum(float((p.detach() - q).abs().sum()) for p, q in zip(tr.net.parameters(), start))
    assert moved > 0 and np.isfinite(moved)


@pytest.mark.parametrize("method,extra", [('active_joint_multi_predignore_top1plbl', ['--dorampup', '--lamscale', '0']),
                                          ('active_joint_multi_predignore_multient', ['--entcoeff', '0'])])
def test_a_zero_weight_gives_the_parameters_of_the_base_trainer(method, extra):
    """one step with the new term weighted 0 == one step of active_joint_multi_predignore, bit for bit.  Compared on the
    full-resolution step (``lowres_loss = False``), the arithmetic the base trainer runs: the quarter-resolution scans sum the
    gradient in fixed point and cannot equal the f32 upsample backward of the base trainer bit for bit."""
    _gpu()
    base = _trainer('active_joint_multi_predignore', [], 1)
    _run(base)
    tr = _trainer(method, extra, 1, lowres=False)
    _run(tr)
    for (name, p), q in zip(base.net.named_parameters(), tr.net.parameters()):
        assert torch.equal(p, q), name
