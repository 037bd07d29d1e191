"""The teacher-weighted group term on the GPU: the MAS_TT_WGROUP instantiations of the loss scans and the weighted finalize
(csrc/losses.hip) against the library's host loop through csrc/teacher_terms.h (``ops.wgroup_loss_reference``) bit for bit -- vector and
scalar path, the three id types, the LDS tables and their overflow to global memory, with and without the co-resident terms --, the
quarter-resolution scans against the materialised upsample, the co-resident terms against the scans without the new bit, the modules
against the executed reference (tests/golden/g18_wgroup.npz), the allocator peak of a quarter-resolution step, and the trainer end to
end."""
import numpy as np
import pytest
import torch

from mulactseg_amd import synth

from test_losses_gpu import _inputs
from test_partial_label_cpu import SHAPES
from test_partial_label_gpu import LOW
from test_teacher_terms_gpu import _run, _trainer
from test_wgroup_cpu import CE, DECOMP, GROUP, ONLY_MULTI, T, WGROUP, _bits, _golden

pytestmark = pytest.mark.gpu
GO3 = np.array([16.0, 8.0, 3.0], dtype=np.float32)
COMPANY = (GROUP, CE | GROUP, CE | DECOMP | GROUP | ONLY_MULTI)


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
def test_kernels_equal_the_host_reference_bit_for_bit(shape):
    ops = _gpu()
    z, zt, tgt, spx, msk = _case(shape, force_bit31=shape[1] == 32)
    invT = ops.inv_temperature(T)
    bits = _bits(tgt)
    if shape[1] == 32:
        assert bool((bits.view(torch.int32) < 0).all())                      # bit 31 in every candidate set
    zc, tc, sc, mc = torch.from_numpy(z), torch.from_numpy(zt), torch.from_numpy(spx), torch.from_numpy(msk)
    zg, tg, mg, bg, gog = zc.cuda(), tc.cuda(), mc.cuda(), bits.cuda(), torch.from_numpy(GO3).cuda()
    for company in COMPANY:
        flags = company | WGROUP
        rl, racc, rgmax, rtmax, rdz = ops.wgroup_loss_reference(zc, tc, sc, mc, bits, invT, flags, grad_out=torch.from_numpy(GO3))
        assert int(racc[6]) > 0 and float(rdz.abs().max()) > 0
        for dt in (torch.int64, torch.int32, torch.int16):
            sg = sc.to(dt).cuda()
            losses, acc, gmax, tmax = ops.wgroup_loss_fwd(zg, tg, None, sg, mg, bg, invT, flags)
            assert torch.equal(acc.cpu()[:7], racc[:7]), (company, dt)
            assert torch.equal(gmax.cpu(), rgmax) and torch.equal(tmax.cpu(), rtmax), (company, dt)
            assert torch.equal(losses.cpu().view(torch.int32), rl.view(torch.int32)), (company, dt)
            dz = ops.wgroup_loss_bwd(zg, tg, None, sg, mg, bg, gmax, tmax, acc, gog, invT, flags)
            assert torch.equal(dz.cpu().view(torch.int32), rdz.view(torch.int32)), (company, dt)
            # two launches give identical bytes
            assert torch.equal(dz, ops.wgroup_loss_bwd(zg, tg, None, sg, mg, bg, gmax, tmax, acc, gog, invT, flags))
        # the values the finalize's last workgroup writes == mas_loss_values after a reduction hook
        l2, a2, _, _ = ops.wgroup_loss_fwd(zg, tg, None, sg, mg, bg, invT, flags, reduce_acc=lambda a: None)
        assert torch.equal(l2.view(torch.int32), losses.view(torch.int32)) and torch.equal(a2[:7], acc[:7])


@pytest.mark.parametrize("shape", [(1, 20, 6, 301, 160), (2, 19, 8, 300, 200)])
def test_more_superpixels_in_a_tile_than_table_slots(shape):
    """Both tables overflow to global memory.  The crops of ``_inputs`` select whole superpixels, at most 15 of them in any 4 x 256 tile
    of SHAPES (S = 150 included), so the 64 slots never fill there; here every pixel is selected and the ids run along the row, so each
    tile holds more than 64 superpixels.  Scalar (W = 301) and vector (W = 300) path."""
    ops = _gpu()
    N, C, H, W, S = shape
    z, tgt, _, _ = _inputs(300 + W + C, N, C, H, W, S)
    zt = synth.logits(500 + W + C, N, C, H, W)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    spx = np.ascontiguousarray(np.broadcast_to((x * 7 + y) % S, (N, H, W))).astype(np.int64)
    msk = np.ones((N, H, W), dtype=bool)
    for t0 in range(0, H, 4):
        for x0 in range(0, W, 256):
            assert np.unique(spx[0, t0:t0 + 4, x0:x0 + 256]).size > 64
    invT, bits = ops.inv_temperature(T), _bits(tgt)
    zc, tc, sc, mc = torch.from_numpy(z), torch.from_numpy(zt), torch.from_numpy(spx), torch.from_numpy(msk)
    for flags in (GROUP | WGROUP, CE | GROUP | ONLY_MULTI | WGROUP):
        rl, racc, rgmax, rtmax, rdz = ops.wgroup_loss_reference(zc, tc, sc, mc, bits, invT, flags, grad_out=torch.from_numpy(GO3))
        assert int(racc[6]) > 64
        losses, acc, gmax, tmax = ops.wgroup_loss_fwd(zc.cuda(), tc.cuda(), None, sc.cuda(), mc.cuda(), bits.cuda(), invT, flags)
        assert torch.equal(acc.cpu()[:7], racc[:7]) and torch.equal(gmax.cpu(), rgmax) and torch.equal(tmax.cpu(), rtmax)
        assert torch.equal(losses.cpu().view(torch.int32), rl.view(torch.int32))
        dz = ops.wgroup_loss_bwd(zc.cuda(), tc.cuda(), None, sc.cuda(), mc.cuda(), bits.cuda(), gmax, tmax, acc, torch.from_numpy(GO3).cuda(),
                                 invT, flags)
        assert torch.equal(dz.cpu().view(torch.int32), rdz.view(torch.int32))


@pytest.mark.parametrize("N,C,h,w,H,W,S", LOW)
def test_lowres_scans_equal_the_materialised_path(N, C, h, w, H, W, S):
    ops = _gpu()
    from mulactseg_amd import _lib
    _, tgt, spx, msk = _inputs(900 + W + C, N, C, H, W, S)
    zq = torch.from_numpy(synth.logits(77 + h, N, C, h, w)).cuda()
    tq = torch.from_numpy(synth.logits(78 + h, N, C, h, w)).cuda()
    invT = ops.inv_temperature(T)
    st, mt = torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda()
    bits = ops.target_bits(torch.from_numpy(tgt).cuda())
    zfull, tfull = ops.upsample_bilinear(zq, (H, W)), ops.upsample_bilinear(tq, (H, W))
    got = torch.from_numpy(GO3).cuda()
    for flags in (GROUP | WGROUP, CE | GROUP | WGROUP):
        l_full, a_full, g_full, t_full = ops.wgroup_loss_fwd(zfull, tfull, None, st, mt, bits, invT, flags)
        l_low, a_low, g_low, t_low = ops.wgroup_loss_fwd(zq, tq, (H, W), st, mt, bits, invT, flags)
        assert int(a_full[6]) > 0
        assert torch.equal(a_low[:7], a_full[:7]) and torch.equal(l_low.view(torch.int32), l_full.view(torch.int32))
        assert torch.equal(g_low, g_full) and torch.equal(t_low, t_full) and bool((t_full != 0).any())
        dzq = ops.wgroup_loss_bwd(zq, tq, (H, W), st, mt, bits, g_low, t_low, a_low, got, invT, flags)
        dz = ops.wgroup_loss_bwd(zfull, tfull, None, st, mt, bits, g_full, t_full, a_full, got, invT, flags)
        ref = torch.empty_like(zq)
        _lib.check(_lib.load().mas_upsample_bilinear_bwd(dz.data_ptr(), N * C, h, w, H, W, ref.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "mas_upsample_bilinear_bwd")
        scale, err = float(ref.abs().max()), float((dzq - ref).abs().max())
        print("lowres wgroup flags %d: max error %.3e of max|ref| %.3e" % (flags, err, scale))
        assert scale > 0 and err <= 2e-6 * scale                    # (the bound of tests/test_partial_label_gpu.py: f32 sum against fixed point)
        assert torch.equal(dzq, ops.wgroup_loss_bwd(zq, tq, (H, W), st, mt, bits, g_low, t_low, a_low, got, invT, flags))
    for dt in (torch.int32, torch.int16):                           # the id types take the same path at low resolution
        _, a2, _, t2 = ops.wgroup_loss_fwd(zq, tq, (H, W), st.to(dt), mt, bits, invT, flags)
        assert torch.equal(a2[:7], a_low[:7]) and torch.equal(t2, t_low)
        assert torch.equal(dzq, ops.wgroup_loss_bwd(zq, tq, (H, W), st.to(dt), mt, bits, g_low, t_low, a_low, got, invT, flags))


def test_the_co_resident_terms_are_untouched_by_the_weighting():
    """ce / mc values, the student's table and the counts == the scan without the new bit; with a zero upstream gradient of the group
    term the backward is that scan's, bit for bit"""
    ops = _gpu()
    z, zt, tgt, spx, msk = _case(SHAPES[2])
    invT = ops.inv_temperature(T)
    zg, tg = torch.from_numpy(z).cuda(), torch.from_numpy(zt).cuda()
    sg, mg, bg = torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda(), _bits(tgt).cuda()
    base = CE | GROUP
    l0, a0, g0 = ops.partial_loss_fwd(zg, sg, mg, bg, invT, base)
    l1, a1, g1, t1 = ops.wgroup_loss_fwd(zg, tg, None, sg, mg, bg, invT, base | WGROUP)
    assert torch.equal(g0, g1) and torch.equal(a0[:5], a1[:5]) and int(a0[6]) == int(a1[6]) > 0
    assert torch.equal(l0[:2].view(torch.int32), l1[:2].view(torch.int32))
    assert float(l1[0]) > 0 and 0 < float(l1[2]) < float(l0[2])       # every weight is a probability
    go = torch.tensor([16.0, 0.0, 0.0], device='cuda')
    d0 = ops.partial_loss_bwd(zg, sg, mg, bg, g0, a0, go, invT, base)
    d1 = ops.wgroup_loss_bwd(zg, tg, None, sg, mg, bg, g1, t1, a1, go, invT, base | WGROUP)
    assert torch.equal(d0, d1) and float(d0.abs().max()) > 0
    # a teacher equal to the student: its table is the probability half of the student's
    _, _, g2, t2 = ops.wgroup_loss_fwd(zg, zg.clone(), None, sg, mg, bg, invT, base | WGROUP)
    assert torch.equal(t2, (g2 >> 32).to(torch.int32)) and bool((g2 != 0).any())


def _close(got, ref, tol=1e-4):
    return abs(float(got) - float(ref)) <= tol * max(1.0, abs(float(ref)))


@pytest.mark.parametrize("only_single", [False, True])
def test_modules_match_the_executed_reference(only_single):
    import types
    _gpu()
    from mulactseg_amd.utils import loss as L
    g, z, zt, tgt, spx, msk = _golden()
    C, S, w, temp = int(g['C']), int(g['S']), float(g['weight']), float(g['temp'])
    key = 'single' if only_single else 'all'
    tt, ts, tm, teach = torch.from_numpy(tgt).cuda(), torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda(), torch.from_numpy(zt).cuda()
    zs = torch.from_numpy(z).cuda().requires_grad_(True)
    crit = L.WeightedGroupMultiLabelCE(types.SimpleNamespace(group_only_single=only_single), num_class=C, num_superpixel=S, temperature=temp)
    loss = crit(zs, teach, tt, ts, tm)
    (w * loss).backward()
    ref = g[key + '_grad']
    err = float(np.max(np.abs(zs.grad.cpu().numpy() - ref)))
    print("module %s: loss %.7g golden %.7g, n %d; gradient max error %.3e of max|ref| %.3e"
          % (key, float(loss.detach()), float(g[key + "_loss"]), int(crit.last_acc[6]), err, np.max(np.abs(ref))))
    assert int(crit.last_acc[6]) == int(g[key + '_n'])
    assert _close(loss, g[key + '_loss']) and err <= 1e-4 * float(np.max(np.abs(ref)))
    # the fused module: each value is the stand-alone module's, bit for bit
    zd = torch.from_numpy(z).cuda()
    pos, group = L.FusedWGroupLoss(S, temp, temp, group_only_single=only_single)(zd, teach, tt, ts, tm)
    assert float(pos) == float(L.MultiChoiceCE_(num_class=C, temperature=temp)(zd, tt, ts, tm)) and float(pos) > 0
    assert float(group) == float(loss)


def test_forward_lowres_builds_no_full_resolution_tensor():
    _gpu()
    from mulactseg_amd.utils import loss as L
    N, C, h, w, S = 2, 20, 24, 40, 64
    H, W = 4 * h, 4 * w
    _, tgt, spx, msk = _inputs(43, N, C, H, W, S)
    tg, sp, mk = torch.from_numpy(tgt).cuda(), torch.from_numpy(spx).cuda(), torch.from_numpy(msk).cuda()
    zq = torch.from_numpy(synth.logits(6, N, C, h, w)).cuda().requires_grad_(True)
    tq = torch.from_numpy(synth.logits(7, N, C, h, w)).cuda()
    crit = L.FusedWGroupLoss(S, T, T, sync_normalisers=False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pos, group = crit.forward_lowres(zq, tq, (H, W), tg, sp, mk)
    (16.0 * pos + group).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak allocation of a forward_lowres step: %d bytes; one [N,C,H,W] f32 tensor: %d bytes" % (peak, N * C * H * W * 4))
    assert peak < N * C * H * W * 4 and float(group) > 0 and float(zq.grad.abs().max()) > 0


@pytest.mark.parametrize("freeze,extra", [(False, []), (True, []), (False, ['--group_only_single'])])
def test_the_trainer_runs_the_quarter_resolution_step(freeze, extra):
    _gpu()
    tr = _trainer('active_joint_multi_predignore_wgroup', extra, 3, freeze=freeze)
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
    assert bool(tr.fused_loss.flags & ONLY_MULTI) is bool(extra)
    start = [p.detach().clone() for p in tr.net.parameters()]
    _run(tr)
    assert seen['lowres'] == [True] * 3
    for m in seen['meters']:
        assert set(m) == {'train-loss', 'pos-loss', 'group-loss'} and all(bool(torch.isfinite(v)) for v in m.values())
    assert float(seen['meters'][-1]['group-loss']) > 0
    for before, after in seen['modes']:                             # every module is back in the mode it had
        assert before == after
        bn = [t for m, t in zip(tr.net.modules(), before) if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        assert bn and all(t is (not freeze) for t in bn)
    assert tr.net.training
    moved = sum(float((p.detach() - q).abs().sum()) for p, q in zip(tr.net.parameters(), start))
    assert moved > 0 and np.isfinite(moved)
