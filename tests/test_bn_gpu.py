"""csrc/bn.hip (BatchNorm2d + ReLU + residual add, fused) against torch.nn.BatchNorm2d on the CPU in float64:
forward, running statistics, all gradients, inference mode, determinism; model-level parity and a training step.

Second half: every kernel of the file element by element within derived float32 bounds (tests/helpers.py, proved on the CPU by
tests/test_kernel_bounds_cpu.py), in two steps -- (a) the device's own mean / invstd / running statistics against float64 of the
float32 input, (b) y, dx, dres, dgamma, dbeta against float64 evaluations of the kernels' formulas that take the device's float32
statistics as given -- on a table of shapes that reaches every chunk, boundary-group and loop form of the launchers, each case
asserting the restated launcher arithmetic it is in the table for."""
import copy
import functools
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import helpers as hp

pytestmark = pytest.mark.gpu

CASES = [(4, 8, 24, 32, True, True), (2, 16, 7, 9, True, False), (4, 64, 1, 1, True, False), (3, 5, 33, 37, False, True),
         (2, 12, 96, 96, True, True), (1, 3, 5, 4, False, False),
         # odd planes longer than one reduction chunk (the 769 crop's 193 x 193): aligned-group path, three of four planes misaligned
         (2, 6, 193, 193, True, True), (1, 5, 97, 97, True, False)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _ref(bn64, x, res, relu):
    y = bn64(x)
    if res is not None:
        y = y + res
    return F.relu(y) if relu else y


@pytest.mark.parametrize("N,C,H,W,relu,with_res", CASES)
def test_training_forward_backward_and_running_stats(N, C, H, W, relu, with_res):
    ops = _gpu()
    g = torch.Generator().manual_seed(N * 1000 + C * 10 + H)
    x = torch.randn((N, C, H, W), generator=g) * 2 + 0.5
    res = torch.randn((N, C, H, W), generator=g) if with_res else None
    go = torch.randn((N, C, H, W), generator=g)
    bn = nn.BatchNorm2d(C, momentum=0.1)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    ref_bn = copy.deepcopy(bn).double().train()
    dev_bn = copy.deepcopy(bn).cuda().train()
    xr = x.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if with_res else None
    yr = _ref(ref_bn, xr, rr, relu)
    yr.backward(go.double())
    xd = x.cuda().requires_grad_(True)
    rd = res.cuda().requires_grad_(True) if with_res else None
    assert ops.bn_act_supported(dev_bn, xd, rd)
    yd = ops.bn_act(dev_bn, xd, relu, rd)
    yd.backward(go.cuda())
    tol = lambda ref: 2e-5 * max(1.0, float(ref.abs().max()))
    assert float((yd.detach().double().cpu() - yr.detach()).abs().max()) < tol(yr.detach())
    assert float((xd.grad.double().cpu() - xr.grad).abs().max()) < 5 * tol(xr.grad)
    if with_res:
        assert float((rd.grad.double().cpu() - rr.grad).abs().max()) < tol(rr.grad)
    assert float((dev_bn.weight.grad.double().cpu() - ref_bn.weight.grad).abs().max()) < 20 * tol(ref_bn.weight.grad)
    assert float((dev_bn.bias.grad.double().cpu() - ref_bn.bias.grad).abs().max()) < 20 * tol(ref_bn.bias.grad)
    assert float((dev_bn.running_mean.double().cpu() - ref_bn.running_mean).abs().max()) < 1e-6
    assert float((dev_bn.running_var.double().cpu() - ref_bn.running_var).abs().max()) < 1e-5
    assert int(dev_bn.num_batches_tracked) == 1
    # determinism: a second identical forward/backward gives the same bits
    dev2 = copy.deepcopy(bn).cuda().train()
    x2 = x.cuda().requires_grad_(True)
    r2 = res.cuda().requires_grad_(True) if with_res else None
    y2 = ops.bn_act(dev2, x2, relu, r2)
    y2.backward(go.cuda())
    assert torch.equal(y2, yd) and torch.equal(x2.grad, xd.grad) and torch.equal(dev2.weight.grad, dev_bn.weight.grad)


@pytest.mark.parametrize("N,C,H,W,relu,with_res", CASES[:4])
def test_inference_uses_running_statistics(N, C, H, W, relu, with_res):
    ops = _gpu()
    g = torch.Generator().manual_seed(C)
    x = torch.randn((N, C, H, W), generator=g)
    res = torch.randn((N, C, H, W), generator=g) if with_res else None
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.2)
    bn.eval()
    with torch.no_grad():
        ref = _ref(copy.deepcopy(bn).double(), x.double(), res.double() if with_res else None, relu)
        dev = copy.deepcopy(bn).cuda()
        assert ops.bn_act_supported(dev, x.cuda(), res.cuda() if with_res else None)
        y = ops.bn_act(dev, x.cuda(), relu, res.cuda() if with_res else None)
    assert float((y.double().cpu() - ref).abs().max()) < 2e-6 * max(1.0, float(ref.abs().max()))
    # a frozen BatchNorm inside a training graph is left to PyTorch
    assert not ops.bn_act_supported(dev, x.cuda().requires_grad_(True))


def test_model_training_step_matches_unfused_modules():
    """One SGD step of a Bottleneck stack with the fused path vs the same modules run op by op."""
    ops = _gpu()
    from mulactseg_amd.models import deeplab
    torch.manual_seed(0)
    blk = deeplab.Bottleneck(32, 8, downsample=None).cuda().train()
    ref = copy.deepcopy(blk)
    x = torch.randn(4, 32, 20, 24, device='cuda')

    def unfused(m, t):
        y = F.relu(m.bn1(m.conv1(t)))
        y = F.relu(m.bn2(m.conv2(y)))
        return F.relu(m.bn3(m.conv3(y)) + t)

    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = blk(xa), unfused(ref, xb)
    assert float((ya - yb).detach().abs().max()) < 1e-4
    ya.square().mean().backward()
    yb.square().mean().backward()
    assert float((xa.grad - xb.grad).abs().max()) < 1e-5 * max(1.0, float(xb.grad.abs().max()))
    for (n, p), (_, q) in zip(blk.named_parameters(), ref.named_parameters()):
        assert float((p.grad - q.grad).abs().max()) < 2e-4 * max(1.0, float(q.grad.abs().max())), n
    for (n, b), (_, c) in zip(blk.named_buffers(), ref.named_buffers()):
        assert float((b.double() - c.double()).abs().max()) < 1e-5, n


def test_model_golden_parity_with_fused_bn():
    _gpu()
    from test_model import _check, _load
    g, net, x = _load()
    _check(g, net.cuda(), x.cuda(), 1e-4)


def test_tensors_with_a_storage_offset_take_the_element_path_and_agree():
    """x / residual / upstream gradient that are contiguous views at an odd element offset (planes misaligned differently from the
    freshly allocated outputs): the launch falls back to element-wise groups; values agree with those on aligned copies to rounding."""
    ops = _gpu()
    g = torch.Generator().manual_seed(7)
    N, C, H, W = 2, 4, 9, 11
    big = torch.randn((N * C * H * W + 3,), generator=g).cuda()
    bigr = torch.randn((N * C * H * W + 1,), generator=g).cuda()
    x_view = big[3:].view(N, C, H, W)
    r_view = bigr[1:].view(N, C, H, W)
    bn = nn.BatchNorm2d(C).cuda().train()
    outs = []
    for xs, rs in ((x_view, r_view), (x_view.clone(), r_view.clone())):
        b = copy.deepcopy(bn)
        xq = xs.detach().requires_grad_(True)
        rq = rs.detach().requires_grad_(True)
        y = ops.bn_act(b, xq, True, rq)
        y.backward(torch.ones_like(y) * 0.5)
        outs.append((y.detach(), xq.grad, rq.grad, b.weight.grad, b.running_var.clone()))
    for a, c in zip(*outs):         # the partial sums are grouped by address, so the last bits may differ between the two alignments
        assert float((a - c).abs().max()) <= 2e-6 * max(1.0, float(c.abs().max()))


def test_last_block_statistics_equal_the_separate_launch_bit_for_bit():
    """Round 5: the workgroup that writes a channel's last partial sums forms the channel's statistics (forward: mean / invstd / running
    statistics / num_batches_tracked; backward: dgamma / dbeta / the two means) instead of a launch of their own.  Same partials, same
    order of summation: every output equals the three-launch form (MAS_BN_LASTBLOCK=off) bit for bit, on aligned and odd planes, with
    and without residual, across repeated calls (the completion counters must come back to zero)."""
    import os
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    for (N, C, H, W, res) in ((4, 64, 48, 48, False), (2, 256, 49, 49, True), (4, 128, 97, 33, True), (1, 20, 5, 7, False), (4, 2048, 12, 12, False),
                            # a chunk with one boundary group / one whole group, an empty chunk on every plane (it counts towards per_channel),
                            # planes without a whole group (helpers.BN_CASES 1, 3, 6)
                            (2, 5, 1, 8193, True), (2, 3, 64, 128, True), (3, 5, 1, 3, True)):
        torch.manual_seed(N * C + H)
        x = torch.randn(N, C, H, W, device='cuda') * 2.0 + 0.3
        r = torch.randn(N, C, H, W, device='cuda') if res else None
        dy = torch.randn(N, C, H, W, device='cuda')
        outs = {}
        for mode in ("off", "on", "on"):
            os.environ["MAS_BN_LASTBLOCK"] = mode
            try:
                bn = torch.nn.BatchNorm2d(C).cuda().train()
                with torch.no_grad():
                    bn.weight.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-1, 1, C))
                xi = x.clone().requires_grad_(True)
                ri = r.clone().requires_grad_(True) if res else None
                y = ops.bn_act(bn, xi, True, ri)
                y.backward(dy)
                got = [y.detach(), xi.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()]
                if res:
                    got.append(ri.grad)
            finally:
                os.environ.pop("MAS_BN_LASTBLOCK")
            if mode in outs:
                for a, b in zip(outs[mode], got):
                    assert torch.equal(a, b)
            outs[mode] = got
        for a, b in zip(outs["off"], outs["on"]):
            assert torch.equal(a, b), (N, C, H, W)
        assert int(outs["on"][6]) == 1
    key = (torch.device('cuda', torch.cuda.current_device()), torch.cuda.current_stream().cuda_stream)
    assert int(ops._BN_COUNTERS[key].abs().sum()) == 0


# ---- every kernel of bn.hip, element by element, within derived bounds ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn_case(shape, seed=0, const=None):
    """Inputs of one shape: made once, shared by the tests, never written to."""
    return hp.bn_inputs(*shape, seed=seed, const=const)


def _offset_view(t):
    """A contiguous copy of ``t`` one element into a larger buffer: its address is 4 modulo 16."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device='cuda')
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _module(t, affine=True, track=True, momentum=0.1, eps=1e-5, freeze=()):
    C = t['gamma'].numel()
    bn = nn.BatchNorm2d(C, eps=eps, momentum=momentum, affine=affine, track_running_stats=track)
    with torch.no_grad():
        if affine:
            bn.weight.copy_(t['gamma']); bn.bias.copy_(t['beta'])
        if track:
            bn.running_mean.copy_(t['rm']); bn.running_var.copy_(t['rv'])
    for name in freeze:
        getattr(bn, name).requires_grad_(False)
    return bn.cuda().train()


def _run_bn(bn, t, relu=True, res_grad=True, dy=None, partials=None):
    """One forward / backward of ops.bn_act on aligned device copies of t (dy: a device tensor to use as the upstream gradient).
    -> the outputs, the statistics the forward saved for the backward, and the running statistics before and after."""
    from mulactseg_amd import ops
    xd, rd = t['x'].cuda().requires_grad_(True), t['res'].cuda().requires_grad_(res_grad)
    dyd = t['dy'].cuda() if dy is None else dy
    before = (bn.running_mean.clone().cpu(), bn.running_var.clone().cpu()) if bn.track_running_stats else (None, None)
    assert ops.bn_act_supported(bn, xd, rd)
    y = ops.bn_act(bn, xd, relu, rd, partials=partials)
    saved = y.grad_fn.saved_tensors
    assert all(v.data_ptr() % 16 == 0 for v in (xd, rd, y))                    # the forward takes the float4 form
    y.backward(dyd)
    assert xd.grad.data_ptr() % 16 == 0
    return dict(x=xd.detach(), y=y.detach(), mean=saved[3].clone(), invstd=saved[4].clone(), mask=saved[5], dx=xd.grad, dres=rd.grad,
                dgamma=None if bn.weight is None else bn.weight.grad, dbeta=None if bn.bias is None else bn.bias.grad, rm0=before[0], rv0=before[1],
                rm=bn.running_mean.clone() if bn.track_running_stats else None, rv=bn.running_var.clone() if bn.track_running_stats else None,
                nbt=int(bn.num_batches_tracked) if bn.track_running_stats else None)


def _check_stats(t, out, bn, what, **chain):
    """(a) the device's statistics against float64 of the float32 input."""
    ref = hp.bn_stats_reference(t['x'], bn.eps, bn.momentum, out['rm0'], out['rv0'], **chain) if bn.track_running_stats else \
        hp.bn_stats_reference(t['x'], bn.eps, **chain)
    hp.assert_within(out['mean'], ref['mean'], ref['mean_bound'], "bn mean " + what)
    hp.assert_within(out['invstd'], ref['invstd'], ref['invstd_bound'], "bn invstd " + what)
    if bn.track_running_stats:
        hp.assert_within(out['rm'], ref['rm'], ref['rm_bound'], "bn running_mean " + what)
        hp.assert_within(out['rv'], ref['rv'], ref['rv_bound'], "bn running_var " + what)
    return ref


def _check_apply_and_backward(t, out, bn, what, relu=True, res_grad=True):
    """(b) y, dres (exact), dbeta, dgamma, dx against the kernels' formulas on the device's float32 statistics."""
    gamma, beta = (t['gamma'], t['beta']) if bn.affine else (None, None)
    mean, invstd = out['mean'].cpu(), out['invstd'].cpu()
    y = out['y'].cpu()
    yr, yb = hp.bn_apply_reference(t['x'], gamma, beta, t['res'], mean, invstd, relu)
    hp.assert_within(y, yr, yb, "bn y " + what)
    if relu:
        assert bool((y >= 0).all()) and not bool(torch.signbit(y).any())       # exact zeros, none of them negative
        assert out['mask'] is not None
    ref = hp.bn_backward_reference(t['x'], t['dy'], y, gamma, mean, invstd, relu)
    if res_grad:
        assert torch.equal(out['dres'].cpu(), ref['dres']), "dres is not dy * [y > 0] bit for bit"
    else:
        assert out['dres'] is None
    hp.assert_within(out['dx'], ref['dx'], ref['dx_bound'], "bn dx " + what)
    for name, p in (('dgamma', 'weight'), ('dbeta', 'bias')):
        if bn.affine and getattr(bn, p).requires_grad:
            hp.assert_within(out[name], ref[name], ref[name + '_bound'], "bn %s %s" % (name, what))
        else:
            assert out[name] is None
    return ref


def _paths_on_device(shape, out):
    N, C, H, W = shape
    return hp.bn_paths(N, C, H * W, offset=(out['x'].data_ptr() // 4) % 4)


@pytest.mark.parametrize("shape,expect", hp.BN_CASES)
def test_every_chunk_and_group_form(shape, expect):
    """relu + residual on the case table: chunk edges (a second chunk that is empty, holds one boundary group, holds one whole
    group), every misalignment, two trips through the four-group loop of k_bn_bwd_partial, its clamped duplicate, planes without a whole
    group, one-element planes.  The same bits twice."""
    _gpu()
    t = _bn_case(shape)
    bn = _module(t)
    out = _run_bn(bn, t)
    got = _paths_on_device(shape, out)
    assert got.pop('per_thread') <= 8 and got == expect
    what = "%dx%dx%dx%d" % shape
    _check_stats(t, out, bn, what)
    _check_apply_and_backward(t, out, bn, what)
    assert out['nbt'] == 1
    again = _run_bn(_module(t), t)
    for name in ('y', 'mean', 'invstd', 'dx', 'dres', 'dgamma', 'dbeta', 'rm', 'rv'):
        assert torch.equal(out[name], again[name]), name


@pytest.mark.parametrize("option", hp.BN_OPTIONS)
@pytest.mark.parametrize("shape", hp.BN_OPTION_CASES)
def test_options_one_at_a_time(shape, option):
    """Null gamma / beta, null running pointers, dres / dgamma / dbeta not asked for, no ReLU under a residual, other momenta and eps, a
    second step on the same module -- each on a two-chunk case, on odd planes and on planes without a whole group."""
    _gpu()
    t = _bn_case(shape)
    kw, relu, res_grad = {}, True, True
    if option == 'affine_false':
        kw['affine'] = False
    elif option == 'no_running_stats':
        kw['track'] = False
    elif option == 'residual_no_grad':
        res_grad = False
    elif option == 'frozen_weight':
        kw['freeze'] = ('weight',)
    elif option == 'frozen_bias':
        kw['freeze'] = ('bias',)
    elif option == 'no_relu':
        relu = False
    elif option.startswith('momentum_'):
        kw['momentum'] = float(option.split('_')[1])
    elif option == 'eps_1e-3':
        kw['eps'] = 1e-3
    bn = _module(t, **kw)
    what = "%dx%dx%dx%d %s" % (shape + (option,))
    out = _run_bn(bn, t, relu=relu, res_grad=res_grad)
    _check_stats(t, out, bn, what)
    _check_apply_and_backward(t, out, bn, what, relu=relu, res_grad=res_grad)
    if option == 'no_relu':
        assert out['mask'] is None and bool((out['y'] < 0).any())
    if option == 'no_running_stats':
        assert bn.running_mean is None and out['nbt'] is None
    else:
        assert out['nbt'] == 1
    if option == 'two_steps':
        # the second step starts from the running statistics the first one left on the device (taken as given) and counts to 2
        t2 = dict(_bn_case(shape, seed=1), gamma=t['gamma'], beta=t['beta'])          # (the module keeps its parameters)
        bn.zero_grad(set_to_none=True)
        out2 = _run_bn(bn, t2)
        assert torch.equal(out2['rm0'], out['rm'].cpu()) and torch.equal(out2['rv0'], out['rv'].cpu())
        assert not torch.equal(out2['rm'], out['rm']) and not torch.equal(out2['rv'], out['rv'])
        _check_stats(t2, out2, bn, what + " step 2")
        _check_apply_and_backward(t2, out2, bn, what + " step 2")
        assert out2['nbt'] == 2


@pytest.mark.parametrize("shape", hp.BN_OPTION_CASES)
def test_forward_vectorised_backward_not(shape):
    """The upstream gradient is a contiguous view one element off a 16-byte boundary: k_bn_apply ran on float4 groups, k_bn_bwd_partial /
    k_bn_bwd_apply fall back to the element path (not congruent with x).  Within the bounds of (b), which do not depend on the
    partition of the sums; dres, which has no sum in it, equals the aligned run bit for bit."""
    _gpu()
    t = _bn_case(shape)
    bn = _module(t)
    dy = _offset_view(t['dy'].cuda())
    out = _run_bn(bn, t, dy=dy)
    assert (out['x'].data_ptr() ^ dy.data_ptr()) & 15 != 0                        # congruent(x, dy) of the launcher is false
    _check_apply_and_backward(t, out, bn, "%dx%dx%dx%d dy at +1" % shape)
    aligned = _run_bn(_module(t), t)
    assert torch.equal(out['y'], aligned['y']) and torch.equal(out['dres'], aligned['dres'])


def _bwd_direct(t, fwd, y, shape):
    """mas_bn_act_train_bwd through the C ABI with relu_mask = NULL: the gate is read from y."""
    from mulactseg_amd import _lib, ops
    N, C, H, W = shape
    lib = _lib.load()
    xd, dyd, gm = fwd['x'], t['dy'].cuda(), t['gamma'].cuda()
    ws = torch.empty(int(lib.mas_bn_workspace_bytes(N, C, H * W)), dtype=torch.uint8, device='cuda')
    dx, dres = torch.full_like(xd, float('nan')), torch.full_like(xd, float('nan'))
    dg, db = torch.full((C,), float('nan'), device='cuda'), torch.full((C,), float('nan'), device='cuda')
    assert all(v.data_ptr() % 16 == 0 for v in (xd, dyd, dx, dres))
    _lib.check(lib.mas_bn_act_train_bwd(dyd.data_ptr(), xd.data_ptr(), y.data_ptr(), None, gm.data_ptr(), fwd['mean'].data_ptr(),
                                        fwd['invstd'].data_ptr(), N, C, H * W, 1, ws.data_ptr(), dx.data_ptr(), dres.data_ptr(), dg.data_ptr(),
                                        db.data_ptr(), None, ops._stream(xd)), "mas_bn_act_train_bwd")
    torch.cuda.synchronize()
    return dict(dx=dx, dres=dres, dgamma=dg, dbeta=db)


@pytest.mark.parametrize("shape,expect", [hp.BN_CASES[0], hp.BN_CASES[5]])
def test_backward_gated_by_y_equals_the_mask_gated_backward(shape, expect):
    """The ReLU gate read from y (relu_mask = NULL: part of the C ABI, never taken by ops.py) against the gate read from the mask: the
    same gate, so every output has the same bits as the mask-gated launch OF THE SAME FORM.  y congruent with x: the float4 form, against
    the aligned autograd run.  y one element off: the element form, against the mask-gated element form (upstream gradient one element
    off).  The two forms hand the groups to the threads differently when a plane is misaligned (from flo / from lo), so their sums
    may differ in the last bit -- except where no plane has a whole group, where they are one partition; dres, which has no sum in
    it, agrees across the forms everywhere."""
    _gpu()
    t = _bn_case(shape)
    vec = _run_bn(_module(t), t)
    elem = _run_bn(_module(t), t, dy=_offset_view(t['dy'].cuda()))
    assert vec['mask'] is not None
    by_y = _bwd_direct(t, vec, vec['y'], shape)
    y_off = _offset_view(vec['y'])
    assert (vec['x'].data_ptr() ^ y_off.data_ptr()) & 15 != 0
    by_y_elem = _bwd_direct(t, vec, y_off, shape)
    for name in ('dx', 'dres', 'dgamma', 'dbeta'):
        assert torch.equal(by_y[name], vec[name]), "float4 form, %s" % name
        assert torch.equal(by_y_elem[name], elem[name]), "element form, %s" % name
        if expect['no_full']:
            assert torch.equal(by_y_elem[name], vec[name]), "both forms, %s" % name
    assert torch.equal(by_y_elem['dres'], vec['dres'])


@pytest.mark.parametrize("per_channel", [1, 255, 256, 257, 1000])
def test_statistics_from_exact_partials(per_channel):
    """k_bn_stats_wide: bn_act(partials=) with float64 partial sums of disjoint pixel sets (pixel j of a channel in set j % per_channel;
    sets beyond the 640 pixels are empty), around the 256-way stride.  The partials are exact to double rounding, so the statistics err
    only by their final casts: the bounds of (a) with no float32 chain."""
    _gpu()
    shape = (2, 3, 16, 20)
    N, C, H, W = shape
    t = _bn_case(shape)
    xc = t['x'].double().transpose(0, 1).reshape(C, -1)
    n = xc.shape[1]
    sets = torch.arange(n) % per_channel
    P = torch.zeros((C, per_channel, 2), dtype=torch.float64)
    P[:, :, 0].index_add_(1, sets, xc)
    P[:, :, 1].index_add_(1, sets, xc * xc)
    bn = _module(t)
    out = _run_bn(bn, t, partials=P.cuda())
    what = "partials=%d" % per_channel
    # double roundings: up to ceil(n / per_channel) additions inside a partial, ceil(per_channel / 256) per thread, six shuffles, three waves
    chain = dict(c_s=0, c_q=0, c_d=(n + per_channel - 1) // per_channel + (per_channel + 255) // 256 + 9)
    _check_stats(t, out, bn, what, **chain)
    _check_apply_and_backward(t, out, bn, what)
    assert out['nbt'] == 1


@pytest.mark.parametrize("shape", [hp.BN_CASES[4][0], hp.BN_CASES[5][0]])
def test_constant_planes(shape):
    """x == 0.5 everywhere: every float32 partial sum is exact, so mean == 0.5, var == 0 and invstd == 1 / sqrt(eps) exactly;
    xhat == 0, so y == relu(beta + res) with one rounding, dgamma == 0, and dx = k (g - mean g) within the bound of (b)."""
    _gpu()
    t = _bn_case(shape, const=0.5)
    bn = _module(t)
    out = _run_bn(bn, t)
    C = shape[1]
    assert torch.equal(out['mean'].cpu(), torch.full((C,), 0.5))
    assert torch.equal(out['invstd'].cpu(), torch.full((C,), 1.0 / math.sqrt(hp.f32_as_float(bn.eps)), dtype=torch.float64).float())
    assert torch.equal(out['y'].cpu(), torch.relu(t['beta'].view(1, C, 1, 1) + t['res']))
    assert torch.equal(out['dgamma'].cpu(), torch.zeros(C))
    what = "%dx%dx%dx%d constant" % shape
    _check_stats(t, out, bn, what)
    _check_apply_and_backward(t, out, bn, what)


def test_conditioning_of_the_one_pass_variance():
    """var = Q / n - m^2 from float32 partial sums loses (mean / std)^2 roundings: four channels of unit variance with mean / std of 0,
    1, 8 and 64, judged by the bound of (a), which grows the same way (relative bound on invstd: 4e-7, 1.4e-6, 6e-5, 4e-3).  The
    measured relative error of invstd is printed per channel (on an MI355X: 2.8e-8, 1.4e-8, 1.0e-7, 9.8e-6).  The one-pass form is
    good to a relative 1e-4 up to mean / std of about 64; beyond that it wants a shifted or two-pass variance."""
    _gpu()
    x = hp.bn_conditioning_input()
    C = x.shape[1]
    t = dict(_bn_case((2, C, 1, 1221)), x=x)
    bn = _module(t)
    out = _run_bn(bn, t)
    ref = _check_stats(t, out, bn, "conditioning")
    rel = ((out['invstd'].double().cpu() - ref['invstd']) / ref['invstd']).abs()
    print("relative invstd error at mean/std 0, 1, 8, 64:", ["%.2e" % float(v) for v in rel],
          " bound:", ["%.2e" % float(v) for v in ref['invstd_bound'] / ref['invstd']])
    _check_apply_and_backward(t, out, bn, "conditioning")


@pytest.mark.parametrize("shape", [hp.BN_CASES[4][0], hp.BN_CASES[5][0]])
@pytest.mark.parametrize("relu", [True, False])
def test_inference_within_the_apply_bound(shape, relu):
    """k_bn_apply<FROM_VAR>: the bound of (b) with the three roundings of 1 / sqrtf(var + eps)."""
    ops = _gpu()
    t = _bn_case(shape)
    bn = _module(t).eval()
    with torch.no_grad():
        y = ops.bn_act(bn, t['x'].cuda(), relu, t['res'].cuda())
    yr, yb = hp.bn_apply_reference(t['x'], t['gamma'], t['beta'], t['res'], t['rm'], t['rv'], relu, eps=bn.eps)
    hp.assert_within(y, yr, yb, "bn y inference %dx%dx%dx%d" % shape)
    assert torch.equal(bn.running_mean.cpu(), t['rm']) and int(bn.num_batches_tracked) == 0
