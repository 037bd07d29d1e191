"""csrc/head.hip against float64 evaluations of its own formulas, element by element within worst-case float32 rounding bounds
(tests/helpers.py; tests/test_kernel_bounds_cpu.py proves them): the cosine classifier on every kernel its launchers select, the
wrapper against F.normalize + conv2d, and the fixed-order dense products of the 1x1 map."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import helpers as hp

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _head_case(N, Ch, H, W, K):
    """Inputs and float64 reference of one shape: computed once, shared by the tests, never written to."""
    f, phat, g = hp.head_inputs(N, Ch, H, W, K)
    return f, phat, g, hp.head_reference(f, phat, g)


def _offset_view(t):
    """A contiguous copy of ``t`` one element into a larger buffer: its address is no multiple of 16."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device='cuda')
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _run_head(feat, phat, g):
    """(logits, inv_norm, dfeat) of ops._CosineHead on device tensors."""
    from mulactseg_amd import ops
    fd = feat.detach().requires_grad_(True)
    out = ops._CosineHead.apply(fd, phat)
    inv = out.grad_fn.saved_tensors[3].clone()
    assert out.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    out.backward(g)
    assert fd.grad.data_ptr() % 16 == 0
    return out.detach(), inv, fd.grad


def _check_head(ref, logits, dfeat, what):
    """logits and dfeat within their bounds; zero feature vectors as the kernel documents them (n = eps): logits exactly 0,
    dfeat_c = (sum_k g_k p_kc) / eps."""
    assert torch.isfinite(logits).all() and torch.isfinite(dfeat).all()
    hp.assert_within(logits, ref['logits'], ref['logits_bound'], what + " logits")
    z = ref['zero']
    assert int(z.sum()) >= 1
    live = (~z)[:, None].expand_as(ref['dfeat'])
    dead = z[:, None].expand_as(ref['dfeat'])
    df = dfeat.cpu()
    hp.assert_within(df[live], ref['dfeat'][live], ref['dfeat_bound'][live], what + " dfeat")
    hp.assert_within(df[dead], ref['dfeat_zero'][dead], ref['dfeat_zero_bound'][dead], what + " dfeat at |f| = 0")
    assert float(logits.cpu()[z[:, None].expand_as(ref['logits'])].abs().max()) == 0.0


@pytest.mark.parametrize("N,Ch,H,W,K,fwd,bwd,offset", hp.HEAD_CASES)
def test_cosine_head_kernel_paths(N, Ch, H, W, K, fwd, bwd, offset):
    """Every kernel of launch_fwd / launch_bwd, each class count on each: the case restates the launcher's predicate on the tensors it
    passes and asserts the kernels it was written for (the bounds: helpers.head_reference)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    f, phat, g, ref = _head_case(N, Ch, H, W, K)
    HW = H * W
    fd = _offset_view(f.cuda()) if offset else f.cuda()
    pd, gd = phat.cuda(), g.cuda()
    assert (fd.data_ptr() % 16 != 0) == offset
    assert hp.head_paths(Ch, HW, fd.data_ptr() % 16 == 0) == (fwd, bwd)
    if fwd == 'fwd4<8>':
        assert HW % 4 == 0 and Ch % 8 == 0
    elif fwd == 'fwd4<4>':
        assert HW % 4 == 0 and Ch % 4 == 0 and Ch % 8 != 0
    else:
        assert HW % 4 != 0 or Ch % 4 != 0 or fd.data_ptr() % 16 != 0
    assert (bwd == 'bwd4') == (HW % 4 == 0 and fd.data_ptr() % 16 == 0)
    logits, inv, dfeat = _run_head(fd, pd, gd)
    _check_head(ref, logits, dfeat, "%s/%s K=%d Ch=%d" % (fwd, bwd, K, Ch))
    hp.assert_within(1.0 / inv.double().cpu(), ref['n'], hp.rounding_bound((Ch + 2, ref['n'])), "norm")    # Ch fma steps, sqrt, 1/n
    logits2, inv2, dfeat2 = _run_head(fd, pd, gd)                                   # run-to-run identity
    assert torch.equal(logits, logits2) and torch.equal(inv, inv2) and torch.equal(dfeat, dfeat2)


@pytest.mark.parametrize("N,Ch,H,W,K,fwd,bwd", [c[:7] for c in hp.HEAD_CASES if not c[7] and (c[5] != 'fwd' or c[6] != 'bwd')])
def test_cosine_head_packed_and_scalar_kernels_agree_bitwise(N, Ch, H, W, K, fwd, bwd):
    """head.hip: the 4-pixel kernels do, per pixel, the same operations in the same order as the 1-pixel ones -- the same bits.
    The same data once aligned (4-pixel kernels) and once at an element offset of 1 (1-pixel kernels)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    f, phat, g, _ = _head_case(N, Ch, H, W, K)
    fa, pd, gd = f.cuda(), phat.cuda(), g.cuda()
    fo = _offset_view(fa)
    assert hp.head_paths(Ch, H * W, fa.data_ptr() % 16 == 0) == (fwd, bwd)
    assert hp.head_paths(Ch, H * W, fo.data_ptr() % 16 == 0) == ('fwd', 'bwd')
    packed, scalar = _run_head(fa, pd, gd), _run_head(fo, pd, gd)
    for name, a, b in zip(("logits", "inv_norm", "dfeat"), packed, scalar):
        assert torch.equal(a, b), "%s: %d elements differ between %s/%s and the 1-pixel kernels" % (name, int((a != b).sum()), fwd, bwd)


@pytest.mark.parametrize("N,Ch,K,H,W", [(2, 256, 20, 24, 40), (1, 64, 19, 9, 13), (3, 32, 21, 16, 16)])
def test_cosine_head_matches_pytorch(N, Ch, K, H, W):
    """The wrapper: logits and proxy gradient against F.normalize + conv2d in float64; the feature gradient against the kernel's
    formula with the unit proxies the wrapper hands to the kernel."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    g = torch.Generator().manual_seed(N * 10 + K)
    f = torch.randn((N, Ch, H, W), generator=g)
    f[0, :, 0, 0] = 0.0                                   # a zero feature vector: logits 0, finite gradients
    proxy = torch.randn((K, Ch, 1, 1), generator=g)
    go = torch.randn((N, K, H, W), generator=g)
    fd, pd = f.cuda().requires_grad_(True), proxy.cuda().requires_grad_(True)
    assert ops.cosine_head_supported(fd, pd)
    out = ops.cosine_head(fd, pd)
    out.backward(go.cuda())
    fr, pr = f.double().requires_grad_(True), proxy.double().requires_grad_(True)
    ref = F.conv2d(F.normalize(fr), F.normalize(pr, dim=1))
    ref.backward(go.double())
    assert float((out.detach().double().cpu() - ref.detach()).abs().max()) < 2e-6
    assert float(out[0, :, 0, 0].abs().max()) == 0.0
    phat = F.normalize(pd.detach(), dim=1).reshape(K, Ch).cpu()          # the wrapper's own operation: the kernel's float32 operand
    _check_head(hp.head_reference(f, phat, go), out.detach(), fd.grad, "wrapper")
    assert float((pd.grad.double().cpu() - pr.grad).abs().max()) < 2e-4 * max(1.0, float(pr.grad.abs().max()))


def test_model_parity_with_cosine_head_kernel():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from test_model import _check, _load
    g, net, x = _load()
    _check(g, net.cuda(), x.cuda(), 1e-4)


# ---- mas_dense_small_fwd / _bwd ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_case(N, K, M):
    x, w, dy = hp.dense_inputs(N, K, M)
    return x, w, dy, hp.dense_reference(x, w, dy)


def _run_dense(x, w, dy, need_x=True, need_w=True):
    from mulactseg_amd import ops
    xd, wd = x.cuda().requires_grad_(need_x), w.cuda().requires_grad_(need_w)
    y = ops._DenseSmall.apply(xd, wd)
    y.backward(dy.cuda())
    return y.detach(), xd.grad, wd.grad


@pytest.mark.parametrize("N,K,M", hp.DENSE_CASES)
def test_dense_small_matches_float64(N, K, M):
    """k_dense_fwd / k_dense_bwd_x / k_dense_bwd_w against x w^T, dy w and dy^T x (the bounds: helpers.dense_reference): the unrolled
    loop and its tail (M = 256: no tail, 13: one trip and five, 7 and 1: tail only), K off the 64-lane stride, a last workgroup with
    idle waves (N M = 39), K across two workgroups of the backward kernels (300); the fixed order gives the same bits twice."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    x, w, dy, ref = _dense_case(N, K, M)
    y, dx, dw = _run_dense(x, w, dy)
    for name, got in (('y', y), ('dx', dx), ('dw', dw)):
        assert got.shape == ref[name].shape and torch.isfinite(got).all()
        hp.assert_within(got, ref[name], ref[name + '_bound'], "dense %s [%d,%d,%d]" % (name, N, K, M))
    y2, dx2, dw2 = _run_dense(x, w, dy)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2)


@pytest.mark.parametrize("N,K,M", hp.DENSE_CASES)
def test_dense_small_bwd_one_output(N, K, M):
    """dx only and dw only: the requested product has the bits of the full call, the other one is neither returned nor written."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import _lib, ops
    x, w, dy, ref = _dense_case(N, K, M)
    _, dx, dw = _run_dense(x, w, dy)
    _, dx_only, none_w = _run_dense(x, w, dy, need_w=False)
    _, none_x, dw_only = _run_dense(x, w, dy, need_x=False)
    assert none_w is None and none_x is None
    assert torch.equal(dx_only, dx) and torch.equal(dw_only, dw)
    # the C entry with a null pointer for the other product, beside sentinel-filled tensors of both shapes that are not passed
    xd, wd, gd = x.cuda(), w.cuda(), dy.cuda()
    for want in ('dx', 'dw'):
        out = torch.full((N, K) if want == 'dx' else (M, K), float('nan'), device='cuda')
        held = [torch.full(s, -7.0, device='cuda') for s in ((N, K), (M, K))]
        _lib.check(_lib.load().mas_dense_small_bwd(gd.data_ptr(), xd.data_ptr(), wd.data_ptr(), N, K, M, out.data_ptr() if want == 'dx' else None,
                                                   out.data_ptr() if want == 'dw' else None, ops._stream(xd)), "mas_dense_small_bwd")
        torch.cuda.synchronize()
        assert torch.equal(out, dx if want == 'dx' else dw)
        assert all(bool((h == -7.0).all()) for h in held)


def test_conv1x1_on_1x1_is_the_dense_kernel():
    """ops.conv1x1_on_1x1 through a Conv2d at the model's shape: bit for bit the direct call, values and gradients."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    N, K, M = 4, 2048, 256
    x, w, dy, ref = _dense_case(N, K, M)
    conv = nn.Conv2d(K, M, 1, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(w.cuda().reshape(M, K, 1, 1))
    xd = x.cuda().reshape(N, K, 1, 1).requires_grad_(True)
    assert ops.conv1x1_on_1x1_supported(conv, xd)
    y = ops.conv1x1_on_1x1(conv, xd)
    assert y.shape == (N, M, 1, 1)
    y.backward(dy.cuda().reshape(N, M, 1, 1))
    y0, dx0, dw0 = _run_dense(x, w, dy)
    assert torch.equal(y.detach().reshape(N, M), y0)
    assert torch.equal(xd.grad.reshape(N, K), dx0) and torch.equal(conv.weight.grad.reshape(M, K), dw0)
    hp.assert_within(y.detach().reshape(N, M), ref['y'], ref['y_bound'], "conv1x1_on_1x1")
