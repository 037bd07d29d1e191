"""csrc/upsample.hip against F.interpolate(bilinear, align_corners=False) computed on the CPU (float32 forward within
rounding; backward against the float64 adjoint), determinism of the backward, exact adjointness.

Second half: both kernels element by element against float64 combinations of the kernel's own float32 taps (tests/helpers.py:
upsample_reference, proved on the CPU by tests/test_kernel_bounds_cpu.py) on shapes that select every form of the launchers, each case
asserting the form it was written for."""
import functools

import pytest
import torch
import torch.nn.functional as F

import helpers as hp

pytestmark = pytest.mark.gpu

CASES = [(2, 5, 12, 12, 48, 48), (1, 20, 48, 96, 192, 384), (2, 3, 9, 13, 33, 37), (1, 4, 7, 5, 7, 5), (1, 2, 16, 16, 40, 90)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


@pytest.mark.parametrize("N,C,Hi,Wi,Ho,Wo", CASES)
def test_forward_and_backward(N, C, Hi, Wi, Ho, Wo):
    ops = _gpu()
    g = torch.Generator().manual_seed(Hi * 100 + Wo)
    x = torch.randn((N, C, Hi, Wi), generator=g)
    go = torch.randn((N, C, Ho, Wo), generator=g)
    xd = x.cuda().requires_grad_(True)
    assert ops.upsample_bilinear_supported(xd, (Ho, Wo))
    y = ops.upsample_bilinear(xd, (Ho, Wo))
    ref = F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=False)
    assert float((y.detach().cpu() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))
    y.backward(go.cuda())
    xr = x.double().requires_grad_(True)
    F.interpolate(xr, size=(Ho, Wo), mode='bilinear', align_corners=False).backward(go.double())
    assert float((xd.grad.double().cpu() - xr.grad).abs().max()) <= 1e-5 * max(1.0, float(xr.grad.abs().max()))
    first = xd.grad.clone()
    xd.grad = None
    ops.upsample_bilinear(xd, (Ho, Wo)).backward(go.cuda())
    assert torch.equal(first, xd.grad)                                   # no atomics: bit-identical from run to run
    # <U x, g> == <x, U^T g> (the gather is the adjoint of this forward, not of an approximation of it)
    lhs = float((y.detach().double() * go.cuda().double()).sum())
    rhs = float((xd.detach().double() * first.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs))


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and float64 references of one shape: made once, shared, never written to."""
    N, C, Hi, Wi, Ho, Wo = shape
    x, g = hp.upsample_inputs(*shape)
    return x, g, hp.upsample_reference(x, Ho, Wo), hp.upsample_backward_reference(g, Hi, Wi)


def _offset_view(t):
    """A contiguous copy of ``t`` one element into a larger buffer: its address is 4 modulo 16."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device='cuda')
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _run(ops, x, g, size):
    xd = x.cuda().requires_grad_(True)
    assert ops.upsample_bilinear_supported(xd, size)
    y = ops.upsample_bilinear(xd, size)
    y.backward(g)
    return y.detach(), xd.grad


@pytest.mark.parametrize("shape,expect", hp.UPSAMPLE_CASES)
def test_every_kernel_form_within_its_bound(shape, expect):
    """The x4 backward (k_upsample_bwd<true>) with interior and edge columns, the second block column of the forward, five block columns
    of the backward with a partial last one, the 769-crop relation Wo = 4 Wi - 3 with scalar stores, the tap limit Wo = 6 Wi and a
    fractional ratio next to it, one input pixel (i1 == i0 on every tap), the identity (bit-exact).  Forward: 4 roundings over
    sum w |v|; backward: candidate columns + contributing rows over sum w |g|."""
    ops = _gpu()
    N, C, Hi, Wi, Ho, Wo = shape
    x, g, (ref, bound), (gref, gbound) = _case(shape)
    gd = g.cuda()
    got = hp.upsample_paths(Hi, Wi, Ho, Wo, gy_aligned=gd.data_ptr() % 16 == 0)
    for key, val in expect.items():
        assert val is None or got[key] == val, (key, got[key])
    y, gx = _run(ops, x, gd, (Ho, Wo))
    what = "%dx%d -> %dx%d" % (Hi, Wi, Ho, Wo)
    hp.assert_within(y, ref, bound, "upsample forward " + what)
    hp.assert_within(gx, gref, gbound, "upsample backward " + what)
    if (Hi, Wi) == (Ho, Wo):
        assert torch.equal(y.cpu(), x) and torch.equal(gx.cpu(), g)              # weights 1 and 0 only
    y2, gx2 = _run(ops, x, gd, (Ho, Wo))
    assert torch.equal(y, y2) and torch.equal(gx, gx2)


@pytest.mark.parametrize("shape", [hp.UPSAMPLE_CASES[0][0], hp.UPSAMPLE_CASES[1][0]])
def test_x4_backward_has_the_bits_of_the_general_loop(shape):
    """upsample.hip on FAST4: "the same fmas in the same order".  The same gradient once 16-byte aligned (k_upsample_bwd<true>) and once as
    a contiguous view one element off (the launcher's alignment test fails: k_upsample_bwd<false>)."""
    ops = _gpu()
    N, C, Hi, Wi, Ho, Wo = shape
    x, g, _, (gref, gbound) = _case(shape)
    ga = g.cuda()
    go = _offset_view(ga)
    assert hp.upsample_paths(Hi, Wi, Ho, Wo, gy_aligned=ga.data_ptr() % 16 == 0)['fast4']
    assert not hp.upsample_paths(Hi, Wi, Ho, Wo, gy_aligned=go.data_ptr() % 16 == 0)['fast4']
    _, fast = _run(ops, x, ga, (Ho, Wo))
    _, general = _run(ops, x, go, (Ho, Wo))
    hp.assert_within(general, gref, gbound, "upsample backward, gy at +1")
    assert torch.equal(fast, general), "%d elements differ" % int((fast != general).sum())


def test_upsample_into_a_channel_slice():
    """ops.upsample_bilinear_into: one launch per picture into channels 2..4 of a [2,7,Ho,Wo] buffer -- the bits of upsample_bilinear,
    every other channel untouched."""
    ops = _gpu()
    shape = (2, 3, 5, 13, 17, 49)
    N, C, Hi, Wi, Ho, Wo = shape
    x, _ = hp.upsample_inputs(*shape)
    xd = x.cuda()
    buf = torch.full((N, 7, Ho, Wo), -7.0, device='cuda')
    out = ops.upsample_bilinear_into(xd, buf[:, 2:5])
    assert out.data_ptr() == buf[:, 2:5].data_ptr()
    assert torch.equal(buf[:, 2:5], ops.upsample_bilinear(xd, (Ho, Wo)))
    assert bool((buf[:, :2] == -7.0).all()) and bool((buf[:, 5:] == -7.0).all())
    ref, bound = hp.upsample_reference(x, Ho, Wo)
    hp.assert_within(buf[:, 2:5], ref, bound, "upsample_bilinear_into")


def test_model_takes_the_hip_upsample_and_keeps_golden_parity():
    _gpu()
    from test_model import _check, _load
    g, net, x = _load()
    _check(g, net.cuda(), x.cuda(), 1e-4)
