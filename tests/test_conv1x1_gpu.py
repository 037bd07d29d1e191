"""csrc/conv1x1.hip: small-K 1x1 convolution, plain and with the inference BatchNorm + ReLU + residual epilogue,
against float64 PyTorch; the cached constants follow parameter updates; every tile of the launch map against a float64
evaluation within a worst-case float32 rounding bound (tests/helpers.py)."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import helpers as hp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,K,M,H,W,res", [(2, 128, 64, 24, 40, False), (1, 256, 64, 17, 12, True), (3, 8, 32, 6, 6, False)])
def test_conv1x1_bn_relu_matches_pytorch(N, K, M, H, W, res):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    g = torch.Generator().manual_seed(K + M)
    conv = nn.Conv2d(K, M, 1, bias=False)
    bn = nn.BatchNorm2d(M)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(M, generator=g) + 0.5); bn.bias.copy_(torch.randn(M, generator=g))
        bn.running_mean.copy_(torch.randn(M, generator=g)); bn.running_var.copy_(torch.rand(M, generator=g) + 0.3)
    x = torch.randn((N, K, H, W), generator=g)
    r = torch.randn((N, M, H, W), generator=g) if res else None
    conv.eval(); bn.eval()
    with torch.no_grad():
        ref = bn.double()(conv.double()(x.double()))
        if res:
            ref = ref + r.double()
        ref = F.relu(ref)
        conv, bn = conv.float().cuda(), bn.float().cuda()
        xd = x.cuda()
        assert ops.conv1x1_bn_act_supported(conv, bn, xd)
        y = ops.conv1x1_bn_act(conv, bn, xd, True, r.cuda() if res else None)
        assert float((y.double().cpu() - ref).abs().max()) < 1e-5 * max(1.0, float(ref.abs().max()))
        # constants are cached on the module and refreshed when a parameter changes
        conv.weight.mul_(0.5)
        y2 = ops.conv1x1_bn_act(conv, bn, xd, False, None)
        ref2 = bn(conv(xd))
        assert float((y2 - ref2).abs().max()) < 1e-4 * max(1.0, float(ref2.abs().max()))
    assert not ops.conv1x1_bn_act_supported(conv, bn.train(), xd)
    with torch.enable_grad():
        assert not ops.conv1x1_bn_act_supported(conv, bn.eval(), xd)


def test_model_parity_with_conv1x1_kernel():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from test_model import _check, _load
    g, net, x = _load()
    _check(g, net.cuda(), x.cuda(), 1e-4)


# ---- the launch map: pixel tile = q * 8 + xcd, output-channel tile = (bid >> 3) % mtiles ----------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(N, K, M, H, W, res):
    return hp.conv1x1_inputs(N, K, M, H, W, res)


def _raw(x, w_t, scale, shift, res, relu, M):
    """mas_conv1x1_fwd into an output filled with NaN: returns (status, y)."""
    from mulactseg_amd import _lib, ops
    N, K, H, W = x.shape
    y = torch.full((N, M, H, W), float('nan'), device='cuda')
    st = _lib.load().mas_conv1x1_fwd(x.data_ptr(), w_t.data_ptr(), N, K, M, H * W, ops._opt(scale), ops._opt(shift), ops._opt(res), int(relu),
                                     y.data_ptr(), ops._stream(x))
    torch.cuda.synchronize()
    return st, y


# what each case of helpers.CONV1X1_CASES is there for: (ptiles, mtiles, lanes of the last pixel tile that have pixels)
_TILES = [(2, 2, 104), (10, 1, 1), (8, 2, 256), (1, 1, 1), (2, 2, 104)]


@pytest.mark.parametrize("case,tiles", list(zip(hp.CONV1X1_CASES, _TILES)), ids=["-".join(str(v) for v in c) for c in hp.CONV1X1_CASES])
def test_conv1x1_every_tile_matches_float64(case, tiles):
    """Several pixel tiles, a second round of eight (ptiles 10: two live XCD slots, six that exit), exactly eight, a partly filled last
    tile, one live lane, two output-channel tiles with several pixel tiles, residual without ReLU, and the bare kernel.
    Bound (helpers.conv1x1_reference): K fma steps, * scale, + shift, + residual -> c = K + 3 (bare: K) over
    A = |scale| sum_k |x_k w_k| + |shift| + |res|.  The output starts as NaN: a tile the map skips leaves some behind."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import _lib, ops
    N, K, M, H, W, res, relu, epi = case
    HW = H * W
    assert HW % 4 == 0 and M % 32 == 0 and K % 4 == 0                                                   # the entry's own conditions
    assert (hp.conv1x1_tiles(M, HW) + ((HW - 1024 * (hp.conv1x1_tiles(M, HW)[0] - 1)) // 4,)) == tiles
    x, w, bnp, r = _case(N, K, M, H, W, res)
    xd, wd, rd = x.cuda(), w.cuda(), (r.cuda() if res else None)
    name = "conv1x1 [%d,%d,%d,%d] ptiles %d mtiles %d" % (N, K, M, HW, tiles[0], tiles[1])
    if not epi:
        assert not res and not relu
        st, y = _raw(xd, wd.t().contiguous(), None, None, None, 0, M)
        _lib.check(st, "mas_conv1x1_fwd")
        ref, bound = hp.conv1x1_reference(x, w, None, None, None, False)
        assert not torch.isnan(y).any()
        hp.assert_within(y, ref, bound, name + " bare")
        assert torch.equal(y, _raw(xd, wd.t().contiguous(), None, None, None, 0, M)[1])
        return
    conv, bn = nn.Conv2d(K, M, 1, bias=False), nn.BatchNorm2d(M)
    with torch.no_grad():
        conv.weight.copy_(w.reshape(M, K, 1, 1))
        for dst, src in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), bnp):
            dst.copy_(src)
        conv, bn = conv.cuda().eval(), bn.cuda().eval()
        assert ops.conv1x1_bn_act_supported(conv, bn, xd)
        y = ops.conv1x1_bn_act(conv, bn, xd, relu, rd)
        scale, shift = ops._bn_fold(bn)                              # the float32 constants the kernel reads
    assert y.shape == (N, M, H, W) and torch.isfinite(y).all()
    ref, bound = hp.conv1x1_reference(x, w, scale.cpu(), shift.cpu(), r, relu)
    hp.assert_within(y, ref, bound, name)
    if relu:
        assert float(y.min()) == 0.0 and float(y.max()) > 0.0
    else:
        assert float(y.min()) < 0.0
    st, y_raw = _raw(xd, wd.t().contiguous(), scale, shift, rd, relu, M)
    _lib.check(st, "mas_conv1x1_fwd")
    assert not torch.isnan(y_raw).any()                              # every output element is written
    assert torch.equal(y_raw, y)


def test_conv1x1_entry_checks_launch_nothing():
    """HW % 4, M % 32, K % 4 and scale without shift (or shift without scale): the documented codes, the output untouched."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    MAS_ERR_NULL, MAS_ERR_SHAPE = -1, -2
    x = torch.randn((1, 8, 4, 8), device='cuda')
    w_t = torch.randn((8, 64), device='cuda')
    s = torch.ones(64, device='cuda')

    def call(N, K, M, HW, scale, shift):
        from mulactseg_amd import _lib, ops
        y = torch.full((1, 64, 4, 8), float('nan'), device='cuda')
        st = _lib.load().mas_conv1x1_fwd(x.data_ptr(), w_t.data_ptr(), N, K, M, HW, ops._opt(scale), ops._opt(shift), None, 0, y.data_ptr(),
                                         ops._stream(x))
        torch.cuda.synchronize()
        assert torch.isnan(y).all()
        return st
    assert call(1, 8, 64, 30, s, s) == MAS_ERR_SHAPE
    assert call(1, 8, 48, 32, s, s) == MAS_ERR_SHAPE
    assert call(1, 6, 64, 32, s, s) == MAS_ERR_SHAPE
    assert call(1, 8, 64, 32, s, None) == MAS_ERR_NULL
    assert call(1, 8, 64, 32, None, s) == MAS_ERR_NULL
