"""The rounding bounds of tests/helpers.py, proved without a GPU: for the inputs and shapes the GPU tests of csrc/head.hip and
csrc/conv1x1.hip use, a float32 evaluation in the kernels' operation order stays inside every element's bound of the float64
evaluation, and an evaluation that is wrong by 2^-18 of its own magnitude, or that loses one term, does not.

float32 fma is restated through float64: the product of two float32 numbers is exact in float64, so ``(a * b + c).float()`` rounds
a * b + c once to 53 bits and once to 24, which differs from the single rounding of the instruction only when the first lands exactly
on a float32 tie.  Every other operation is torch's own float32 one (IEEE, one kernel per operation: nothing is contracted, as in the
library, which is built with -ffp-contract=off)."""
import pytest
import torch

import helpers as hp

EPS32 = torch.tensor(1e-12, dtype=torch.float32)


def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


# ---- the kernels' arithmetic, restated ----------------------------------------------------------------------------------------------
def head_f32(f, phat, g, drop=False):
    """k_cosine_fwd + k_cosine_bwd per pixel.  drop: the dot products lose channel 0, the sum over classes of dfeat loses class 0."""
    N, Ch, H, W = f.shape
    K = phat.shape[0]
    ff, gg = f.reshape(N, Ch, H * W), g.reshape(N, K, H * W)
    ss, dot = torch.zeros((N, H * W)), torch.zeros((N, K, H * W))
    for c in range(Ch):
        ss = fma32(ff[:, c], ff[:, c], ss)
        if not (drop and c == 0):
            dot = fma32(ff[:, c, None], phat[None, :, c, None], dot)
    nrm = ss.sqrt()
    inv = 1.0 / torch.where(nrm < EPS32, EPS32, nrm)
    logits = dot * inv[:, None]
    if drop:
        logits_used = head_f32(f, phat, g)[0].reshape(N, K, H * W)           # (dfeat's own lost term is judged on correct logits)
    else:
        logits_used = logits
    s, a = torch.zeros((N, H * W)), torch.zeros((N, Ch, H * W))
    for k in range(K):
        s = fma32(gg[:, k], logits_used[:, k], s)
        if not (drop and k == 0):
            a = fma32(gg[:, k, None], phat[k][None, :, None], a)
    df = (a - (s * inv)[:, None] * ff) * inv[:, None]
    return logits.reshape(N, K, H, W), df.reshape(N, Ch, H, W)


def dense_f32(x, w, dy):
    (N, K), M = x.shape, w.shape[0]
    trips = (K + 63) // 64
    xp, wp = torch.zeros((N, trips * 64)), torch.zeros((M, trips * 64))         # (a lane past K adds nothing: fma(0, 0, a) == a)
    xp[:, :K], wp[:, :K] = x, w
    a = torch.zeros((N, M, 64))
    for t in range(trips):
        a = fma32(xp[:, None, t * 64:(t + 1) * 64], wp[None, :, t * 64:(t + 1) * 64], a)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ off]
    dx, dw = torch.zeros((N, K)), torch.zeros((M, K))
    for m in range(M):
        dx = fma32(dy[:, m, None], w[m][None], dx)
    for n in range(N):
        dw = fma32(dy[n][:, None], x[n][None], dw)
    return {'y': a[..., 0], 'dx': dx, 'dw': dw}


def bn_fold(bn, eps=1e-5):
    weight, bias, mean, var = bn
    scale = weight.double() * torch.rsqrt(var.double() + eps)
    return scale.float(), (bias.double() - mean.double() * scale).float()


def conv1x1_f32(x, w, scale, shift, res, relu):
    N, K, H, W = x.shape
    xx = x.reshape(N, K, H * W)
    a = torch.zeros((N, w.shape[0], H * W))
    for k in range(K):
        a = fma32(xx[:, k, None], w[None, :, k, None], a)
    if scale is not None:
        a = a * scale[None, :, None] + shift[None, :, None]
        if res is not None:
            a = a + res.reshape(N, -1, H * W)
        if relu:
            a = torch.where(a > 0, a, torch.zeros_like(a))
    return a.reshape(N, -1, H, W)


# ---- what every bound is asked --------------------------------------------------------------------------------------------------------
def perturbed(v):
    return v.double() + 2.0 ** -18 * v.double().abs()


def passes(got, ref, bound):
    return bool((hp.bound_ratio(got, ref, bound) <= 1.0).all())


def check(name, good, lossy, ref, bound, relative_detectable=True):
    assert torch.isfinite(bound).all() and torch.isfinite(ref).all()
    hp.assert_within(good, ref, bound, name)
    assert not passes(lossy, ref, bound), name + ": an evaluation that lost a term passed"
    assert passes(perturbed(good), ref, bound) != relative_detectable, name + ": +2^-18 of the value"


@pytest.mark.parametrize("N,Ch,H,W,K,fwd,bwd,offset", hp.HEAD_CASES)
def test_cosine_head_bounds(N, Ch, H, W, K, fwd, bwd, offset):
    f, phat, g = hp.head_inputs(N, Ch, H, W, K)
    assert hp.head_paths(Ch, H * W, not offset) == (fwd, bwd)                   # the table names the kernels its shapes select
    ref = hp.head_reference(f, phat, g)
    logits, df = head_f32(f, phat, g)
    bad_logits, bad_df = head_f32(f, phat, g, drop=True)
    check("logits", logits, bad_logits, ref['logits'], ref['logits_bound'])
    check("dfeat", df, bad_df, ref['dfeat'], ref['dfeat_bound'])
    z = ref['zero']
    assert int(z.sum()) == 2 and bool(z.reshape(N, -1)[0, 0]) and bool(z.reshape(N, -1)[N - 1, -1])
    zc = z[:, None].expand(N, Ch, H, W)
    assert float(logits[z[:, None].expand_as(logits)].abs().max()) == 0.0
    check("dfeat at |f| = 0", df[zc], bad_df[zc], ref['dfeat_zero'][zc], ref['dfeat_zero_bound'][zc])
    # the |f| ~ 1e-20 pixel takes the clamp and is judged with the others
    assert float(ref['n'][0].reshape(-1)[1]) == hp.COSINE_EPS and not bool(z[0].reshape(-1)[1])


@pytest.mark.parametrize("N,K,M", hp.DENSE_CASES)
def test_dense_small_bounds(N, K, M):
    x, w, dy = hp.dense_inputs(N, K, M)
    ref = hp.dense_reference(x, w, dy)
    good = dense_f32(x, w, dy)
    x0, dy_m0, dy_n0 = x.clone(), dy.clone(), dy.clone()
    x0[:, 0], dy_m0[:, 0], dy_n0[0] = 0.0, 0.0, 0.0                              # y loses k = 0, dx loses m = 0, dw loses n = 0
    lossy = {'y': dense_f32(x0, w, dy)['y'], 'dx': dense_f32(x, w, dy_m0)['dx'], 'dw': dense_f32(x, w, dy_n0)['dw']}
    # A >= |value|, so a bound of c >= 64 roundings (2^-18 = 64 * 2^-24) holds every relative error of 2^-18: the 256-step chain of dx
    # at the model's shape cannot see that one, by arithmetic; the shape's other two products and the lost term do
    detectable = {'y': True, 'dx': M < 64, 'dw': True}
    for name in ('y', 'dx', 'dw'):
        check(name, good[name], lossy[name], ref[name], ref[name + '_bound'], detectable[name])
    assert any(detectable.values())


@pytest.mark.parametrize("N,K,M,H,W,res,relu,epi", hp.CONV1X1_CASES)
def test_conv1x1_bounds(N, K, M, H, W, res, relu, epi):
    x, w, bn, r = hp.conv1x1_inputs(N, K, M, H, W, res)
    scale, shift = bn_fold(bn) if epi else (None, None)
    ref, bound = hp.conv1x1_reference(x, w, scale, shift, r, relu)
    x0 = x.clone()
    x0[:, 0] = 0.0
    check("conv1x1", conv1x1_f32(x, w, scale, shift, r, relu), conv1x1_f32(x0, w, scale, shift, r, relu), ref, bound)
    if epi:                                                                      # the epilogue's own terms
        check("conv1x1 without shift", conv1x1_f32(x, w, scale, shift, r, relu), conv1x1_f32(x, w, scale, torch.zeros_like(shift), r, relu),
              ref, bound)
