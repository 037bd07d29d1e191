"""The rounding bounds of tests/helpers.py, proved without a GPU: for the inputs and shapes the GPU tests of csrc/head.hip,
csrc/conv1x1.hip, csrc/bn.hip and csrc/upsample.hip use, a float32 evaluation in the kernels' operation order stays inside every
element's bound of the float64 evaluation, and an evaluation that is wrong by 2^-18 of its own magnitude, or that loses one term, does
not.  Where a bound cannot see a fault by arithmetic, the test says so and names the check that does.

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


# ---- csrc/bn.hip restated in float32, in the kernels' order ------------------------------------------------------------------------------
def _plane_groups(t, n, c, a, ngroups, fill=0.0):
    """Plane (n, c) of t laid out in the aligned groups of four the kernels walk: [ngroups, 4], `fill` outside the plane."""
    HW = t.shape[2] * t.shape[3]
    buf = torch.full((4 * ngroups,), fill, dtype=t.dtype)
    buf[a:a + HW] = t[n, c].reshape(-1)
    return buf.view(ngroups, 4)


def _pad_trips(g):
    """[k, 4] -> [trips, 256, 4]: thread t of a chunk takes groups t, t + 256, ... (zero groups add nothing: s + 0 == s)."""
    trips = (g.shape[0] + hp.BN_THREADS - 1) // hp.BN_THREADS
    out = torch.zeros((trips * hp.BN_THREADS, 4), dtype=g.dtype)
    out[:g.shape[0]] = g
    return out.view(trips, hp.BN_THREADS, 4)


def bn_stats_f32(x, eps, momentum, rm0, rv0, drop=False, biased=False):
    """k_bn_partial + k_bn_stats.  drop: every chunk stops one group short.  biased: the running variance divides by n, not n - 1."""
    N, C, H, W = x.shape
    HW, n = H * W, N * H * W
    chunks = hp.bn_chunks(HW)
    S, Q = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for c in range(C):
        for b in range(N):
            a = ((b * C + c) * HW) & 3
            ngroups, per_chunk = hp.bn_plane_groups(a, HW, chunks)
            grp = _plane_groups(x, b, c, a, ngroups)
            for lo, hi, _, _ in per_chunk:
                hi = hi - 1 if (drop and hi > lo) else hi
                s, q = torch.zeros(hp.BN_THREADS), torch.zeros(hp.BN_THREADS)
                for v in _pad_trips(grp[lo:hi]):
                    s = s + ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3]))
                    q = q + ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + (v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3]))
                S[c] += s.double().sum()
                Q[c] += q.double().sum()
    m = S / n
    var = (Q / n - m * m).clamp_min(0.0)
    mom = hp.f32_as_float(momentum)
    unb = var if (biased or n == 1) else var * n / (n - 1.0)
    return dict(mean=m.float(), invstd=(var + hp.f32_as_float(eps)).rsqrt().float(),
                rm=((1.0 - mom) * rm0.double() + mom * m).float(), rv=((1.0 - mom) * rv0.double() + mom * unb).float())


def bn_apply_f32(x, gamma, beta, res, mean, invstd, relu):
    v = lambda t: t.view(1, -1, 1, 1)
    t = ((x - v(mean)) * v(invstd)) * v(gamma) + v(beta)
    t = t + res
    return torch.where(t > 0, t, torch.zeros_like(t)) if relu else t


def swap_mask_bits(gate):
    """The ReLU mask of every aligned group with bits 1 and 2 exchanged (planes at their addresses in a 16-byte aligned tensor;
    a bit that belongs to no element of the plane reads 0)."""
    N, C, H, W = gate.shape
    HW, out = H * W, torch.empty_like(gate)
    for b in range(N):
        for c in range(C):
            a = ((b * C + c) * HW) & 3
            ngroups = (a + HW + 3) >> 2
            grp = _plane_groups(gate, b, c, a, ngroups)[:, [0, 2, 1, 3]].reshape(-1)
            out[b, c] = grp[a:a + HW].view(H, W)
    return out


def bn_bwd_f32(x, dy, gate, gamma, mean, invstd, drop=False):
    """k_bn_bwd_partial<VEC> + k_bn_bwd_stats + k_bn_bwd_apply: thread t of a chunk adds the whole groups flo + t, flo + t + 256, ... element
    by element, then the plane's boundary groups that fall into the chunk (thread (i - lo) % 256).  gate: [y > 0] as 0 / 1.
    (The element-wise form of the launch, VEC false, walks the groups from lo instead of flo: another partition of the same
    additions, no longer a chain; the bounds hold for both.)"""
    N, C, H, W = x.shape
    HW, n = H * W, N * H * W
    chunks = hp.bn_chunks(HW)
    g = dy * gate
    St, Qt = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    lane = torch.arange(hp.BN_THREADS)
    for c in range(C):
        mu, inv = mean[c], invstd[c]
        for b in range(N):
            a = ((b * C + c) * HW) & 3
            ngroups, per_chunk = hp.bn_plane_groups(a, HW, chunks)
            gg, xg = _plane_groups(g, b, c, a, ngroups), _plane_groups(x, b, c, a, ngroups, float(mu))
            for lo, hi, flo, fhi in per_chunk:
                if drop and hi > lo:
                    hi -= 1
                    fhi = max(flo, min(fhi, hi))
                s, q = torch.zeros(hp.BN_THREADS), torch.zeros(hp.BN_THREADS)
                for gv, xv in zip(_pad_trips(gg[flo:fhi]), _pad_trips(xg[flo:fhi])):
                    for k in range(4):
                        s = s + gv[:, k]
                        q = q + gv[:, k] * ((xv[:, k] - mu) * inv)
                for i in [j for j in range(lo, hi) if not (flo <= j < fhi)]:
                    t = (i - lo) % hp.BN_THREADS
                    for k in range(4):
                        s = torch.where(lane == t, s + gg[i, k], s)
                        q = torch.where(lane == t, q + gg[i, k] * ((xg[i, k] - mu) * inv), q)
                St[c] += s.double().sum()
                Qt[c] += q.double().sum()
    v = lambda t: t.view(1, -1, 1, 1)
    k, mg, mgx = gamma * invstd, (St / n).float(), (Qt / n).float()
    dx = v(k) * ((g - v(mg)) - ((x - v(mean)) * v(invstd)) * v(mgx))
    return dict(dres=g, dbeta=St.float(), dgamma=Qt.float(), dx=dx)


@pytest.mark.parametrize("shape,expect", hp.BN_CASES)
def test_batchnorm_bounds(shape, expect):
    """Every bound of helpers.bn_*_reference on the case table of test_bn_gpu.py: the float32 restatement passes; a chunk that stops one
    group short fails the mean, the running mean, dbeta and dgamma on every case (a group that is lost holds at least one element of the
    plane; the error is that element over the count against 10 roundings of mean|x|); exchanged mask bits fail the exact dres; a running
    variance divided by n fails; y without beta fails."""
    N, C, H, W = shape
    got = hp.bn_paths(N, C, H * W)
    assert got.pop('per_thread') <= 8
    assert got == expect                                                         # the table names what its shapes reach
    t = hp.bn_inputs(N, C, H, W)
    x, res, dy, gamma, beta = t['x'], t['res'], t['dy'], t['gamma'], t['beta']
    ref = hp.bn_stats_reference(x, 1e-5, 0.1, t['rm'], t['rv'])
    good = bn_stats_f32(x, 1e-5, 0.1, t['rm'], t['rv'])
    lossy = bn_stats_f32(x, 1e-5, 0.1, t['rm'], t['rv'], drop=True)
    for name in ('mean', 'invstd', 'rm', 'rv'):
        hp.assert_within(good[name], ref[name], ref[name + '_bound'], name)
    assert not passes(lossy['mean'], ref['mean'], ref['mean_bound']) and not passes(lossy['rm'], ref['rm'], ref['rm_bound'])
    assert not passes(lossy['invstd'], ref['invstd'], ref['invstd_bound'])       # (mean / std = 0.25: well conditioned; see below)
    biased = bn_stats_f32(x, 1e-5, 0.1, t['rm'], t['rv'], biased=True)
    assert not passes(biased['rv'], ref['rv'], ref['rv_bound'])
    # (b): the statistics of the float32 run are the given ones, as the device's are on the GPU
    mean, invstd = good['mean'], good['invstd']
    y = bn_apply_f32(x, gamma, beta, res, mean, invstd, True)
    yr, yb = hp.bn_apply_reference(x, gamma, beta, res, mean, invstd, True)
    check("y", y, bn_apply_f32(x, gamma, torch.zeros_like(beta), res, mean, invstd, True), yr, yb)
    assert bool((y >= 0).all()) and not bool(torch.signbit(y).any())
    gate = (y > 0).float()
    bref = hp.bn_backward_reference(x, dy, y, gamma, mean, invstd, True)
    out = bn_bwd_f32(x, dy, gate, gamma, mean, invstd)
    bad = bn_bwd_f32(x, dy, gate, gamma, mean, invstd, drop=True)
    assert torch.equal(out['dres'], bref['dres'])
    for name in ('dbeta', 'dgamma', 'dx'):
        hp.assert_within(out[name], bref[name], bref[name + '_bound'], name)
        assert not passes(bad[name], bref[name], bref[name + '_bound']), name + ": a chunk one group short passed"
    swapped = bn_bwd_f32(x, dy, swap_mask_bits(gate), gamma, mean, invstd)
    assert not torch.equal(swapped['dres'], bref['dres'])


def test_batchnorm_inference_bound():
    """k_bn_apply<FROM_VAR>: 1 / sqrtf(var + eps) in float32, then the same chain."""
    t = hp.bn_inputs(3, 5, 33, 37)
    is32 = 1.0 / torch.sqrt(t['rv'] + torch.tensor(1e-5, dtype=torch.float32))
    for relu in (True, False):
        yr, yb = hp.bn_apply_reference(t['x'], t['gamma'], t['beta'], t['res'], t['rm'], t['rv'], relu, eps=1e-5)
        check("inference y", bn_apply_f32(t['x'], t['gamma'], t['beta'], t['res'], t['rm'], is32, relu),
              bn_apply_f32(t['x'], t['gamma'], t['beta'], torch.zeros_like(t['res']), t['rm'], is32, relu), yr, yb)


def test_batchnorm_conditioning_bound():
    """The one-pass variance Q / n - m^2: the bound on invstd grows with (mean / std)^2, and so does what it can no longer see.  One
    element of 2442 read 1.0 too large moves the variance by (2 d + 1) / n ~ 1e-3 of itself (d its distance from the mean): the invstd
    bound catches that at mean / std of 0, 1 and 8, and by arithmetic cannot at 64, where dvar / var ~ 31 * 2^-24 * 64^2 = 8e-3.  There
    the mean carries the detection: its bound is 10 roundings of mean|x| (4e-5 at 64) against 1 / n = 4e-4, on every channel.  (A whole
    lost group moves the mean by 0.1 at 64 and is seen by both.)"""
    x = hp.bn_conditioning_input()
    z = torch.zeros(4)
    ref = hp.bn_stats_reference(x, 1e-5, 0.1, z, z + 1)
    good = bn_stats_f32(x, 1e-5, 0.1, z, z + 1)
    off = x.clone()
    off[0, :, 0, 0] += 1.0
    lossy = bn_stats_f32(off, 1e-5, 0.1, z, z + 1)
    assert not passes(bn_stats_f32(x, 1e-5, 0.1, z, z + 1, drop=True)['invstd'][3:], ref['invstd'][3:], ref['invstd_bound'][3:])
    for name in ('mean', 'invstd', 'rm', 'rv'):
        hp.assert_within(good[name], ref[name], ref[name + '_bound'], name)
    rel = ((good['invstd'].double() - ref['invstd']) / ref['invstd']).abs()
    print("relative invstd error at mean/std 0, 1, 8, 64:", ["%.2e" % float(v) for v in rel],
          " bound:", ["%.2e" % float(v) for v in ref['invstd_bound'] / ref['invstd']])
    seen = hp.bound_ratio(lossy['invstd'], ref['invstd'], ref['invstd_bound']) > 1.0
    assert seen.tolist() == [True, True, True, False]
    assert bool((hp.bound_ratio(lossy['mean'], ref['mean'], ref['mean_bound']) > 1.0).all())


def test_batchnorm_formulas_are_batchnorm():
    """The restated formulas, run with float64 statistics, against torch.nn.BatchNorm2d autograd in float64: the restatement of
    helpers.bn_apply_reference / bn_backward_reference is BatchNorm + residual + ReLU, to 1e-12."""
    N, C, H, W = 3, 5, 33, 37
    EPS, MOM = 2.0 ** -17, 0.125                # (float32 numbers: the references take eps and momentum as the C floats the kernels receive)
    t = hp.bn_inputs(N, C, H, W)
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double().train()
    with torch.no_grad():
        bn.weight.copy_(t['gamma']); bn.bias.copy_(t['beta']); bn.running_mean.copy_(t['rm']); bn.running_var.copy_(t['rv'])
    xr, rr = t['x'].double().requires_grad_(True), t['res'].double().requires_grad_(True)
    yt = torch.relu(bn(xr) + rr)
    yt.backward(t['dy'].double())
    st = hp.bn_stats_reference(t['x'], EPS, MOM, t['rm'], t['rv'])
    yr, _ = hp.bn_apply_reference(t['x'], t['gamma'], t['beta'], t['res'], st['mean'], st['invstd'], True)
    ref = hp.bn_backward_reference(t['x'], t['dy'], yr, t['gamma'], st['mean'], st['invstd'], True)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(yr, yt.detach()) and close(ref['dx'], xr.grad) and close(ref['dres'].double(), rr.grad)
    assert close(ref['dgamma'], bn.weight.grad) and close(ref['dbeta'], bn.bias.grad)
    assert close(st['rm'], bn.running_mean) and close(st['rv'], bn.running_var)


# ---- csrc/upsample.hip restated in float32 ---------------------------------------------------------------------------------------------
def upsample_fwd_f32(x, Ho, Wo, drop=False):
    """k_upsample_fwd.  drop: the l1w * v01 / l1w * v11 taps are lost."""
    Hi, Wi = x.shape[2:]
    j0, j1, m0, m1 = hp.upsample_taps(Hi, Ho)
    i0, i1, l0, l1 = hp.upsample_taps(Wi, Wo)
    if drop:
        l1 = torch.zeros_like(l1)
    r0, r1 = x[:, :, j0], x[:, :, j1]
    top = l0 * r0[..., i0] + l1 * r0[..., i1]
    bot = l0 * r1[..., i0] + l1 * r1[..., i1]
    return m0[:, None] * top + m1[:, None] * bot


def upsample_bwd_f32(g, Hi, Wi, drop=False):
    """k_upsample_bwd: per input pixel the row sums by fma over the output columns in ascending order, then fma over the rows (a zero
    weight leaves the sum as it is: fma(0, g, s) == s, so the x4 form and the tested loop are one chain).  drop: every input column
    loses its last weighted output column (wx[9] of the x4 form)."""
    Ho, Wo = g.shape[2:]
    wy, wx = hp.upsample_weights(Hi, Ho, torch.float32), hp.upsample_weights(Wi, Wo, torch.float32)
    if drop:
        wx = wx.clone()
        last = (wx != 0).float().mul(torch.arange(Wo)[:, None] + 1.0).argmax(0)
        wx[last, torch.arange(Wi)] = 0.0
    row = torch.zeros(g.shape[:3] + (Wi,))
    for ox in range(Wo):
        row = fma32(wx[ox], g[..., ox, None], row)
    acc = torch.zeros(g.shape[:2] + (Hi, Wi))
    for oy in range(Ho):
        acc = fma32(wy[oy][:, None], row[:, :, oy, None, :], acc)
    return acc


@pytest.mark.parametrize("shape,expect", hp.UPSAMPLE_CASES)
def test_upsample_bounds(shape, expect):
    """helpers.upsample_reference / upsample_backward_reference on the case table of test_upsample_gpu.py: the float32 restatement
    passes, a lost class of taps fails, forward and backward, at every shape.  (The identity has weights 1 and 0 only: l1 = 0, the
    forward loses nothing with it -- exactness is what that case is for -- and its backward loses the one weight it has.)"""
    N, C, Hi, Wi, Ho, Wo = shape
    got = hp.upsample_paths(Hi, Wi, Ho, Wo)
    for key, val in expect.items():
        assert val is None or got[key] == val, (key, got[key])
    x, g = hp.upsample_inputs(*shape)
    ref, bound = hp.upsample_reference(x, Ho, Wo)
    y = upsample_fwd_f32(x, Ho, Wo)
    identity = (Hi, Wi) == (Ho, Wo)
    if identity:
        assert torch.equal(y, x)
        hp.assert_within(y, ref, bound, "upsample forward")
    elif expect['single']:
        # one input pixel: l0 v + l1 v with l0 + l1 = 1; without l1 the result is l0 v, off by l1 |v| wherever l1 > 0 -- but every tap is
        # clamped to s = 0 or has i1 == i0 with l1 of any size: the lost term is judged where it is not 0
        hp.assert_within(y, ref, bound, "upsample forward")
        assert not passes(upsample_fwd_f32(x, Ho, Wo, drop=True), ref, bound)
    else:
        check("upsample forward", y, upsample_fwd_f32(x, Ho, Wo, drop=True), ref, bound)
    gref, gbound = hp.upsample_backward_reference(g, Hi, Wi)
    good, lossy = upsample_bwd_f32(g, Hi, Wi), upsample_bwd_f32(g, Hi, Wi, drop=True)
    if expect['single']:
        # one sum of fifteen gradients of both signs per plane: sum |g| is many times |sum g|, a relative 2^-18 of the result is
        # below the bound by arithmetic; the lost column is not
        hp.assert_within(good, gref, gbound, "upsample backward")
        assert not passes(lossy, gref, gbound)
    else:
        check("upsample backward", good, lossy, gref, gbound)
    # <U x, g> == <x, U^T g> in float64: the two references are adjoint
    assert abs(float((ref * g.double()).sum()) - float((x.double() * gref).sum())) <= 2.0 ** -22 * float((ref * g.double()).abs().sum())
