"""The two ends of a ring-scan strip and the weighted finalize, against oracle/exact.c bit for bit.

k_single_pass_ring issues one row past the end of every wave's 16 rows (never consumed; its address must stay inside the
picture for every shape) and reduces the per-thread class accumulators of a strip in LDS; k_region_finalize_weighted reads
a region's row with a 16-lane row of a wave.  All outputs are integers or one rounding of an integer quotient, so every
comparison is equality."""

import functools

import numpy as np
import pytest
import torch

from mulactseg_amd import synth

pytestmark = pytest.mark.gpu

ID_DTYPES = (torch.int64, torch.int32, torch.int16)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _equal(got, want):
    ps, cs, hh = got
    eps_, ecs, eh = want
    return (np.array_equal(ps.cpu().numpy().view(np.uint64), eps_) and np.array_equal(cs.cpu().numpy().view(np.uint64), ecs)
            and np.array_equal(hh.cpu().numpy().view(np.uint32), eh))


# B, H, W, S: every one goes to the ring kernel (H >= 64, W % 4 == 0)
RING_SHAPES = [
    (1, 64, 256, 32),       # one strip: every wave's last trip is the dead one
    (1, 65, 256, 32),       # the second strip has one live row
    (2, 100, 516, 64),      # ragged last strip and a 4-pixel last tile column
    (1, 128, 64, 16),       # narrower than a tile: whole lanes masked
    (3, 192, 256, 48),      # three pictures: the per-picture class sums must not mix
]


@functools.lru_cache(maxsize=None)
def _ring_case(B, C, H, W, S):
    from oracle import exact
    z = synth.logits(900 + C + H, B, C, H, W)
    spx = np.stack([synth.superpixel_map(77 * H + i, H, W, S) for i in range(B)])
    invT = np.float32(1.0) / np.float32(0.1)
    return z, spx, exact.single_pass_accum(z, spx, S, invT)


@pytest.mark.parametrize("C", [19, 20, 21])
@pytest.mark.parametrize("B,H,W,S", RING_SHAPES)
def test_ring_shapes_bit_exact(B, H, W, S, C):
    ops = _gpu()
    z, spx, want = _ring_case(B, C, H, W, S)
    zt = torch.from_numpy(z).cuda()
    for dtype in ID_DTYPES:
        got = ops.single_pass_accum(zt, torch.from_numpy(spx).to(dtype).cuda(), S, ops.inv_temperature(0.1))
        assert _equal(got, want), dtype


@pytest.mark.parametrize("kind", ["one_class_far_ahead", "all_equal"])
def test_saturated_accumulators(kind):
    """The largest sums the strip epilogue sees: 2^23 quanta per pixel in ONE class (a thread's word reaches 64 * 2^23, a
    strip's class total 2^37), and the same quanta spread evenly over all classes."""
    ops = _gpu()
    from oracle import exact
    B, C, H, W, S = 2, 20, 128, 512, 32
    z = np.zeros((B, C, H, W), dtype=np.float32)
    if kind == "one_class_far_ahead":
        z[0, 3] = 50.0
        z[1, C - 1] = 50.0
    spx = np.stack([synth.superpixel_map(5 + i, H, W, S) for i in range(B)])
    invT = ops.inv_temperature(0.1)
    want = exact.single_pass_accum(z, spx, S, np.float32(invT))
    if kind == "one_class_far_ahead":
        assert int(want[0][0, 3]) == H * W << 23 and int(want[0][1, C - 1]) == H * W << 23
    zt = torch.from_numpy(z).cuda()
    for dtype in ID_DTYPES:
        assert _equal(ops.single_pass_accum(zt, torch.from_numpy(spx).to(dtype).cuda(), S, invT), want), dtype


def test_second_call_doubles_all_three_outputs():
    ops = _gpu()
    B, C, H, W, S = 2, 20, 100, 516, 64
    z, spx, want = _ring_case(B, C, H, W, S)
    zt, st = torch.from_numpy(z).cuda(), torch.from_numpy(spx).cuda()
    invT = ops.inv_temperature(0.1)
    ps, cs, hh = ops.single_pass_accum(zt, st, S, invT)
    assert _equal((ps, cs, hh), want)
    ps2, cs2, hh2 = ops.single_pass_accum(zt, st, S, invT, prob_sum=ps.clone(), class_sum=cs.clone(), hist=hh.clone())
    assert torch.equal(ps2, 2 * ps) and torch.equal(cs2, 2 * cs) and torch.equal(hh2, 2 * hh)


@pytest.mark.parametrize("H,W", [(64, 256), (100, 516)])
def test_last_picture_of_an_allocation(H, W):
    """z and spx are the LAST picture of their allocations: the views end where the storage ends, so an address behind
    the picture is an address outside the tensor."""
    ops = _gpu()
    C, S = 20, 32
    z, spx, want = _ring_case(1, C, H, W, S)
    invT = ops.inv_temperature(0.1)
    zall = torch.full((3, C, H, W), float('nan'), dtype=torch.float32, device='cuda')
    zall[2] = torch.from_numpy(z[0]).cuda()
    zt = zall.narrow(0, 2, 1)
    assert zt.is_contiguous() and zt.data_ptr() + zt.numel() * 4 == zall.data_ptr() + zall.numel() * 4
    for dtype in ID_DTYPES:
        sall = torch.full((3, H, W), -1, dtype=dtype, device='cuda')
        sall[2] = torch.from_numpy(spx[0]).to(dtype).cuda()
        st = sall.narrow(0, 2, 1)
        assert st.is_contiguous() and st.data_ptr() + st.numel() * st.element_size() == sall.data_ptr() + sall.numel() * sall.element_size()
        assert _equal(ops.single_pass_accum(zt, st, S, invT), want), dtype


def _finalize_inputs(n, C, seed):
    """Small counts (ties for the dominant class, the lowest index wins), a third of the regions empty, sums of up to 2^40 per
    pixel, and non-zero sums under zero counts (they must not count)."""
    rs = np.random.RandomState(seed)
    hist = rs.randint(0, 4, size=(n, C)).astype(np.uint32)
    hist[rs.rand(n, C) < 0.1] = 70000
    hist[rs.rand(n) < 0.33] = 0
    cs = hist.astype(np.uint64) * rs.randint(1, 1 << 40, size=(n, C), dtype=np.int64).astype(np.uint64)
    stray = (hist == 0) & (rs.rand(n, C) < 0.25)
    cs[stray] = rs.randint(1, 1 << 62, size=int(stray.sum()), dtype=np.int64).astype(np.uint64)
    w = rs.uniform(0.2, 1.9, size=C).astype(np.float32)
    return cs, hist, w


@pytest.mark.parametrize("want_hist_i64", [False, True])
@pytest.mark.parametrize("C", [1, 7, 19, 20, 21, 32])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_finalize_weighted_bit_exact(n, C, want_hist_i64):
    ops = _gpu()
    from oracle import exact
    cs, hist, w = _finalize_inputs(n, C, 1000 * C + n)
    w31 = ops.weights_to_fixed31(w)
    dom_ref = exact.region_finalize_weighted(cs, hist, w31, -1)[1]
    ban = int(np.bincount(dom_ref.ravel(), minlength=C).argmax())       # the class that dominates most regions is banned
    cst, ht = torch.from_numpy(cs.view(np.int64)).cuda(), torch.from_numpy(hist.view(np.int32)).cuda()
    w31t = torch.from_numpy(w31.view(np.int32)).cuda()
    for ban_class in (ban, -1):
        escore, edom, ecnt = exact.region_finalize_weighted(cs, hist, w31, ban_class)
        if ban_class >= 0:
            assert (edom == ban_class).any() and (escore[edom == ban_class] == 0).all()
        score, dom, cnt, h64 = ops.region_finalize_weighted(cst, ht, w31t, ban_class, want_hist_i64)
        assert np.array_equal(score.cpu().numpy(), escore)
        assert np.array_equal(dom.cpu().numpy(), edom)
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), ecnt)
        assert (h64 is not None) == want_hist_i64
        if want_hist_i64:
            assert np.array_equal(h64.cpu().numpy(), hist.astype(np.int64))


def test_finalize_weighted_even_classes_on_8_byte_aligned_sums():
    """An even class count whose class sums start 8 bytes into a 16-byte unit: the two-class vector loads do not apply."""
    ops = _gpu()
    from oracle import exact
    n, C = 300, 20
    cs, hist, w = _finalize_inputs(n, C, 7)
    w31 = ops.weights_to_fixed31(w)
    store = torch.zeros(n * C + 1, dtype=torch.int64, device='cuda')
    cst = store[1:].view(n, C)
    cst.copy_(torch.from_numpy(cs.view(np.int64)))
    assert cst.is_contiguous() and cst.data_ptr() % 16 == 8
    score, dom, cnt, h64 = ops.region_finalize_weighted(cst, torch.from_numpy(hist.view(np.int32)).cuda(),
                                                        torch.from_numpy(w31.view(np.int32)).cuda(), 3, True)
    escore, edom, ecnt = exact.region_finalize_weighted(cs, hist, w31, 3)
    assert np.array_equal(score.cpu().numpy(), escore) and np.array_equal(dom.cpu().numpy(), edom)
    assert np.array_equal(cnt.cpu().numpy().view(np.uint32), ecnt) and np.array_equal(h64.cpu().numpy(), hist.astype(np.int64))
