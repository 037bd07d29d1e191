"""Acquisition measures beyond BvSB on the device (csrc/uncertainty.hip): the kernel against the library's host entry bit for bit,
measure = bvsb against the headline scan's kernels, the low-resolution form against the materialised tensor, and the six selectors
on HipBackend against the CPU stand-in of tests/test_uncertainty_cpu.py."""
import types

import numpy as np
import pytest
import torch

from helpers import fake_trainer
from test_uncertainty_cpu import MEASURES, NEW_MEASURES, SELECTORS, cpu_round, make_selector, run_round, tiny_pool

pytestmark = pytest.mark.gpu
DTYPES = (torch.int64, torch.int32, torch.int16)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def ops():
    from mulactseg_amd import ops as o
    return o


def case(seed, B, C, H, W, S, dtype=torch.int64, scale=0.4):
    """Seeded logits and ids in [-1, S] (u16: [0, S]) with id S - 1 unused."""
    rs = np.random.RandomState(seed)
    z = torch.from_numpy((rs.randn(B, C, H, W) * scale).astype(np.float32))
    ids = rs.randint(-1, S - 1, (B, H, W))
    ids[:, H // 2, :] = S
    if dtype == torch.int16:
        ids[ids < 0] = 0
    return z, torch.from_numpy(ids).to(dtype)


def same(got, want):
    return all(torch.equal(g.cpu(), w.cpu()) for g, w in zip(got, want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [2, 19, 21, 32])
def test_kernel_equals_the_host_entry_bit_for_bit(C, dtype):
    _need_gpu()
    B, H, W, S = 2, 37, 53, 7
    z, spx = case(10 + C, B, C, H, W, S, dtype)
    invT = ops().inv_temperature(0.1)
    for m in MEASURES:
        want = ops().uncertainty_reference(z, spx, S, invT, m)
        got = ops().uncertainty_accum(z.cuda(), spx.cuda(), S, invT, m)
        assert same(got, want), m
        assert int(want[2][:, S - 1].sum()) == 0 and int(want[2].sum()) < B * H * W       # an unused id; skipped ids
        again = ops().uncertainty_accum(z.cuda(), spx.cuda(), S, invT, m, *got)             # += into the caller's buffers
        assert same(again, [2 * t for t in want]), m


def test_kernel_equals_the_host_entry_across_column_tiles():
    """A picture wider than one 256-column tile and taller than one 16-row tile, with an odd width."""
    _need_gpu()
    z, spx = case(3, 1, 20, 19, 301, 9)
    for m in MEASURES:
        assert same(ops().uncertainty_accum(z.cuda(), spx.cuda(), 9, 10.0, m), ops().uncertainty_reference(z, spx, 9, 10.0, m)), m


@pytest.mark.parametrize("C", [2, 19, 20, 21, 32])
def test_bvsb_measure_equals_the_headline_scan_full_resolution(C):
    """The yardstick that is not the code under test: mas_single_pass_accum."""
    _need_gpu()
    z, spx = case(40 + C, 2, C, 37, 53, 7)
    invT = ops().inv_temperature(0.1)
    ps, cs, hh = ops().single_pass_accum(z.cuda(), spx.cuda(), 7, invT)
    assert same(ops().uncertainty_accum(z.cuda(), spx.cuda(), 7, invT, 'bvsb'), (ps, cs, hh))
    for m in NEW_MEASURES:
        p2, c2, h2 = ops().uncertainty_accum(z.cuda(), spx.cuda(), 7, invT, m)
        assert torch.equal(p2, ps) and torch.equal(h2, hh) and not torch.equal(c2, cs), m


@pytest.mark.parametrize("C", [19, 20, 21])
def test_bvsb_measure_equals_the_headline_scan_low_resolution(C):
    """(64, 96) from (16, 24): the headline scan's low-resolution form takes ratios from ~3.8 up with a 68-column footprint."""
    _need_gpu()
    size = (64, 96)
    zq, _ = case(60 + C, 2, C, 16, 24, 7)
    _, spx = case(61 + C, 2, C, size[0], size[1], 7)
    invT = ops().inv_temperature(0.1)
    ps, cs, hh = ops().single_pass_accum_lowres(zq.cuda(), size, spx.cuda(), 7, invT)
    assert same(ops().uncertainty_accum_lowres(zq.cuda(), size, spx.cuda(), 7, invT, 'bvsb'), (ps, cs, hh))
    for m in NEW_MEASURES:
        p2, _, h2 = ops().uncertainty_accum_lowres(zq.cuda(), size, spx.cuda(), 7, invT, m)
        assert torch.equal(p2, ps) and torch.equal(h2, hh), m


@pytest.mark.parametrize("shape,size", [((2, 20, 17, 23), (65, 89)), ((1, 19, 16, 24), (64, 96)), ((2, 20, 17, 23), (17, 23))])
def test_low_resolution_form_equals_the_scan_of_the_materialised_tensor(shape, size):
    _need_gpu()
    B, C, h, w = shape
    zq, _ = case(80 + h, B, C, h, w, 7)
    _, spx = case(81 + h, B, C, size[0], size[1], 7, torch.int32)
    full = ops().upsample_bilinear(zq.cuda(), size)
    assert tuple(full.shape) == (B, C) + size
    for m in MEASURES:
        assert same(ops().uncertainty_accum_lowres(zq.cuda(), size, spx.cuda(), 7, 10.0, m),
                    ops().uncertainty_accum(full, spx.cuda(), 7, 10.0, m)), m


@pytest.mark.parametrize("shape,size", [((1, 20, 16, 16), (12, 64)), ((1, 20, 16, 16), (64, 12)), ((1, 20, 16, 16), (64, 97))])
def test_low_resolution_form_refuses_ratios_outside_its_limits_before_launch(shape, size):
    """A ratio below 1 along either axis, or above 6 along the rows: refused by the argument check, nothing accumulated."""
    _need_gpu()
    from mulactseg_amd import _lib
    zq, _ = case(5, *shape, 4)
    spx = torch.zeros((1,) + size, dtype=torch.int64, device='cuda')
    bufs = ops().uncertainty_accum(torch.zeros((1, 20, 2, 2), device='cuda'), torch.zeros((1, 2, 2), dtype=torch.int64, device='cuda'),
                                   4, 10.0, 'entropy')
    before = [t.clone() for t in bufs]
    with pytest.raises(_lib.MulActSegHipError, match="out of range"):
        ops().uncertainty_accum_lowres(zq.cuda(), size, spx, 4, 10.0, 'entropy', *bufs)
    torch.cuda.synchronize()
    assert same(bufs, before)


def test_low_resolution_call_allocates_no_full_resolution_logits():
    _need_gpu()
    B, C, h, w, H, W, S = 2, 20, 64, 128, 256, 512, 16
    zq, _ = case(7, B, C, h, w, S)
    _, spx = case(8, B, C, H, W, S)
    zq, spx = zq.cuda(), spx.cuda()
    bufs = ops().uncertainty_accum_lowres(zq, (H, W), spx, S, 10.0, 'entropy')          # (warm: library, kernels, allocator pools)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ops().uncertainty_accum_lowres(zq, (H, W), spx, S, 10.0, 'entropy', *bufs)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 4 * B * C * H * W
    assert int(bufs[2].sum()) == 2 * int(((spx >= 0) & (spx < S)).sum())


@pytest.mark.parametrize("modname,ncls,method", SELECTORS)
def test_selectors_on_the_device_equal_the_cpu_stand_in(modname, ncls, method):
    _need_gpu()
    from mulactseg_amd.active_selection.engine import HipBackend
    for measure in NEW_MEASURES:
        want_scores, want_prefix, _ = cpu_round(modname, ncls, method, measure)
        sel = make_selector(modname, ncls, method, measure)
        scores, prefix = run_round(sel, fake_trainer('cuda:0'), tiny_pool())
        assert isinstance(sel.backend, HipBackend)
        assert np.array_equal(scores, want_scores), measure
        assert prefix == want_prefix, measure


def test_entropy_round_through_a_real_model_on_its_low_resolution_logits():
    """One select_next_batch of the PixBal + ban selector with --uncertainty entropy through a seeded deeplabv3pluswn_resnet50deepstem
    on two 128 x 160 pictures: the scan reads the model's quarter-resolution logits (no fall-back), and scores and selection equal the
    same selector fed the materialised logits (ops.upsample_bilinear of the very tensors the model emitted)."""
    _need_gpu()
    from mulactseg_amd import synth
    from mulactseg_amd.active_selection.engine import HipBackend
    from mulactseg_amd.models import get_model
    dev = torch.device('cuda:0')
    n_img, Hh, Ww, nseg = 2, 128, 160, 16
    torch.manual_seed(3)
    net = get_model('deeplabv3pluswn_resnet50deepstem', 20, 16, True, pretrained_backbone=False).to(dev).eval()

    class Recording(torch.nn.Module):
        lowres_logits = True

        def __init__(self):
            super().__init__()
            self.net, self.seen = net, []

        def forward(self, x, lowres=False):
            y = self.net(x, lowres=lowres)
            self.seen.append((lowres, y))
            return y

    class Backend(HipBackend):
        calls = []

        def uncertainty_pass_lowres(self, *a):
            self.calls.append('lowres')
            return super().uncertainty_pass_lowres(*a)

        def uncertainty_pass(self, *a):
            self.calls.append('full')
            return super().uncertainty_pass(*a)

    g = torch.Generator(device=dev).manual_seed(5)
    pics = torch.randn((n_img, 3, Hh, Ww), generator=g, device=dev)
    maps = np.stack([synth.superpixel_map(900 + i, Hh, Ww, nseg) for i in range(n_img)])
    im_idx = [["i/%03d.png" % i, "l/%03d.png" % i, "s/spx_%04d.pkl" % i] for i in range(n_img)]
    suppix = {k[2]: list(range(nseg)) for k in im_idx}
    kw = dict(nseg=nseg)
    rec = Recording()
    sel = make_selector('my_bvsb_predclsbal_pwr_banignore', 19, SELECTORS[3][2], 'entropy', Backend(dev), **kw)
    tr = types.SimpleNamespace(net=rec, device=dev, model_save_dir=None, selection_iter=1)
    scores, prefix = run_round(sel, tr, (pics.cpu().numpy(), maps, im_idx, suppix), budget=5)
    assert Backend.calls == ['lowres'] and [low for low, _ in rec.seen] == [True]
    zq = rec.seen[0][1]
    assert tuple(zq.shape) == (n_img, 20, Hh // 4, Ww // 4)
    full = ops().upsample_bilinear(zq.contiguous(), (Hh, Ww)).cpu().numpy()
    ref = make_selector('my_bvsb_predclsbal_pwr_banignore', 19, SELECTORS[3][2], 'entropy', **kw)
    ref_scores, ref_prefix = run_round(ref, fake_trainer('cuda:0'), (full, maps, im_idx, suppix), budget=5)
    assert float(scores.max()) > 0 and np.array_equal(scores, ref_scores) and prefix == ref_prefix and len(prefix) >= 5
