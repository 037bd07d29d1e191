"""--cosprop_threshold_method on the GPU: the threshold kernels (csrc/stage2.hip, k_s2thr_*) against the plain definition on synthetic
assignments, and ops.stage2_pseudo_labels with 'min' and 'median' against the oracle port, pixel for pixel."""
import functools
import os
import tempfile
import types

import numpy as np
import pytest
import torch

import stage2_threshold_restated as R
from test_oracle_golden import stage2_inputs

pytestmark = pytest.mark.gpu

INPUTS = {'a': (71, 2, 20, 32, 64, 96, 48), 'b': (91, 2, 20, 8, 50, 77, 30)}
# pixels on which the port's 'min' and 'median' maps differ (include_onehot False, True): recorded from oracle/port.py on the CPU
PORT_MIN_VS_MEDIAN = {'a': (1053, 2438), 'b': (1678, 1811)}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(feats, z, tgt, spx, msk, S) of one input; 'b1' is input 'b' with a one-pixel and a two-pixel superpixel of two classes each."""
    if name != 'b1':
        feats, z, tgt, spx, msk, _ = stage2_inputs(*INPUTS[name])
        return feats, z, tgt, spx, msk, INPUTS[name][-1]
    feats, z, tgt, spx, msk, S = _inputs('b')
    tgt, spx, msk = tgt.copy(), spx.copy(), msk.copy()
    free = [s for s in range(S) if not msk[0][spx[0] == s].any()]
    one, two, into = free[0], free[1], free[2]
    spx[0][np.isin(spx[0], (one, two))] = into                 # the two ids give their pixels away ...
    y, x = 20, 30
    assert not msk[0, y:y + 2, x:x + 3].any()
    spx[0, y, x] = one                                         # ... and get one and two pixels back, selected
    spx[0, y + 1, x + 1:x + 3] = two
    msk[0, y, x] = msk[0, y + 1, x + 1:x + 3] = True
    tgt[0, one] = tgt[0, two] = 0
    tgt[0, one, [2, 5]] = 1
    tgt[0, two, [3, 11]] = 1
    assert (spx[0] == one).sum() == 1 and (spx[0] == two).sum() == 2
    return feats, z, tgt, spx, msk, S


@functools.lru_cache(maxsize=None)
def _port(name, include, method):
    from oracle import port
    feats, z, tgt, spx, msk, S = _inputs(name)
    n = torch.get_num_threads()
    torch.set_num_threads(1)                    # (ATen's CPU rounding depends on the thread count: tests/test_oracle_golden.py)
    try:
        T = torch.from_numpy
        out = port.cosine_pseudo_labels(T(feats), T(z), T(tgt), T(msk), T(spx), S, include, threshold_method=method).numpy()
    finally:
        torch.set_num_threads(n)
    out.setflags(write=False)
    return out


def _product(ops, name, include, method, feats=None):
    f, z, tgt, spx, msk, _ = _inputs(name)
    return ops.stage2_pseudo_labels(_c(f if feats is None else feats), _c(z), _c(tgt), _c(msk), _c(spx), include,
                                    threshold_method=method).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("HW,n_proto", R.SHAPES)
def test_kernel_equals_the_definition(HW, n_proto, method, monkeypatch):
    """thr == sort / min of the selected similarities, bit for bit, on every value pattern; an id without a pixel gets 1.0; the same call
    twice gives the same bytes; the torch chain (MAS_STAGE2_THRESHOLD=aten) gives equal values."""
    ops = _gpu()
    monkeypatch.delenv("MAS_STAGE2_THRESHOLD", raising=False)
    for pattern in R.PATTERNS:
        nn, sim = R.case(HW, n_proto, pattern)
        want = R.thresholds_plain(nn, sim, n_proto, method)
        dn, ds = _c(nn), _c(sim)
        got = ops.stage2_thresholds(dn, ds, n_proto, method)
        again = ops.stage2_thresholds(dn, ds, n_proto, method)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n_proto,)
        got, again = got.cpu().numpy(), again.cpu().numpy()
        print(pattern, HW, n_proto, method, "mismatches", int((got != want).sum()))
        assert np.array_equal(got, want), pattern
        assert got.tobytes() == again.tobytes(), pattern
        if n_proto > 1:
            assert got[n_proto - 1] == 1.0 and not (nn == n_proto - 1).any()
        monkeypatch.setenv("MAS_STAGE2_THRESHOLD", "aten")
        aten = ops.stage2_thresholds(dn, ds, n_proto, method).cpu().numpy()
        monkeypatch.delenv("MAS_STAGE2_THRESHOLD")
        assert np.array_equal(got, aten), pattern


def test_no_pixel_takes_part():
    ops = _gpu()
    nn = torch.full((50 * 77,), -1, dtype=torch.int32, device='cuda')
    sim = torch.rand(50 * 77, device='cuda')
    for method in R.METHODS:
        assert torch.equal(ops.stage2_thresholds(nn, sim, 5, method), torch.ones(5, device='cuda'))


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include", [False, True])
@pytest.mark.parametrize("name", ['a', 'b'])
def test_label_maps_equal_the_oracle_for_both_methods(name, include):
    """Full-resolution features: the map equals oracle.port.cosine_pseudo_labels(..., threshold_method=...) on every pixel.  (On these
    inputs the port gives identical maps in float32 and float64 for both methods and both include_onehot values: no near-tie sits
    within float32 rounding of a decision.)"""
    ops = _gpu()
    maps = {}
    for method in ('min', 'median'):
        maps[method] = _product(ops, name, include, method)
        want = _port(name, include, method)
        print(name, include, method, "pixels that differ from the port:", int((maps[method] != want).sum()))
        assert np.array_equal(maps[method], want), method
    assert int((_port(name, include, 'min') != _port(name, include, 'median')).sum()) == PORT_MIN_VS_MEDIAN[name][int(include)]
    assert (maps['min'] != maps['median']).any()
    f, z, tgt, spx, msk, _ = _inputs(name)
    assert np.array_equal(maps['median'], ops.stage2_pseudo_labels(_c(f), _c(z), _c(tgt), _c(msk), _c(spx), include).cpu().numpy())   # the default


def test_median_port_equals_the_c_oracle():
    _gpu()
    from oracle import exact
    feats, z, tgt, spx, msk, _ = _inputs('a')
    for include in (False, True):
        assert np.array_equal(_port('a', include, 'median'), exact.stage2_pseudo_labels(feats, z, tgt, msk, spx, include))


@pytest.mark.parametrize("include", [False, True])
def test_prototype_without_pixels_in_a_picture(include):
    """A selected superpixel of one pixel with two target classes: both prototypes are that pixel, the first attracts it, the second
    attracts nothing and gets the threshold 1.0; a two-pixel superpixel has the even count."""
    ops = _gpu()
    for method in R.METHODS:
        got = _product(ops, 'b1', include, method)
        assert np.array_equal(got, _port('b1', include, method)), method
    feats, z, tgt, spx, msk, _ = _inputs('b1')
    assert got[0, 20, 30] in (2, 5) and set(got[0, 21, 31:33].tolist()) <= {3, 11}


@pytest.mark.parametrize("include", [False, True])
def test_quarter_resolution_min_admits_what_median_admits(include):
    """Lower thresholds only admit more: the pixels labelled under 'median' are labelled under 'min'; the pixels that take their own
    prototype's class carry the same label under both."""
    ops = _gpu()
    feats, z, tgt, spx, msk, S = _inputs('a')
    q = torch.nn.functional.avg_pool2d(torch.from_numpy(feats), 4)
    q = torch.nn.functional.normalize(q).numpy()
    lo, md = _product(ops, 'a', include, 'min', q), _product(ops, 'a', include, 'median', q)
    assert np.all((lo != 255) | (md == 255)) and (lo != 255).sum() >= (md != 255).sum() > 0
    own = msk if include else msk & (tgt.sum(-1) > 1)[np.arange(msk.shape[0])[:, None, None], spx]
    assert own.any() and np.array_equal(lo[own], md[own]) and np.all(md[own] != 255)


def test_trainer_writes_the_min_labels():
    """trainer/eval_save_cosplbl_prop_includeonehot with --cosprop_threshold_method min: the PNG decodes to the 'min' map."""
    ops = _gpu()
    from PIL import Image
    from mulactseg_amd.trainer import eval_save_cosplbl_prop_includeonehot as G
    feats, z, tgt, spx, msk, S = _inputs('b')
    labels = stage2_inputs(*INPUTS['b'])[5]
    dev = torch.device('cuda:0')

    class Net(torch.nn.Module):
        def feat_forward_lowres(self, images):
            return _c(feats[:1]), _c(z[:1])
    batch = {'images': torch.zeros((1, 3, 50, 77), device=dev), 'labels': _c(labels[:1]), 'spx': _c(spx[:1]), 'spmask': _c(msk[:1]),
             'target': _c(tgt[:1]), 'fnames': [["i/p000.png", "l/p000.png", "s/p000.pkl"]]}

    class Loader:
        def __len__(self):
            return 1

        def __next__(self):
            return batch
    tmp = tempfile.mkdtemp(prefix="mas_s2thr_")
    tr = object.__new__(G.ActiveTrainer)
    tr.args = types.SimpleNamespace(ignore_idx=255, init_checkpoint=os.path.join(tmp, "checkpoint01.tar"), plbl_type=None, val_batch_size=1,
                                    cosprop_threshold_method='min')
    tr.net, tr.device, tr.num_classes, tr.selection_iter, tr.save_dir = Net().to(dev), dev, 19, 1, None
    tr.inference(Loader())
    png = np.asarray(Image.open(os.path.join(tr._save_dir(), "p000.png"))).astype(np.int64)
    want = {m: ops.stage2_pseudo_labels(_c(feats[:1]), _c(z[:1]), _c(tgt[:1]), _c(msk[:1]), _c(spx[:1]), True, threshold_method=m)[0].cpu().numpy()
            for m in R.METHODS}
    assert np.array_equal(png, want['min']) and (want['min'] != want['median']).any()
