"""The cross-view hierarchical group terms without a GPU: the second section of csrc/hier_group.h through the library's host loop
(``ops.async_hier_loss_reference``) against a float64 numpy restatement written here from the formula (``restated_async``), and against
the executed reference (tests/golden/g20_async_hier.npz) at the tolerances of tests/test_wgroup_cpu.py -- 1e-5 * |restated| for the loss
against float64, 1e-4 * max(1, |ref|) for loss values and 1e-4 * max|ref| for gradients against the executed reference; counts and the
integer tables exactly, the f32 weight table within 1e-6 relative of float64 --, plus the corner cases, the entry-point checks, the
parser rules, the constructors, the trainer modules, the transforms and the ABI tables."""
import os
import re
import types

import numpy as np
import pytest
import torch

from test_losses_gpu import _inputs as inputs          # (the same function as record_partial_label_golden.inputs)
from test_hier_group_cpu import BASE, bits_of, restated, small_map, with_last_column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g20_async_hier.npz")
EPS = 1e-8
SEED, N, C, HO, WO, S = 41, 2, 20, 40, 44, 48                # the weak view: g19's inputs
ROWS, COLS, STRONG_SEED = slice(5, 29), slice(8, 40), 7      # the strong view: a flipped 24 x 32 window of the weak maps
KEYS = {'async': None, 'wmax': 'max', 'wmean': 'mean'}
# the issue's table: Ss -> (n, sum of `async`, of `wmax`, of `wmean`) of the executed reference
ISSUE = {192: (91, 282.4527, 27.1341, 16.2179), 12: (674, 2091.2817, 223.0869, 107.3213)}


def _ops():
    from mulactseg_amd import ops
    return ops


def window(a):
    """Rows 5..29 and columns 8..40 of a weak-view [N,H,W] array, flipped left-right."""
    return np.ascontiguousarray(a[:, ROWS, COLS][:, :, ::-1])


_VIEWS = {}


def views(Ss):
    """The two views of g20 for a fine map of Ss ids, made once: a dict of host arrays -- zw, tgt [N,S,C+1], spx_w, small_w, msk_w (the
    weak view) and z, spx, small, msk (the strong view)."""
    if Ss not in _VIEWS:
        from mulactseg_amd import synth
        zw, tgt, spx_w, msk_w = inputs(SEED, N, C, HO, WO, S)
        small_w = small_map(SEED, spx_w, S, Ss)
        _VIEWS[Ss] = dict(zw=zw, tgt=with_last_column(tgt), spx_w=spx_w, small_w=small_w, msk_w=msk_w, z=synth.logits(STRONG_SEED, N, C, 24, 32),
                          spx=window(spx_w), small=window(small_w), msk=window(msk_w))
    return _VIEWS[Ss]


def softmax64(z):
    x = z.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    n, c = z.shape[:2]
    return (e / e.sum(axis=1, keepdims=True)).transpose(0, 2, 3, 1).reshape(n, -1, c)


def restated_async(v, Ss, weight=None, upstream=1.0, tables=None):
    """The term in float64, from the formula, on the views ``v``.  ``weight`` None / 'max' / 'mean'.  ``tables`` = (mult, wgt or None)
    replaces the weak view.  Returns a dict: loss, n, total (the sum before the division), mult int64 [N,Ss,C], wgt float64 [N,Ss,C] or
    None, grad (of upstream * loss), gap (of the weak view's arg-pixel decisions, see ``test_hier_group_cpu.restated``), value float64
    [N,Ss,C] (the unweighted summed likelihood of every fine superpixel and class over the strong view) and size int64 [N,Ss]."""
    z, small, msk = v['z'], v['small'], np.asarray(v['msk']).astype(bool)
    n_pic, n_cls = z.shape[:2]
    gap, wgt = np.inf, None
    if tables is not None:
        mult, wgt = tables
        mult = np.asarray(mult).astype(np.int64)
        wgt = None if wgt is None else np.asarray(wgt).astype(np.float64)
    else:
        r = restated(v['zw'], v['tgt'], v['spx_w'], v['small_w'], v['msk_w'], Ss, False)
        mult, gap = r['mult'], r['gap']
        if weight is not None:
            pw = softmax64(v['zw'])
            wgt = np.zeros((n_pic, Ss, n_cls))
            for i in range(n_pic):
                sel = np.asarray(v['msk_w'][i]).astype(bool).reshape(-1)
                ids = v['small_w'][i].reshape(-1)
                for f in np.nonzero(mult[i].any(axis=1))[0]:
                    rows = pw[i][sel & (ids == f)]
                    if rows.shape[0]:
                        red = rows.max(axis=0) if weight == 'max' else rows.mean(axis=0)
                        wgt[i, f] = np.where(mult[i, f] > 0, red, 0.0)
    p = softmax64(z)
    w_all = mult.astype(np.float64) * (wgt if wgt is not None else 1.0)
    counted_mult = mult * ((wgt != 0) if wgt is not None else 1)
    value, size = np.zeros((n_pic, Ss, n_cls)), np.zeros((n_pic, Ss), dtype=np.int64)
    total, n, counted = 0.0, 0, []
    for i in range(n_pic):
        for pix in np.nonzero(msk[i].reshape(-1))[0]:
            f = small[i].reshape(-1)[pix]
            if not 0 <= f < Ss:
                continue
            value[i, f] += -np.log(p[i, pix] + EPS)
            size[i, f] += 1
            if not mult[i, f].any():
                continue
            total += float((w_all[i, f] * -np.log(p[i, pix] + EPS)).sum())
            n += int(counted_mult[i, f].sum())
            counted.append((i, pix, w_all[i, f]))
    grad = np.zeros(p.shape)
    a = upstream / (1 + n)
    for i, pix, w in counted:
        q = p[i, pix] / (p[i, pix] + EPS)
        grad[i, pix] = a * (p[i, pix] * (w * q).sum() - w * q)
    h, w_ = z.shape[2:]
    return dict(loss=total / (1 + n), n=n, total=total, mult=mult, wgt=wgt, gap=gap, value=value, size=size,
                grad=grad.reshape(n_pic, h, w_, n_cls).transpose(0, 3, 1, 2))


def weak_of(v, dtype=np.int64):
    return (torch.from_numpy(v['zw']), None, torch.from_numpy(v['spx_w']), torch.from_numpy(v['small_w'].astype(dtype)),
            torch.from_numpy(v['msk_w']), bits_of(v['tgt'][..., :-1]))


def host(v, Ss, weight=None, upstream=None, tables=None, dtype=np.int64):
    grad = None if upstream is None else torch.tensor([upstream], dtype=torch.float32)
    return _ops().async_hier_loss_reference(torch.from_numpy(v['z']), None, torch.from_numpy(v['small'].astype(dtype)), Ss,
                                            torch.from_numpy(v['msk']), weak=None if tables is not None else weak_of(v, dtype),
                                            tables=tables, weight_reduce=weight, grad=grad)


def any_of(mult):
    return ((np.asarray(mult) > 0).astype(np.int64) << np.arange(np.asarray(mult).shape[-1])).sum(-1)


def other_views(shape):
    """Views of another shape (N, C, Ho, Wo, S, Ss): the strong view is the flipped window rows 3.., columns 2.. of the weak maps."""
    from mulactseg_amd import synth
    n, c, ho, wo, s, ss = shape
    zw, tgt, spx_w, msk_w = inputs(500 + wo + c, n, c, ho, wo, s)
    small_w = small_map(500 + wo + c, spx_w, s, ss)

    def win(a):
        return np.ascontiguousarray(a[:, 3:ho - 4, 2:wo - 5][:, :, ::-1])
    return dict(zw=zw, tgt=with_last_column(tgt), spx_w=spx_w, small_w=small_w, msk_w=msk_w, z=synth.logits(11 + c, n, c, ho - 7, wo - 7),
                spx=win(spx_w), small=win(small_w), msk=win(msk_w))


@pytest.mark.parametrize("case", [192, 12, (2, 21, 33, 37, 150, 40), (1, 7, 24, 36, 16, 30)])
@pytest.mark.parametrize("key", list(KEYS))
def test_the_host_loop_matches_the_float64_restatement(case, key):
    v, Ss = (views(case), case) if isinstance(case, int) else (other_views(case), case[-1])
    r = restated_async(v, Ss, KEYS[key], upstream=16.0)
    out = host(v, Ss, KEYS[key], upstream=16.0)
    err = abs(float(out['loss']) - r['loss'])
    print("async %s %s: loss %.7g restated %.7g n %d error %.3e bound %.3e gap %.3e" % (case, key, float(out['loss']), r['loss'], r['n'], err,
                                                                                        1e-5 * abs(r['loss']), r['gap']))
    assert r['gap'] > 1e-5                       # no arg-pixel decision that matters is near its edge
    assert int(out['acc'][1]) == r['n'] > 0
    assert np.array_equal(out['mult'].numpy().astype(np.int64), r['mult'])
    assert np.array_equal(out['any'].numpy().astype(np.int64) & 0xffffffff, any_of(r['mult']))
    if KEYS[key] is None:
        assert out['wgt'] is None
    else:
        got = out['wgt'].numpy().astype(np.float64)
        assert np.array_equal(got != 0, r['wgt'] != 0) and np.all(np.abs(got - r['wgt']) <= 1e-6 * r['wgt'])
    assert err <= 1e-5 * abs(r['loss'])
    gerr, scale = float(np.max(np.abs(out['dz'].numpy() - r['grad']))), float(np.max(np.abs(r['grad'])))
    print("   gradient: max error %.3e of max|ref| %.3e" % (gerr, scale))
    assert scale > 0 and gerr <= 1e-4 * scale


@pytest.mark.parametrize("Ss", [192, 12])
@pytest.mark.parametrize("key", list(KEYS))
def test_the_host_loop_matches_the_executed_reference(Ss, key):
    """Measured when the golden was recorded: the executed reference (float32 torch on the CPU) lies within 9.2e-8 relative of the
    float64 restatement for the loss and within 2.3e-7 of max|grad| for the gradient in all six cases; `wmean` alone, whose f32 sum in
    source order is a deliberate difference, measures 2.8e-8 / 7.8e-9 for the loss and 1.9e-7 / 2.3e-7 for the gradient (Ss = 192 /
    12).  All of that is more than 10 times below the 1e-4 of tests/test_wgroup_cpu.py, which therefore is the tolerance here for all
    three classes (the golden carries the two worst figures, and the test asserts them 10 x below the bound)."""
    g = np.load(GOLDEN)
    v = views(Ss)
    k = "%s_%d" % (key, Ss)
    r = restated_async(v, Ss, KEYS[key])
    assert r['gap'] > 1e-5                       # the cap on excluded entries is zero
    assert float(g['worst_loss']) <= 1e-5 and float(g['worst_grad']) <= 1e-5          # the recorder's measurement, 10 x below the bound
    out = host(v, Ss, KEYS[key], upstream=float(g['weight']))
    ref, gref = float(g[k + '_loss']), g[k + '_grad']
    print("g20 %s: n %d (golden %d, restated %d), loss %.7g golden %.7g restated %.7g, gap %.3e"
          % (k, int(out['acc'][1]), int(g[k + '_n']), r['n'], float(out['loss']), ref, r['loss'], r['gap']))
    assert int(out['acc'][1]) == int(g[k + '_n']) == r['n'] > 0
    assert abs(float(out['loss']) - ref) <= 1e-4 * max(1.0, abs(ref))
    total = float(out['loss']) * (r['n'] + 1)
    assert abs(total - float(g[k + '_sum'])) <= 1e-4 * max(1.0, abs(float(g[k + '_sum'])))
    err, scale = float(np.max(np.abs(out['dz'].numpy() - gref))), float(np.max(np.abs(gref)))
    print("g20 %s gradient: max error %.3e of max|ref| %.3e" % (k, err, scale))
    assert scale > 0 and err <= 1e-4 * scale


def test_the_golden_holds_the_issues_counts_and_sums():
    g = np.load(GOLDEN)
    for Ss, (n, *sums) in ISSUE.items():
        for key, want in zip(KEYS, sums):
            assert int(g["%s_%d_n" % (key, Ss)]) == n
            assert abs(float(g["%s_%d_sum" % (key, Ss)]) - want) <= 5e-4, (Ss, key, float(g["%s_%d_sum" % (key, Ss)]))
    assert int(g['max_mult_12']) >= 2 and int(g['absent_pairs_192']) > 0


@pytest.mark.parametrize("shape", [(2, 20, 40, 44, 48, 12), (2, 21, 33, 37, 150, 40)])
def test_the_unweighted_forward_on_given_tables_equals_the_hier_group_reference_when_the_views_coincide(shape):
    from test_hier_group_cpu import case
    ops = _ops()
    z, tgt, spx, small, msk = case(shape)
    Ss = shape[-1]
    grad = torch.tensor([16.0], dtype=torch.float32)
    zt, st, ft, mt, bits = torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(small), torch.from_numpy(msk), bits_of(tgt[..., :-1])
    ref = ops.hier_group_loss_reference(zt, None, st, ft, Ss, mt, bits, grad=grad)
    both = ops.async_hier_loss_reference(zt, None, ft, Ss, mt, weak=(zt, None, st, ft, mt, bits), grad=grad)
    given = ops.async_hier_loss_reference(zt, None, ft, Ss, mt, tables=(ref['mult'], ref['any'], None), grad=grad)
    assert int(ref['acc'][1]) > 0
    for out in (both, given):
        assert torch.equal(out['acc'], ref['acc']) and torch.equal(out['loss'].view(torch.int32), ref['loss'].view(torch.int32))
        assert torch.equal(out['dzq_fix'], ref['dzq_fix']) and torch.equal(out['mult'], ref['mult']) and torch.equal(out['any'], ref['any'])
    assert torch.equal(both['gmax'], ref['gmax'])


def test_pairs_of_weight_zero_add_nothing_to_sum_count_or_gradient():
    v = views(12)
    base = host(v, 12, 'max', upstream=16.0)
    mult, any_, wgt = base['mult'], base['any'], base['wgt'].clone()
    pairs = torch.nonzero(mult > 0)
    assert pairs.shape[0] > 4
    gone = pairs[::2]                                              # every other pair loses its weight
    wgt[gone[:, 0], gone[:, 1], gone[:, 2]] = 0.0
    out = host(v, 12, upstream=16.0, tables=(mult, any_, wgt))
    # the same as a table those pairs were never in
    m2 = mult.clone()
    m2[gone[:, 0], gone[:, 1], gone[:, 2]] = 0
    a2 = torch.from_numpy(any_of(m2.numpy()).astype(np.int64)).to(torch.int32)
    want = host(v, 12, upstream=16.0, tables=(m2, a2, wgt))
    assert 0 < int(out['acc'][1]) < int(base['acc'][1])
    assert torch.equal(out['acc'], want['acc']) and torch.equal(out['dzq_fix'], want['dzq_fix'])
    r = restated_async(v, 12, tables=(mult.numpy(), wgt.numpy()), upstream=16.0)
    assert int(out['acc'][1]) == r['n'] and abs(float(out['loss']) - r['loss']) <= 1e-5 * abs(r['loss'])
    assert float(np.max(np.abs(out['dz'].numpy() - r['grad']))) <= 1e-4 * float(np.max(np.abs(r['grad'])))
    # every weight zero: nothing is counted
    none = host(v, 12, upstream=16.0, tables=(mult, any_, torch.zeros_like(wgt)))
    assert int(none['acc'][0]) == 0 and int(none['acc'][1]) == 0 and float(none['loss']) == 0.0 and not bool(none['dzq_fix'].any())


@pytest.mark.parametrize("key", list(KEYS))
def test_empty_views(key):
    v = dict(views(12))
    whole = host(v, 12, KEYS[key], upstream=1.0)
    # no selected strong pixel at all: loss 0, zero gradient (the tables are still those of the weak view)
    e = dict(v, msk=np.zeros_like(v['msk']))
    out = host(e, 12, KEYS[key], upstream=1.0)
    assert int(out['acc'][0]) == 0 and int(out['acc'][1]) == 0 and float(out['loss']) == 0.0 and not bool(out['dzq_fix'].any())
    assert torch.equal(out['mult'], whole['mult'])
    # one picture without selected strong pixels is skipped: the batch equals the other picture alone
    m = v['msk'].copy()
    m[1] = False
    one = host(dict(v, msk=m), 12, KEYS[key], upstream=1.0)
    alone = host({k: a[:1] for k, a in v.items()}, 12, KEYS[key], upstream=1.0)
    assert torch.equal(one['acc'], alone['acc']) and not bool(one['dz'][1].any()) and int(one['acc'][1]) > 0
    # selected strong pixels but no selected weak pixel: no pair
    w = dict(v, msk_w=np.zeros_like(v['msk_w']))
    out = host(w, 12, KEYS[key], upstream=1.0)
    assert int(out['mult'].sum()) == 0 and int(out['any'].abs().sum()) == 0 and int(out['acc'][1]) == 0 and float(out['loss']) == 0.0
    assert not bool(out['dzq_fix'].any()) and (out['wgt'] is None or not bool(out['wgt'].any()))
    for o in (whole, one, out):
        assert bool(torch.isfinite(o['loss']).all()) and bool(torch.isfinite(o['dz']).all())


def test_the_id_dtypes_agree_and_an_unknown_one_is_refused():
    v = views(12)
    a, b = host(v, 12, 'mean', upstream=1.0), host(v, 12, 'mean', upstream=1.0, dtype=np.int32)
    for k in ('acc', 'mult', 'any', 'wgt', 'dzq_fix'):
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(TypeError):
        host(v, 12, dtype=np.uint8)
    with pytest.raises(ValueError, match="weight_reduce"):
        host(v, 12, 'median')


def _codes():
    codes = {}
    for line in open(os.path.join(ROOT, "mulactseg_amd", "csrc", "common.h")):
        m = re.match(r"#define (MAS_ERR_\w+)\s+\(?(-?\d+)\)?", line)
        if m:
            codes[m.group(1)] = int(m.group(2))
    return codes


def test_error_codes_of_the_reference_entry_point():
    from mulactseg_amd import _lib
    lib = _lib.load()
    v = views(12)
    zw, sw, fw, mw = (torch.from_numpy(v[k]) for k in ('zw', 'spx_w', 'small_w', 'msk_w'))
    z, f, m = (torch.from_numpy(v[k]) for k in ('z', 'small', 'msk'))
    mw, m = mw.view(torch.uint8), m.view(torch.uint8)
    bits = bits_of(v['tgt'][..., :-1])
    mult, any_, wgt = torch.zeros((N, 12, C), dtype=torch.int32), torch.zeros((N, 12), dtype=torch.int32), torch.zeros((N, 12, C))
    acc = torch.zeros(3, dtype=torch.int64)

    def call(zq_weak=zw.data_ptr(), mode=1, zq=z.data_ptr(), C=C, small_dtype=0, weak_dtype=0, Ss=12, mult_p=mult.data_ptr(),
             wgt_p=wgt.data_ptr(), acc_p=acc.data_ptr(), S=S):
        return lib.mas_async_hier_reference(zq_weak, HO, WO, sw.data_ptr(), 0, fw.data_ptr(), weak_dtype, mw.data_ptr(), bits.data_ptr(), HO,
                                            WO, S, mode, zq, 24, 32, f.data_ptr(), small_dtype, m.data_ptr(), N, C, 24, 32, Ss, None, None,
                                            mult_p, any_.data_ptr(), wgt_p, acc_p, None, None)
    codes = _codes()
    assert call() == 0 and call(mode=0, wgt_p=None) == 0 and call(mode=2) == 0
    assert call(zq=None) == codes['MAS_ERR_NULL'] and call(zq_weak=None) == codes['MAS_ERR_NULL']
    assert call(wgt_p=None) == codes['MAS_ERR_NULL']                # a weighted mode without a place for the weights
    assert call(zq_weak=None, mode=_lib.AHG_TABLES_GIVEN) == 0      # given tables: the weak view is not read
    assert call(mode=3) == codes['MAS_ERR_RANGE'] and call(mode=8) == codes['MAS_ERR_RANGE']
    assert call(C=33) == codes['MAS_ERR_CLASSES']
    assert call(small_dtype=7) == codes['MAS_ERR_DTYPE'] and call(weak_dtype=7) == codes['MAS_ERR_DTYPE']
    assert call(Ss=0) == codes['MAS_ERR_SHAPE'] and call(S=0) == codes['MAS_ERR_SHAPE']
    assert call(mult_p=mult.data_ptr() + 2) == codes['MAS_ERR_ALIGN']
    assert call(wgt_p=wgt.data_ptr() + 2) == codes['MAS_ERR_ALIGN']
    assert call(acc_p=acc.data_ptr() + 4) == codes['MAS_ERR_ALIGN']
    assert lib.mas_async_hier_work_bytes(N, S, 12, C, 0) == lib.mas_online_plbl_work_bytes(N, S, C)
    assert lib.mas_async_hier_work_bytes(N, S, 12, C, 2) == 8 * (8 + N * S * C + N * 12 * C + N * 12 // 2)
    assert lib.mas_async_hier_work_bytes(0, S, 12, C, 0) == 0


def test_header_exports_and_ctypes_table_agree_and_the_abi_stays_9():
    from mulactseg_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mulactseg_hip.h")).read()
    assert int(re.search(r"#define MAS_ABI_VERSION (\d+)", header).group(1)) == 9 == lib.mas_abi_version()
    names = ('mas_async_hier_tables', 'mas_async_hier_fwd', 'mas_async_hier_value', 'mas_async_hier_bwd', 'mas_async_hier_reference',
             'mas_train_augment_maps')
    for name in names + ('mas_async_hier_work_bytes',):
        decl = re.search(r"(?:int|size_t) %s\((.*?)\);" % name, header, re.S).group(1)
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(',') if a.strip()])
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        assert 'invT' not in decl                                     # both softmaxes run at temperature 1
    want = tuple(int(re.search(r"#define %s (\d+)" % k, header).group(1))
                 for k in ('MAS_AHG_WEIGHT_NONE', 'MAS_AHG_WEIGHT_MAX', 'MAS_AHG_WEIGHT_MEAN', 'MAS_AHG_TABLES_GIVEN'))
    assert (_lib.AHG_WEIGHT_NONE, _lib.AHG_WEIGHT_MAX, _lib.AHG_WEIGHT_MEAN, _lib.AHG_TABLES_GIVEN) == want == (0, 1, 2, 4)
    spec = open(os.path.join(ROOT, "mulactseg_amd", "csrc", "hier_group.h")).read()
    frac = int(re.search(r"#define MAS_AHG_WEIGHT_FRAC (\d+)", spec).group(1))
    assert (2 ** frac + 2 ** (frac - 23)) * 2 ** 21 < 2 ** 64           # the mean's u64 sum cannot wrap at 1024 x 2048 pixels


def test_arg_assert_rules():
    from mulactseg_amd.utils import common
    p = common.get_parser()
    assert p.parse_args(BASE).weight_reduce == 'max'

    def check(method, extra):
        a = p.parse_args(BASE + extra)
        a.method, a.init_checkpoint, a.trg_datalist, a.region_dict = method, 'x.tar', 'seed64.txt', 'seed64.dict'
        a.datalist_path = a.resume_checkpoint = None
        common.arg_assert(a)
        return a
    plain, weighted = 'active_joint_hier_multi_async', 'active_joint_hier_multi_async_weight'
    for method in (plain, weighted):
        check(method, ['--load_smaller_spx'])
        with pytest.raises(ValueError, match="load_smaller_spx"):
            check(method, [])
        with pytest.raises(NotImplementedError, match="gumbel_scale"):
            check(method, ['--load_smaller_spx', '--gumbel_scale', '0.5'])
        with pytest.raises(NotImplementedError, match="nocropsp"):
            check(method, ['--load_smaller_spx', '--nocropsp'])
        with pytest.raises(NotImplementedError, match="group_only_single"):
            check(method, ['--load_smaller_spx', '--group_only_single'])
    assert check(weighted, ['--load_smaller_spx', '--weight_reduce', 'mean']).weight_reduce == 'mean'
    for method in (plain, 'active_joint_hier_multi', 'active_joint_multi_predignore', 'active_joint_multi_predignore_wgroup'):
        with pytest.raises(NotImplementedError, match="weight_reduce"):
            check(method, ['--load_smaller_spx', '--weight_reduce', 'mean'])
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ['--weight_reduce', 'median'])
    # the sibling's rules keep holding
    a = check('active_joint_hier_multi', ['--load_smaller_spx', '--group_only_single', '--nocropsp'])
    assert a.group_only_single is True and a.nocropsp is True


def test_the_constructors():
    from mulactseg_amd.utils import loss as L
    args = types.SimpleNamespace(small_nseg=12)
    for cls in (L.AsyncHierGroupMultiLabelCE, L.WeightAsyncHierGroupMultiLabelCE):
        assert issubclass(cls, L.HierGroupMultiLabelCE)
        with pytest.raises(NotImplementedError, match="gumbel"):
            cls(args, 19, 48, False, 0.5)
        m = cls(args, 19, 48, False, -1, reduction='none', temperature=0.1)
        assert m.temp == 1.0 and m.num_small_superpixel == 12 and m.reduction == 'none' and m.num_superpixel == 48
    assert L.AsyncHierGroupMultiLabelCE(args, 19, 48, False, -1)._weight_reduce is None
    assert L.WeightAsyncHierGroupMultiLabelCE(args, 19, 48, False, -1).weight_reduce == 'max'
    assert L.WeightAsyncHierGroupMultiLabelCE(args, 19, 48, False, -1, weight_reduce='mean')._weight_reduce == 'mean'
    with pytest.raises(ValueError, match="weight_reduce"):
        L.WeightAsyncHierGroupMultiLabelCE(args, 19, 48, False, -1, weight_reduce='median')


def test_the_trainer_modules_build_their_criteria():
    from mulactseg_amd.trainer import (active_joint_hier_multi, active_joint_hier_multi_async as plain,
                                       active_joint_hier_multi_async_weight as weighted)
    from mulactseg_amd.utils import loss as L
    assert issubclass(plain.ActiveTrainer, active_joint_hier_multi.ActiveTrainer) and issubclass(weighted.ActiveTrainer, plain.ActiveTrainer)

    def trainer(**kw):
        return types.SimpleNamespace(args=types.SimpleNamespace(nseg=64, small_nseg=256, group_ce_temp=0.1, multi_ce_temp=0.1,
                                                                group_only_single=False, gumbel_scale=-1, **kw), num_classes=19)
    tr = trainer()
    tr.group_criterion = lambda: plain.ActiveTrainer.group_criterion(tr)
    plain.ActiveTrainer.get_criterion(tr)
    assert type(tr.hier_group_multi_loss) is L.AsyncHierGroupMultiLabelCE and tr.hier_group_multi_loss.temp == 1.0
    assert tr.hier_group_multi_loss.args is tr.args                 # the reference forgets to pass args
    assert type(tr.multi_pos_loss) is L.MultiChoiceCE and tr.multi_pos_loss.temp == 0.1
    for kw, want in ((dict(), 'max'), (dict(weight_reduce='mean'), 'mean')):
        tr = trainer(**kw)
        tr.group_criterion = lambda: weighted.ActiveTrainer.group_criterion(tr)
        weighted.ActiveTrainer.get_criterion(tr)
        assert type(tr.hier_group_multi_loss) is L.WeightAsyncHierGroupMultiLabelCE and tr.hier_group_multi_loss.weight_reduce == want
    tr.args.gumbel_scale = 0.5
    with pytest.raises(NotImplementedError):
        weighted.ActiveTrainer.get_criterion(tr)


def test_the_transforms():
    from mulactseg_amd import dataloader
    from mulactseg_amd.dataloader import device_transforms as D, get_async_train_transform, get_train_transform

    def args(small):
        return types.SimpleNamespace(ignore_idx=255, nseg=2048, small_nseg=8192, load_smaller_spx=small)
    # get_train_transform answers as before
    t = get_train_transform(args(True), 'rescale_769_multi_notrg')
    assert type(t) is D.DeviceTrainAugment and t.n_maps == 2 and t.pad_values == [2048, 8192]
    t = get_train_transform(args(False), 'rescale_769_multi_notrg_ignore')
    assert type(t) is D.DeviceTrainAugment and t.n_maps == 2 and t.pad_values == [0, 2048]
    for name in ('rescale_769_multi', 'rescale_769_multi_notrg_ignore', 'rescale_769_multi_notrg_ignore_strongv1'):
        with pytest.raises(NotImplementedError):
            get_train_transform(args(True), name)
    # the three-map path of the cross-view loader
    t = get_async_train_transform(args(True), 'rescale_769_multi_notrg_ignore')
    assert type(t) is D.DeviceTrainAugmentThreeMaps and t.n_maps == 3 and t.all_pad_values == [0, 2048, 8192]
    assert t.size == (768, 768) and tuple(t.scale_range) == (0.5, 2.0)
    with pytest.raises(NotImplementedError, match="rescale_769_multi_notrg_ignore"):
        get_async_train_transform(args(True), 'rescale_769_multi_notrg')
    with pytest.raises(NotImplementedError, match="load_smaller_spx"):
        get_async_train_transform(args(False), 'rescale_769_multi_notrg_ignore')
    with pytest.raises(ValueError):
        D.DeviceTrainAugmentThreeMaps(pad_values=[0, 1])
    # the two-map and the three-map transform consume the same draws in the same order
    import random
    a, b = D.DeviceTrainAugment(pad_values=[0, 2048], rng=random.Random(5)), D.DeviceTrainAugmentThreeMaps(rng=random.Random(5))
    assert [a._draw(1024, 2048) for _ in range(3)] == [b._draw(1024, 2048) for _ in range(3)]
    a = types.SimpleNamespace(src_dataset='cityscapes', active_mode='region', loader='region_cityscapes_or_tensor_ignore_async', or_labeling=True,
                              load_smaller_spx=True, nseg=64, small_nseg=128, ignore_idx=255)
    with pytest.raises(NotImplementedError, match="rescale_769_multi_notrg_ignore"):
        dataloader.get_active_dataset(a, train_transform='rescale_769_multi_notrg')


def test_error_codes_of_the_device_entry_points():
    """Every check below answers before anything is launched or any pointer is read, so host memory stands in for device memory."""
    from mulactseg_amd import _lib
    lib = _lib.load()
    codes = _codes()
    v = views(12)
    zw, sw, fw, mw = (torch.from_numpy(v[k]) for k in ('zw', 'spx_w', 'small_w', 'msk_w'))
    z, f, m = (torch.from_numpy(v[k]) for k in ('z', 'small', 'msk'))
    bits = bits_of(v['tgt'][..., :-1])
    mult, any_, wgt = torch.zeros((N, 12, C), dtype=torch.int32), torch.zeros((N, 12), dtype=torch.int32), torch.zeros((N, 12, C))
    acc, grad, fix = torch.zeros(3, dtype=torch.int64), torch.ones(1), torch.zeros(z.shape, dtype=torch.int64)
    need = lib.mas_async_hier_work_bytes(N, S, 12, C, 2)
    work = torch.zeros(need // 8 + 1, dtype=torch.int64)

    def tables(zq=zw.data_ptr(), C=C, spx_dtype=0, small_dtype=0, S=S, Ss=12, mode=2, work_p=work.data_ptr(), nbytes=need, mult_p=mult.data_ptr(),
               any_p=any_.data_ptr(), wgt_p=wgt.data_ptr(), h=HO):
        return lib.mas_async_hier_tables(zq, h, WO, sw.data_ptr(), spx_dtype, fw.data_ptr(), small_dtype, mw.data_ptr(), bits.data_ptr(), N, C, HO,
                                         WO, S, Ss, mode, work_p, nbytes, mult_p, any_p, wgt_p, None)
    assert tables(zq=None) == codes['MAS_ERR_NULL'] and tables(work_p=None) == codes['MAS_ERR_NULL'] and tables(mult_p=None) == codes['MAS_ERR_NULL']
    assert tables(S=0) == codes['MAS_ERR_SHAPE'] and tables(Ss=0) == codes['MAS_ERR_SHAPE'] and tables(h=HO + 1) == codes['MAS_ERR_SHAPE']
    assert tables(C=33) == codes['MAS_ERR_CLASSES']
    assert tables(mode=3) == codes['MAS_ERR_RANGE'] and tables(mode=-1) == codes['MAS_ERR_RANGE'] and tables(mode=4) == codes['MAS_ERR_RANGE']
    assert tables(spx_dtype=7) == codes['MAS_ERR_DTYPE'] and tables(small_dtype=7) == codes['MAS_ERR_DTYPE']
    assert tables(mode=1, wgt_p=None) == codes['MAS_ERR_NULL'] and tables(mode=2, wgt_p=None) == codes['MAS_ERR_NULL']
    assert tables(nbytes=need - 8) == codes['MAS_ERR_WORKSPACE']
    assert tables(mode=2, nbytes=lib.mas_async_hier_work_bytes(N, S, 12, C, 1)) == codes['MAS_ERR_WORKSPACE']      # the mean's sums need more
    assert tables(work_p=work.data_ptr() + 4) == codes['MAS_ERR_ALIGN'] and tables(mult_p=mult.data_ptr() + 2) == codes['MAS_ERR_ALIGN']
    assert tables(any_p=any_.data_ptr() + 2) == codes['MAS_ERR_ALIGN'] and tables(wgt_p=wgt.data_ptr() + 2) == codes['MAS_ERR_ALIGN']

    def fwd(zq=z.data_ptr(), small_dtype=0, Ss=12, wgt_p=wgt.data_ptr(), acc_p=acc.data_ptr(), mult_p=mult.data_ptr(), C=C):
        return lib.mas_async_hier_fwd(zq, 24, 32, f.data_ptr(), small_dtype, m.data_ptr(), mult_p, any_.data_ptr(), wgt_p, N, C, 24, 32, Ss, acc_p,
                                      None, None)

    def bwd(zq=z.data_ptr(), wgt_p=wgt.data_ptr(), grad_p=grad.data_ptr(), fix_p=fix.data_ptr(), acc_p=acc.data_ptr(), Ss=12):
        return lib.mas_async_hier_bwd(zq, 24, 32, f.data_ptr(), 0, m.data_ptr(), mult.data_ptr(), any_.data_ptr(), wgt_p, acc_p, grad_p, N, C, 24,
                                      32, Ss, fix_p, None, None)
    assert fwd(zq=None) == codes['MAS_ERR_NULL'] and fwd(acc_p=None) == codes['MAS_ERR_NULL'] and fwd(mult_p=None) == codes['MAS_ERR_NULL']
    assert fwd(Ss=0) == codes['MAS_ERR_SHAPE'] and fwd(C=1) == codes['MAS_ERR_CLASSES'] and fwd(small_dtype=7) == codes['MAS_ERR_DTYPE']
    assert fwd(wgt_p=wgt.data_ptr() + 2) == codes['MAS_ERR_ALIGN'] and fwd(acc_p=acc.data_ptr() + 4) == codes['MAS_ERR_ALIGN']
    assert fwd(wgt_p=None, mult_p=mult.data_ptr() + 2) == codes['MAS_ERR_ALIGN']
    assert bwd(grad_p=None) == codes['MAS_ERR_NULL'] and bwd(fix_p=None) == codes['MAS_ERR_NULL'] and bwd(zq=None) == codes['MAS_ERR_NULL']
    assert bwd(Ss=0) == codes['MAS_ERR_SHAPE'] and bwd(wgt_p=wgt.data_ptr() + 2) == codes['MAS_ERR_ALIGN']
    assert bwd(acc_p=acc.data_ptr() + 4) == codes['MAS_ERR_ALIGN']
    assert lib.mas_async_hier_value(None, None, None) == codes['MAS_ERR_NULL']

    # the map-only augmentation entry: a 6 x 8 picture scaled to 12 x 16, padded by (2, 3), crop 10 x 12
    xi, yi = torch.zeros(16, dtype=torch.int32), torch.zeros(12, dtype=torch.int32)
    src, dst = torch.zeros((6, 8), dtype=torch.int32), torch.zeros((10, 12), dtype=torch.int64)

    def maps(H=6, xidx=xi.data_ptr(), crop_i=0, crop_j=0, out_h=10, map0=src.data_ptr(), dtype0=1, out0=dst.data_ptr(), map1=None, dtype1=0,
             out1=None, gap_y=2):
        return lib.mas_train_augment_maps(H, 8, 12, 16, xidx, yi.data_ptr(), gap_y, 3, crop_i, crop_j, 0, out_h, 12, map0, dtype0, 48, out0, 0, map1,
                                          dtype1, 0, out1, 0, None)
    assert maps(map0=None, out0=None) == codes['MAS_ERR_NULL']                     # no map at all
    assert maps(xidx=None) == codes['MAS_ERR_NULL'] and maps(out0=None) == codes['MAS_ERR_NULL']
    assert maps(map1=src.data_ptr()) == codes['MAS_ERR_NULL']                      # a second map without an output
    assert maps(H=0) == codes['MAS_ERR_SHAPE'] and maps(out_h=0) == codes['MAS_ERR_SHAPE']
    assert maps(crop_i=7) == codes['MAS_ERR_RANGE'] and maps(crop_j=11) == codes['MAS_ERR_RANGE']      # the crop leaves the padded picture
    assert maps(crop_i=-1) == codes['MAS_ERR_RANGE'] and maps(gap_y=-1) == codes['MAS_ERR_RANGE']
    assert maps(dtype0=9) == codes['MAS_ERR_DTYPE'] and maps(dtype0=-1) == codes['MAS_ERR_DTYPE']
    assert maps(map1=src.data_ptr(), out1=dst.data_ptr(), dtype1=9) == codes['MAS_ERR_DTYPE']


def test_the_weights_own_fixed_point_floor_equals_mas_fix():
    """``mas_ahg_fix(p)`` (csrc/hier_group.h) is ``mas_fix(p, MAS_AHG_WEIGHT_FRAC)`` for every p the softmax can give -- compared by a host
    function of the test library on both ends of the range, every binade in between, random bit patterns in [0, 1 + 2^-23], and the
    inputs that must give 0 (zero, subnormals, negatives)."""
    import ctypes
    from mulactseg_amd import _lib
    _lib.load()
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "libmulactseg_test.so"))
    lib.mas_test_ahg_fix.restype = ctypes.c_int
    lib.mas_test_ahg_fix.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    top = np.float32(1.0) + np.float32(2.0 ** -23)
    rs = np.random.RandomState(0)
    bits = np.concatenate([
        rs.randint(0, int(top.view(np.uint32)) + 1, size=200000).astype(np.uint32),                              # uniform over the bit patterns
        (np.arange(1, 128, dtype=np.uint32)[:, None] << 23 | np.array([0, 1, 0x400000, 0x7fffff], np.uint32)[None, :]).ravel(),  # binade ends
        np.array([0, 1, 0x7fffff, 0x800000, 0x80000000, 0xbf800000], np.uint32)])                                # 0, subnormals, FLT_MIN, -0, -1
    p = np.concatenate([bits.view(np.float32), rs.uniform(0.0, 1.0, size=100000).astype(np.float32), np.array([1.0, top], np.float32)])
    own, general = np.zeros(p.size, np.uint64), np.zeros(p.size, np.uint64)
    assert lib.mas_test_ahg_fix(p.ctypes.data, p.size, own.ctypes.data, general.ctypes.data) == 0
    assert np.array_equal(own, general)
    ok = (p >= np.float32(1.17549435e-38)) & (p <= top)
    assert np.array_equal(own[ok], np.floor(p[ok].astype(np.float64) * 2.0 ** 40).astype(np.uint64))             # exact in float64
    assert not own[~ok & ~(p > top)].any() and int(own[ok].max()) == 2 ** 40 + 2 ** 17          # (p in (top, 2) agrees too, above)
