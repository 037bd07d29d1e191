"""The hierarchical group term without a GPU: csrc/hier_group.h through the library's host loop (``ops.hier_group_loss_reference``)
against a float64 numpy restatement written here from the formula, and against the executed reference
(tests/golden/g19_hier_group.npz) at the tolerance tests/test_wgroup_cpu.py uses for the same quantities -- 1e-5 * |restated| for the
loss against float64, 1e-4 * max(1, |ref|) for loss values and 1e-4 * max|ref| for gradients against the executed reference; counts and
the pair table exactly -- plus the corner cases, the parser rules, the trainer module and the ABI tables."""
import os
import re
import types

import numpy as np
import pytest
import torch

from test_losses_gpu import _inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EPS = 1e-8
BASE = ['-m', 'deeplabv3pluswn_resnet50deepstem', '--nseg', '64', '-p', '/tmp/x']
# (N, C, H, W, S, Ss): the golden shape with a fine and a coarse second map, the non-integer-scale shape of the GPU test, a small one
SHAPES = [(2, 20, 40, 44, 48, 192), (2, 20, 40, 44, 48, 12), (2, 21, 33, 37, 150, 40), (1, 7, 24, 36, 16, 30)]


def _ops():
    from mulactseg_amd import ops
    return ops


def small_map(seed, spx, S, Ss):
    """The fine maps of a batch: ``synth.superpixel_map(seed * 23 + i, H, W, Ss)`` with the pad pixels (id ``S`` in ``spx``) set to Ss."""
    from mulactseg_amd import synth
    N, H, W = spx.shape
    out = np.stack([synth.superpixel_map(seed * 23 + i, H, W, Ss) for i in range(N)])
    out[spx == S] = Ss
    return out


def with_last_column(tgt):
    """[N,S,C] -> [N,S,C+1] with a zero last column (the "undefined" column both terms drop)."""
    return np.concatenate([tgt, np.zeros(tgt.shape[:2] + (1,), np.uint8)], axis=2)


def cleared_rows(tgt, spx, S):
    """A copy of ``tgt`` with the rows of every id in [0, S) on the outermost rows and columns cleared (--nocropsp)."""
    out = tgt.copy()
    for i in range(spx.shape[0]):
        edge = np.unique(np.concatenate([spx[i, :, 0], spx[i, 0, :], spx[i, -1, :], spx[i, :, -1]]))
        out[i, edge[(edge >= 0) & (edge < S)]] = 0
    return out


def bits_of(rows):
    """int32 [N,S] bit masks of u8 rows [N,S,C]."""
    v = (rows.astype(np.int64) << np.arange(rows.shape[-1], dtype=np.int64)).sum(-1)
    return torch.from_numpy(np.where(v >= 2 ** 31, v - 2 ** 32, v).astype(np.int32))


def restated(z, tgt, spx, small, msk, Ss, only_single, nocropsp=False, upstream=1.0):
    """The term in float64, from the formula.  ``tgt`` [N,S,C+1] (last column dropped).  Returns a dict: loss, n, mult int64
    [N,Ss,C], grad (of upstream * loss, float64 [N,C,H,W]), gap (the smallest relative distance, over the counted pairs, between the
    maximum and the largest probability of a selected pixel of the superpixel that lies in ANOTHER fine superpixel)."""
    N, C, H, W = z.shape
    S = tgt.shape[1]
    rows_all = cleared_rows(tgt, spx, S) if nocropsp else tgt
    x = z.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).transpose(0, 2, 3, 1).reshape(N, H * W, C)
    mult = np.zeros((N, Ss, C), dtype=np.int64)
    gap = np.inf
    for i in range(N):
        sel = np.nonzero(np.asarray(msk[i]).astype(bool).reshape(-1))[0]
        ids, sm = spx[i].reshape(-1)[sel], small[i].reshape(-1)[sel]
        for s in np.unique(ids):
            if s < 0 or s >= S:
                continue
            y = rows_all[i, s, :C]
            if int(y.sum()) <= (1 if only_single else 0):
                continue
            mine = np.nonzero(ids == s)[0]
            for c in np.nonzero(y)[0]:
                col = p[i, sel[mine], c]
                k = int(np.argmax(col))                     # the first maximum in row-major order
                fine = sm[mine[k]]
                other = col[sm[mine] != fine]
                if other.size:
                    gap = min(gap, (col[k] - other.max()) / col[k])
                if 0 <= fine < Ss:
                    mult[i, fine, c] += 1
    total, n = 0.0, 0
    counted = []
    for i in range(N):
        for pix in np.nonzero(np.asarray(msk[i]).astype(bool).reshape(-1))[0]:
            f = small[i].reshape(-1)[pix]
            if not (0 <= f < Ss) or not mult[i, f].any():
                continue
            w = mult[i, f].astype(np.float64)
            total += float((w * -np.log(p[i, pix] + EPS)).sum())
            n += int(mult[i, f].sum())
            counted.append((i, pix, w))
    grad = np.zeros((N, H * W, C))
    a = upstream / (1 + n)
    for i, pix, w in counted:
        r = p[i, pix] / (p[i, pix] + EPS)
        grad[i, pix] = a * (p[i, pix] * (w * r).sum() - w * r)
    return dict(loss=total / (1 + n), n=n, mult=mult, gap=gap, grad=grad.reshape(N, H, W, C).transpose(0, 3, 1, 2))


def restated_pos(z, rows, spx, msk, temp):
    """The merged-positive CE (reference utils/loss.py:535-588) in float64 on the class columns ``rows`` [N,S,C]: (loss, count)."""
    N, C, H, W = z.shape
    x = z.astype(np.float64) / temp
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).transpose(0, 2, 3, 1).reshape(N, H * W, C)
    total, n = 0.0, 0
    for i in range(N):
        sel = np.asarray(msk[i]).astype(bool).reshape(-1)
        y = rows[i][spx[i].reshape(-1)[sel]].astype(np.float64)
        keep = y.any(axis=1)
        total += float(-np.log((p[i][sel][keep] * y[keep]).sum(axis=1) + EPS).sum())
        n += int(keep.sum())
    return total / (1 + n), n


_CASES = {}


def case(shape):
    """(z, tgt [N,S,C+1], spx, small, msk) of a shape, made once."""
    if shape not in _CASES:
        N, C, H, W, S, Ss = shape
        z, tgt, spx, msk = _inputs(300 + W + C, N, C, H, W, S)
        _CASES[shape] = (z, with_last_column(tgt), spx, small_map(300 + W + C, spx, S, Ss), msk)
    return _CASES[shape]


def golden_case(Ss):
    g = np.load(os.path.join(GOLDEN, "g19_hier_group.npz"))
    N, C, H, W, S = (int(g[k]) for k in 'NCHWS')
    z, tgt, spx, msk = _inputs(int(g['seed']), N, C, H, W, S)
    return g, z, with_last_column(tgt), spx, small_map(int(g['seed']), spx, S, Ss), msk


def host(z, tgt, spx, small, msk, Ss, only_single=False, nocropsp=False, upstream=None, size=None, dtype=np.int64):
    ops = _ops()
    grad = None if upstream is None else torch.tensor([upstream], dtype=torch.float32)
    return ops.hier_group_loss_reference(torch.from_numpy(z), size, torch.from_numpy(spx), torch.from_numpy(small.astype(dtype)), Ss,
                                         torch.from_numpy(msk), bits_of(tgt[..., :-1]), only_single=only_single, nocropsp=nocropsp, grad=grad)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("only_single", [False, True])
@pytest.mark.parametrize("nocropsp", [False, True])
def test_the_host_loop_matches_the_float64_restatement(shape, only_single, nocropsp):
    z, tgt, spx, small, msk = case(shape)
    Ss = shape[-1]
    r = restated(z, tgt, spx, small, msk, Ss, only_single, nocropsp, upstream=16.0)
    out = host(z, tgt, spx, small, msk, Ss, only_single, nocropsp, upstream=16.0)
    err = abs(float(out['loss']) - r['loss'])
    print("hier %s single %s nocropsp %s: loss %.7g restated %.7g n %d error %.3e bound %.3e gap %.3e"
          % (shape, only_single, nocropsp, float(out['loss']), r['loss'], r['n'], err, 1e-5 * abs(r['loss']), r['gap']))
    assert r['gap'] > 1e-5                       # no arg-pixel decision that matters is near its edge
    assert int(out['acc'][1]) == r['n'] > 0
    assert np.array_equal(out['mult'].numpy().astype(np.int64), r['mult'])
    assert np.array_equal(out['any'].numpy().astype(np.int64) & 0xffffffff,
                          ((r['mult'] > 0).astype(np.int64) << np.arange(shape[1])).sum(-1))
    assert err <= 1e-5 * abs(r['loss'])
    gerr, scale = float(np.max(np.abs(out['dz'].numpy() - r['grad']))), float(np.max(np.abs(r['grad'])))
    print("   gradient: max error %.3e of max|ref| %.3e" % (gerr, scale))
    assert scale > 0 and gerr <= 1e-4 * scale


@pytest.mark.parametrize("Ss", [192, 12])
@pytest.mark.parametrize("key", ['hier_all', 'hier_single', 'aug_all', 'aug_single'])
def test_the_host_loop_matches_the_executed_reference(Ss, key):
    """Measured when the golden was recorded: the executed reference (float32 torch on the CPU) lies within 9.1e-8 relative of the
    float64 restatement for the loss and within 2.3e-7 of max|grad| for the gradient in all eight cases -- far below the 1e-4 of
    tests/test_wgroup_cpu.py, which therefore is the tolerance here."""
    g, z, tgt, spx, small, msk = golden_case(Ss)
    aug, single = key.startswith('aug'), key.endswith('single')
    k = "%s_%d" % (key, Ss)
    w = float(g['weight'])
    r = restated(z, tgt, spx, small, msk, Ss, single, aug)
    assert r['gap'] > 1e-5                       # the cap on excluded entries is zero
    out = host(z, tgt, spx, small, msk, Ss, single, aug, upstream=w)
    ref, gref = float(g[k + '_loss']), g[k + '_grad']
    print("g19 %s: n %d (golden %d, restated %d), loss %.7g golden %.7g restated %.7g, gap %.3e"
          % (k, int(out['acc'][1]), int(g[k + '_n']), r['n'], float(out['loss']), ref, r['loss'], r['gap']))
    assert int(out['acc'][1]) == int(g[k + '_n']) == r['n'] > 0
    assert np.array_equal(out['mult'].numpy().astype(np.int64), r['mult'])
    assert abs(float(out['loss']) - ref) <= 1e-4 * max(1.0, abs(ref))
    err, scale = float(np.max(np.abs(out['dz'].numpy() - gref))), float(np.max(np.abs(gref)))
    print("g19 %s gradient: max error %.3e of max|ref| %.3e" % (k, err, scale))
    assert scale > 0 and err <= 1e-4 * scale


def test_the_golden_holds_the_issues_counts_and_multiplicities():
    g = np.load(os.path.join(GOLDEN, "g19_hier_group.npz"))
    counts = {192: (229, 148, 116, 43), 12: (1381, 769, 779, 180)}
    for Ss, want in counts.items():
        got = tuple(int(g["%s_%d_n" % (k, Ss)]) for k in ('hier_all', 'hier_single', 'aug_all', 'aug_single'))
        assert got == want, (Ss, got)
    assert int(g['max_mult_192']) == 1 and int(g['max_mult_12']) >= 2
    assert int(g['rows_changed']) == 40 and int(g['pos_n']) == 692 and int(g['aug_pos_n']) == 468


def test_nocropsp_drops_the_cleared_rows_from_both_terms_and_keeps_the_callers_tensor():
    g, z, tgt, spx, small, msk = golden_case(12)
    S, C = tgt.shape[1], z.shape[1]
    before = tgt.copy()
    bits = bits_of(tgt[..., :-1])
    bits_before = bits.clone()
    ops = _ops()
    out = ops.hier_group_loss_reference(torch.from_numpy(z), None, torch.from_numpy(spx), torch.from_numpy(small), 12, torch.from_numpy(msk),
                                        bits, nocropsp=True)
    assert np.array_equal(tgt, before) and torch.equal(bits, bits_before)
    cleared = cleared_rows(tgt, spx, S)
    assert torch.equal(out['bits_eff'], bits_of(cleared[..., :-1]))
    assert int((cleared != tgt).any(axis=2).sum()) == int(g['rows_changed'])
    # the group term: equal to the plain term on the cleared rows
    plain = host(z, cleared, spx, small, msk, 12)
    assert torch.equal(out['acc'], plain['acc']) and torch.equal(out['mult'], plain['mult'])
    # the merged-positive term on bits_eff: the recorded loss and count of the reference on the labels it modified
    T = float(g['pos_temp'])
    losses, acc = ops.partial_loss_reference(torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(msk), out['bits_eff'],
                                             ops.inv_temperature(T), 1)
    rl, rn = restated_pos(z, cleared[..., :C], spx, msk, T)
    assert int(acc[2]) + int(acc[3]) == int(g["aug_pos_n"]) == rn           # (one-hot + multi-hot pixels)
    assert abs(float(losses[0]) - float(g['aug_pos_loss'])) <= 1e-4 * max(1.0, abs(float(g['aug_pos_loss'])))
    losses0, acc0 = ops.partial_loss_reference(torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(msk), bits, ops.inv_temperature(T), 1)
    assert int(acc0[2]) + int(acc0[3]) == int(g["pos_n"]) > rn


def test_the_temperature_argument_changes_nothing():
    from mulactseg_amd.utils import loss as L
    args = types.SimpleNamespace(small_nseg=12)
    a = L.HierGroupMultiLabelCE(args, 20, 48, False, -1, temperature=0.1)
    b = L.HierGroupMultiLabelCE(args, 20, 48, False, -1)
    assert a.temp == b.temp == 1.0
    header = open(os.path.join(ROOT, "include", "mulactseg_hip.h")).read()
    for name in ('mas_hier_group_fwd', 'mas_hier_group_bwd', 'mas_hier_group_reference'):
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert 'invT' not in decl and 'float ' not in decl.replace('const float*', '').replace('float*', '')


def test_corner_cases_contribute_nothing_and_stay_finite():
    z, tgt, spx, small, msk = (a.copy() for a in case(SHAPES[1]))
    Ss = SHAPES[1][-1]
    whole = host(z, tgt, spx, small, msk, Ss, upstream=1.0)
    # a picture with no selected pixel
    m2 = msk.copy()
    m2[1] = False
    one = host(z, tgt, spx, small, m2, Ss, upstream=1.0)
    alone = host(z[:1], tgt[:1], spx[:1], small[:1], msk[:1], Ss, upstream=1.0)
    assert torch.equal(one['acc'], alone['acc']) and int(one['mult'][1].sum()) == 0 and not bool(one['dz'][1].any())
    # no selected pixel at all: zero, finite
    none = host(z, tgt, spx, small, np.zeros_like(msk), Ss, upstream=1.0)
    assert int(none['acc'][0]) == 0 and int(none['acc'][1]) == 0 and float(none['loss']) == 0.0 and not bool(none['dz'].any())
    # rows with no bit: the superpixels of picture 0 lose their rows
    t2 = tgt.copy()
    t2[0] = 0
    empty = host(z, t2, spx, small, msk, Ss, upstream=1.0)
    assert int(empty['mult'][0].sum()) == 0 and not bool(empty['dz'][0].any()) and torch.equal(empty['mult'][1], whole['mult'][1])
    # small == small_nseg on selected pixels: they are not counted, and an arg-pixel there gives no pair
    s2 = small.copy()
    s2[0][msk[0].astype(bool)] = Ss
    pad = host(z, tgt, spx, s2, msk, Ss, upstream=1.0)
    assert int(pad['mult'][0].sum()) == 0 and not bool(pad['dz'][0].any()) and torch.equal(pad['mult'][1], whole['mult'][1])
    for out in (whole, one, none, empty, pad):
        assert bool(torch.isfinite(out['loss']).all()) and bool(torch.isfinite(out['dz']).all())


def test_the_id_dtypes_agree_and_an_unknown_one_is_refused():
    z, tgt, spx, small, msk = case(SHAPES[3])
    Ss = SHAPES[3][-1]
    a = host(z, tgt, spx, small, msk, Ss, upstream=1.0)
    b = host(z, tgt, spx, small, msk, Ss, upstream=1.0, dtype=np.int32)
    assert torch.equal(a['acc'], b['acc']) and torch.equal(a['mult'], b['mult']) and torch.equal(a['dzq_fix'], b['dzq_fix'])
    with pytest.raises(TypeError):
        host(z, tgt, spx, small, msk, Ss, dtype=np.uint8)


def test_error_codes_of_the_reference_entry_point():
    from mulactseg_amd import _lib
    lib = _lib.load()
    z, tgt, spx, small, msk = case(SHAPES[3])
    N, C, H, W, S, Ss = SHAPES[3]
    zc, sc, fc, mc = torch.from_numpy(z), torch.from_numpy(spx), torch.from_numpy(small), torch.from_numpy(msk).view(torch.uint8)
    bits = bits_of(tgt[..., :-1])
    mult, any_ = torch.zeros((N, Ss, C), dtype=torch.int32), torch.zeros((N, Ss), dtype=torch.int32)
    acc = torch.zeros(3, dtype=torch.int64)

    def call(zq=zc.data_ptr(), C=C, small_dtype=0, flags=0, mult_p=mult.data_ptr(), acc_p=acc.data_ptr(), Ss=Ss):
        return lib.mas_hier_group_reference(zq, H, W, sc.data_ptr(), 0, fc.data_ptr(), small_dtype, mc.data_ptr(), bits.data_ptr(), N, C, H, W, S,
                                            Ss, flags, None, None, None, mult_p, any_.data_ptr(), acc_p, None, None)
    codes = {}
    for line in open(os.path.join(ROOT, "mulactseg_amd", "csrc", "common.h")):
        m = re.match(r"#define (MAS_ERR_\w+)\s+\(?(-?\d+)\)?", line)
        if m:
            codes[m.group(1)] = int(m.group(2))
    assert call() == 0
    assert call(zq=None) == codes['MAS_ERR_NULL']
    assert call(C=33) == codes['MAS_ERR_CLASSES']
    assert call(small_dtype=7) == codes['MAS_ERR_DTYPE']
    assert call(flags=4) == codes['MAS_ERR_RANGE']
    assert call(flags=2) == codes['MAS_ERR_NULL']               # --nocropsp without a place for the cleared table
    assert call(Ss=0) == codes['MAS_ERR_SHAPE']
    assert call(mult_p=mult.data_ptr() + 2) == codes['MAS_ERR_ALIGN']
    assert call(acc_p=acc.data_ptr() + 4) == codes['MAS_ERR_ALIGN']


def test_arg_assert_rules():
    from mulactseg_amd.utils import common
    p = common.get_parser()
    d = p.parse_args(BASE)
    assert d.nocropsp is False and d.gumbel_scale == -1

    def check(method, extra):
        a = p.parse_args(BASE + extra)
        a.method, a.init_checkpoint, a.trg_datalist, a.region_dict = method, 'x.tar', 'seed64.txt', 'seed64.dict'
        a.datalist_path = a.resume_checkpoint = None
        common.arg_assert(a)
        return a
    hier = 'active_joint_hier_multi'
    a = check(hier, ['--load_smaller_spx', '--group_only_single', '--nocropsp'])
    assert a.group_only_single is True and a.nocropsp is True
    check(hier, ['--load_smaller_spx'])
    with pytest.raises(ValueError, match="load_smaller_spx"):
        check(hier, [])
    with pytest.raises(NotImplementedError, match="gumbel_scale"):
        check(hier, ['--load_smaller_spx', '--gumbel_scale', '0.5'])
    for method in ('active_joint_multi_predignore', 'active_joint_multi_predignore_wgroup'):
        with pytest.raises(NotImplementedError, match="nocropsp"):
            check(method, ['--nocropsp'])
        with pytest.raises(NotImplementedError, match="gumbel_scale"):
            check(method, ['--gumbel_scale', '0.5'])
    with pytest.raises(NotImplementedError, match="group_only_single"):
        check('active_joint_multi_predignore', ['--group_only_single'])


def test_the_constructor_refuses_gumbel_noise():
    from mulactseg_amd.utils import loss as L
    args = types.SimpleNamespace(small_nseg=12)
    for cls in (L.HierGroupMultiLabelCE, L.AugHierGroupMultiLabelCE):
        with pytest.raises(NotImplementedError, match="gumbel"):
            cls(args, 19, 48, False, 0.5)
        m = cls(args, 19, 48, True, -1, reduction='none', temperature=0.1)
        assert m.only_single is True and m.num_small_superpixel == 12 and m.reduction == 'none'
    assert L.AugHierGroupMultiLabelCE._nocropsp and not L.HierGroupMultiLabelCE._nocropsp


def test_the_trainer_module_builds_its_criterion():
    from mulactseg_amd.trainer import active, active_joint_hier_multi as mod
    from mulactseg_amd.utils import loss as L
    assert issubclass(mod.ActiveTrainer, active.ActiveTrainer) and not mod.ActiveTrainer.predicts_ignore
    for nocropsp, cls in ((False, L.HierGroupMultiLabelCE), (True, L.AugHierGroupMultiLabelCE)):
        tr = types.SimpleNamespace(args=types.SimpleNamespace(nseg=64, small_nseg=256, group_ce_temp=0.1, multi_ce_temp=0.1, group_only_single=True,
                                                              nocropsp=nocropsp, gumbel_scale=-1), num_classes=19)
        mod.ActiveTrainer.get_criterion(tr)
        assert type(tr.hier_group_multi_loss) is cls and tr.hier_group_multi_loss.only_single and tr.hier_group_multi_loss.temp == 1.0
        assert type(tr.multi_pos_loss) is L.MultiChoiceCE and tr.multi_pos_loss.temp == 0.1
    tr.args.gumbel_scale = 0.5
    with pytest.raises(NotImplementedError):
        mod.ActiveTrainer.get_criterion(tr)


def test_the_transform_pads_the_two_maps():
    from mulactseg_amd.dataloader import get_train_transform
    t = get_train_transform(types.SimpleNamespace(ignore_idx=255, nseg=2048, small_nseg=8192, load_smaller_spx=True), 'rescale_769_multi_notrg')
    assert t.n_maps == 2 and t.pad_values == [2048, 8192]
    t = get_train_transform(types.SimpleNamespace(ignore_idx=255, nseg=2048, small_nseg=8192, load_smaller_spx=False), 'rescale_769_multi_notrg')
    assert t.n_maps == 1 and t.pad_values == [2048]
    for name in ('rescale_769_multi', 'rescale_769_multi_notrg_ignore'):
        with pytest.raises(NotImplementedError):
            get_train_transform(types.SimpleNamespace(ignore_idx=255, nseg=2048, small_nseg=8192, load_smaller_spx=True), name)


def test_header_exports_and_ctypes_table_agree():
    from mulactseg_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mulactseg_hip.h")).read()
    makefile = open(os.path.join(ROOT, "mulactseg_amd", "csrc", "Makefile")).read()
    assert re.search(r"online_plbl\.o:.*hier_group\.h", makefile)
    for name in ('mas_hier_group_fwd', 'mas_hier_group_value', 'mas_hier_group_bwd', 'mas_hier_group_reference'):
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(',') if a.strip()])
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert (_lib.HIER_ONLY_MULTI, _lib.HIER_NOCROPSP) == tuple(int(re.search(r"#define %s (\d+)" % k, header).group(1))
                                                              for k in ('MAS_HIER_ONLY_MULTI', 'MAS_HIER_NOCROPSP'))
