"""The four stage-2 generators without expansion against the EXECUTED reference (tests/golden/g12_stage2_variants.npz, written by
tools/gen_golden_stage2_variants.py from the reference's own inference() loops): the numpy restatement of csrc/candidate_plbl.hip, the
ATen chain of ``ops.candidate_pseudo_labels`` on CPU tensors, the counters as table strings, the argument checks and the trainer
plugins' plumbing.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import candidate_plbl_restated as CR
from test_oracle_golden import digest, stage2_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALLBACK_TAGS = ('naiveprop', 'candprop')
MARGIN = 1e-6                   # the margin of tests/test_naive_plbl_gpu.py:70 around the threshold
SET_ASIDE = 1e-3                # at most 0.1 % of the pixels may lie within it


@pytest.fixture(scope="module")
def g12():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_stage2_variants.npz"))
    feats, z, tgt, spx, msk, labels = stage2_inputs(int(g['seed']), int(g['N']), int(g['C']), int(g['Ch']), int(g['H']), int(g['W']), int(g['S']))
    assert digest(feats, z, tgt, spx, msk) == g['input_digest'] and digest(labels) == g['labels_digest']
    return types.SimpleNamespace(g=g, feats=feats, z=z, tgt=tgt, spx=spx, msk=msk, labels=labels, settings=[tuple(s) for s in g['settings']],
                                 p64={T: CR.pmax64(z, float(CR.inv_temperature(T))) for T in {s[1] for s in g['settings']}})


def cases(g12):
    """(key, fallback, th, ce_temp, candidate mode) of every stored map but eval_save_cosplbl's own."""
    out = [('candidate', False, 0.0, 1.0, True)]
    for tag in FALLBACK_TAGS:
        out += [('%s_%d' % (tag, k), True, th, T, tag == 'candprop') for k, (th, T) in enumerate(g12.settings)]
    return out


def assert_maps_equal(got, want, g12, fallback, th, T):
    """Exact, except unselected pixels whose float64 p_max lies within MARGIN of the threshold -- at most SET_ASIDE of the pixels."""
    far = np.ones(want.shape, dtype=bool)
    if fallback:
        far = g12.msk | (np.abs(g12.p64[T] - th) > MARGIN)
    assert (~far).mean() <= SET_ASIDE
    assert np.array_equal(np.asarray(got)[far], want.astype(np.int64)[far])


def test_the_fixture_holds_what_the_issue_describes(g12):
    g, unq = g12.g, ~g12.msk
    assert not g12.msk[2].any() and g12.msk[:2].any()
    kept = [float((g['plbl_candprop_%d' % k][unq] != 255).mean()) for k in range(3)]
    assert kept[0] == 1.0 and 0.40 < kept[1] < 0.46 and 0.26 < kept[2] < 0.31
    assert (g['plbl_candidate'][unq] == 255).all() and (g['plbl_cosplbl'][unq] == 255).all()
    assert (g['plbl_candidate'][g12.msk] != 255).all() and (g['plbl_cosplbl'][g12.msk] != 255).all()
    # the quirk: selected pixels whose candidate logits are all negative carry the first excluded channel
    lab = g['plbl_candidate'].astype(np.int64)
    rows = g12.tgt[np.arange(3)[:, None, None], g12.spx]
    outside = g12.msk & (np.take_along_axis(rows, np.minimum(lab, 19)[..., None], axis=3)[..., 0] == 0)
    assert 0.3 < outside.sum() / g12.msk.sum() < 0.42
    assert str(g['dir_candprop_0']) == 'plbl_gen_wcand' and str(g['dir_candidate']) == 'plbl_gen' and str(g['dir_naiveprop_1']) == 'plbl_gen'
    for T in g12.p64:                                    # the inputs use none of the allowance
        for th, T2 in g12.settings:
            if T2 == T:
                assert not (np.abs(g12.p64[T][unq] - th) <= MARGIN).any()


def test_assignment_without_expansion_is_the_expanding_generator_under_the_mask(g12):
    """eval_save_cosplbl against the oracle of the expanding generator (every selected pixel valid): the last two lines of the expanding
    loop overwrite every masked pixel with its own superpixel's assignment."""
    from oracle import exact
    want = np.where(g12.msk, exact.stage2_pseudo_labels(g12.feats, g12.z, g12.tgt, g12.msk, g12.spx, True), 255)
    assert np.array_equal(want, g12.g['plbl_cosplbl'].astype(np.int64))
    g6 = np.load(os.path.join(ROOT, "tests", "golden", "g6_stage2.npz"))
    assert np.array_equal(np.where(g12.msk, g6['plbl_all'], 255), g12.g['plbl_cosplbl'].astype(np.int64))
    nn, p_cls = np.array([-1, 2, 0, -1, 1]), np.array([7, 19, 3])
    assert CR.assign_labels(nn, p_cls).tolist() == [255, 3, 7, 255, 19]


def test_restatement_reproduces_the_executed_reference(g12):
    H, W = g12.z.shape[2:]
    for key, fallback, th, T, cand in cases(g12):
        kw = dict(rows=g12.tgt, spx=g12.spx) if cand else dict(inner=g12.g['plbl_cosplbl'].astype(np.int64))
        got = CR.labels(g12.z, H, W, g12.msk, fallback=fallback, th=th, inv_T=CR.inv_temperature(T), **kw)
        assert_maps_equal(got, g12.g['plbl_' + key], g12, fallback, th, T)


def test_restatement_edge_cases():
    """The literal product: +-0 for an excluded channel (so all-negative candidates lose to the first excluded channel), NaN for an
    infinity times 0 and for a NaN, the first NaN wins; an id outside the rows gives 255; map mode narrows to u8; th = 0 keeps all."""
    z = np.array([[-1.0, -2.0, -3.0], [1.0, 5.0, 2.0], [0.5, np.inf, 0.1], [0.5, np.nan, 9.0], [3.0, 1.0, 2.0]], dtype=np.float32)
    z = z.T.reshape(1, 3, 1, 5).copy()
    rows = np.array([[[1, 1, 0], [1, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 0]]], dtype=np.uint8)
    spx = np.array([[[0, 1, 2, 3, 5]]], dtype=np.int64)
    mask = np.ones((1, 1, 5), dtype=bool)
    got = CR.labels(z, 1, 5, mask, rows=rows, spx=spx)
    assert got.tolist() == [[[2, 2, 1, 1, 255]]]
    inner = np.array([[[3, 255, 256 + 7, 0, 1]]], dtype=np.int64)
    assert CR.labels(z, 1, 5, mask, inner=inner).tolist() == [[[3, 255, 7, 0, 1]]]
    none = np.zeros((1, 1, 5), dtype=bool)
    assert CR.labels(z, 1, 5, none, inner=inner).tolist() == [[[255] * 5]]
    # (a NaN gives 255, and so does +inf: inf - inf is a NaN)
    assert CR.labels(z, 1, 5, none, inner=inner, fallback=True, th=0.0).tolist() == [[[0, 1, 255, 255, 0]]]
    assert CR.labels(z, 1, 5, none, inner=inner, fallback=True, th=0.9).tolist() == [[[255, 1, 255, 255, 255]]]


def _call(ops, g12, key, fallback, th, T, cand, **extra):
    t = torch.from_numpy
    kw = dict(targets_rows=t(g12.tgt), superpixels=t(g12.spx)) if cand else dict(inner=t(g12.g['plbl_cosplbl'].astype(np.int64)))
    return ops.candidate_pseudo_labels(t(g12.z), g12.z.shape[2:], t(g12.msk), fallback=fallback, th=th, ce_temp=T, **kw, **extra)


def test_ops_on_cpu_tensors_equal_the_executed_reference_and_its_tables(g12):
    from mulactseg_amd import ops
    K = 20
    for key, fallback, th, T, cand in cases(g12):
        counts = torch.zeros(3 * K + 3, dtype=torch.int64)
        got = _call(ops, g12, key, fallback, th, T, cand, targets=torch.from_numpy(g12.labels), counts=counts, num_classes=K)
        assert got.dtype == torch.int64 and tuple(got.shape) == g12.msk.shape
        assert_maps_equal(got.numpy(), g12.g['plbl_' + key], g12, fallback, th, T)
        assert CR.iou_table(counts.numpy(), K) == str(g12.g['table_' + key])
        assert np.array_equal(counts.numpy(), CR.meaniou_counts(got.numpy(), g12.labels, K))
    counts = ops._meaniou_counts_aten(torch.from_numpy(g12.g['plbl_cosplbl'].astype(np.int64)), torch.from_numpy(g12.labels), K, 255,
                                      torch.zeros(3 * K + 3, dtype=torch.int64))
    assert CR.iou_table(counts.numpy(), K) == str(g12.g['table_cosplbl'])
    assert len(str(g12.g['table_cosplbl']).split(',')) == 1 + K


def test_ops_cpu_chain_upsamples_like_the_reference():
    """A real upsampling on the CPU: F.interpolate, then the reference's lines -- against the restatement away from value ties."""
    from mulactseg_amd import ops
    rs = np.random.RandomState(3)
    zq = (2.0 * rs.randn(1, 20, 8, 12)).astype(np.float32)
    H, W, S = 32, 48, 9
    spx = rs.randint(0, S, size=(1, H, W)).astype(np.int64)
    rows = (rs.uniform(size=(1, S, 20)) < 0.2).astype(np.uint8)
    mask = rs.uniform(size=(1, H, W)) < 0.5
    t = torch.from_numpy
    got = ops.candidate_pseudo_labels(t(zq), (H, W), t(mask), targets_rows=t(rows), superpixels=t(spx), fallback=True, th=0.2).numpy()
    want = CR.labels(zq, H, W, mask, rows=rows, spx=spx, fallback=True, th=0.2)
    y = torch.nn.functional.interpolate(t(zq), size=(H, W), mode='bilinear', align_corners=False).numpy()
    top2 = np.sort(y, axis=1)[:, -2:]
    clear = ((top2[:, 1] - top2[:, 0]) > 1e-4) & (np.abs(CR.pmax64(y) - 0.2) > 1e-4) & (np.abs(y).min(axis=1) > 1e-4)
    assert clear.mean() > 0.95 and np.array_equal(got[clear], want[clear])
    assert 0.05 < (got[~mask] != 255).mean() < 0.95


def test_argument_checks_raise():
    from mulactseg_amd import ops
    z = torch.zeros((1, 20, 8, 8))
    m = torch.ones((1, 16, 16), dtype=torch.bool)
    spx = torch.zeros((1, 16, 16), dtype=torch.int64)
    rows = torch.ones((1, 4, 20), dtype=torch.uint8)
    f = ops.candidate_pseudo_labels
    for kw in (dict(), dict(targets_rows=rows), dict(superpixels=spx), dict(targets_rows=rows, superpixels=spx, inner=spx), dict(inner=spx, superpixels=spx)):
        with pytest.raises(ValueError, match="exactly one"):
            f(z, (16, 16), m, **kw)
    with pytest.raises(ValueError, match="cannot be upsampled"):
        f(z, (4, 4), torch.ones((1, 4, 4), dtype=torch.bool), inner=torch.zeros((1, 4, 4), dtype=torch.int64))      # a downsampling
    with pytest.raises(ValueError, match="cannot be upsampled"):
        f(z, (8, 56), torch.ones((1, 8, 56), dtype=torch.bool), inner=torch.zeros((1, 8, 56), dtype=torch.int64))    # wider than x6
    with pytest.raises(ValueError, match="spmask"):
        f(z, (16, 16), None, inner=spx)
    with pytest.raises(ValueError, match="spmask"):
        f(z, (16, 16), m[:, :8], inner=spx)
    with pytest.raises(ValueError, match="at most 32"):
        f(torch.zeros((1, 33, 8, 8)), (16, 16), m, targets_rows=torch.ones((1, 4, 33), dtype=torch.uint8), superpixels=spx)
    with pytest.raises(ValueError, match="targets_rows"):
        f(z, (16, 16), m, targets_rows=torch.ones((1, 4, 19), dtype=torch.uint8), superpixels=spx)
    with pytest.raises(ValueError, match="superpixels"):
        f(z, (16, 16), m, targets_rows=rows, superpixels=spx[:, :8])
    with pytest.raises(TypeError, match="superpixels"):
        f(z, (16, 16), m, targets_rows=rows, superpixels=spx.int())
    with pytest.raises(TypeError, match="inner"):
        f(z, (16, 16), m, inner=spx.int())
    with pytest.raises(ValueError, match="inner"):
        f(z, (16, 16), m, inner=spx[:, :8])
    with pytest.raises(TypeError, match="logits_q"):
        f(z.double(), (16, 16), m, inner=spx)
    with pytest.raises(ValueError, match="th >= 0"):
        f(z, (16, 16), m, inner=spx, fallback=True, th=-0.1)
    counts = torch.zeros(63, dtype=torch.int64)
    with pytest.raises(ValueError, match="num_classes is required"):
        f(z, (16, 16), m, inner=spx, targets=spx, counts=counts)
    with pytest.raises(ValueError, match="targets are required"):
        f(z, (16, 16), m, inner=spx, counts=counts, num_classes=20)
    with pytest.raises(ValueError, match="counts must be"):
        f(z, (16, 16), m, inner=spx, targets=spx, counts=counts[:60], num_classes=20)
    with pytest.raises(TypeError, match="targets"):
        f(z, (16, 16), m, inner=spx, targets=spx.int(), counts=counts, num_classes=20)
    assert f(z, (16, 16), m, inner=spx, targets=spx, counts=counts, num_classes=20).shape == (1, 16, 16) and int(counts[0]) == 256


def test_stage2_pseudo_labels_takes_the_expand_keyword():
    import inspect
    from mulactseg_amd import _lib, ops
    p = inspect.signature(ops.stage2_pseudo_labels).parameters
    assert p['expand'].default is True and list(p)[-1] == 'expand'
    assert len(_lib.SIGNATURES["mas_stage2_assign_labels"][1]) == 5 and len(_lib.SIGNATURES["mas_candidate_plbl"][1]) == 21
    with open(os.path.join(ROOT, "include", "mulactseg_hip.h")) as f:
        text = f.read()
    assert "int mas_candidate_plbl(" in text and "int mas_stage2_assign_labels(" in text
    with open(os.path.join(ROOT, "mulactseg_amd", "csrc", "Makefile")) as f:
        assert "candidate_plbl.hip" in f.read()


# -- the four trainer plugins --------------------------------------------------------------------------------------------------
NAMES = ('eval_save_cosplbl', 'eval_save_cosplbl_naiveprop', 'eval_save_candidateplbl', 'eval_save_candidateplbl_prop')


def _module(name):
    import importlib
    return importlib.import_module('mulactseg_amd.trainer.' + name)


@pytest.mark.parametrize("name, ptype, want", [(n, None, 'plbl_gen_wcand' if n == 'eval_save_candidateplbl_prop' else 'plbl_gen') for n in NAMES] +
                                              [(n, 'wo_expand', 'plbl_gen_wo_expand') for n in NAMES])
def test_directory_rule(tmp_path, name, ptype, want):
    cls = _module(name).ActiveTrainer
    fake = object.__new__(cls)
    fake.args = types.SimpleNamespace(init_checkpoint='%s/run/checkpoint03.tar' % tmp_path, plbl_type=ptype)
    fake.save_dir = None
    assert fake._save_dir() == '%s/run/%s/round_03' % (tmp_path, want) and os.path.isdir(fake._save_dir())


def test_every_plugin_is_a_threaded_generator_of_the_expanding_family():
    from mulactseg_amd.trainer import eval_save_cosplbl_prop, eval_within_multihot
    for name in NAMES:
        cls = _module(name).ActiveTrainer
        assert issubclass(cls, eval_save_cosplbl_prop.ActiveTrainer) and cls.threaded_generation is True
        assert cls.inference is eval_save_cosplbl_prop.ActiveTrainer.inference and cls.after_batch is eval_save_cosplbl_prop.ActiveTrainer.after_batch
        assert cls.extra_channels == 1
        counts_itself = cls.generate_batch is not eval_within_multihot.ActiveTrainer.generate_batch
        assert counts_itself == (name != 'eval_save_cosplbl')


class _Net:
    lowres_logits = True

    def __init__(self):
        self.calls = []

    def __call__(self, images, lowres=False):
        self.calls.append(('forward', lowres))
        return torch.zeros((1, 20, 4, 8))

    def feat_forward_quarter(self, images):
        self.calls.append(('quarter',))
        return torch.zeros((1, 16, 4, 8)), torch.zeros((1, 20, 4, 8))

    def feat_forward_lowres(self, images):
        self.calls.append(('lowres',))
        return torch.zeros((1, 16, 4, 8)), torch.zeros((1, 20, 16, 32))


def _batch():
    return {'images': torch.zeros((1, 3, 16, 32)), 'labels': torch.zeros((1, 16, 32), dtype=torch.int64),
            'spx': torch.zeros((1, 16, 32), dtype=torch.int64), 'spmask': torch.ones((1, 16, 32), dtype=torch.bool),
            'target': torch.ones((1, 4, 20), dtype=torch.uint8), 'fnames': [('a', 'b/c.png', 'd')]}


@pytest.mark.parametrize("name", NAMES)
def test_the_flags_reach_ops(monkeypatch, name):
    from mulactseg_amd import ops
    from mulactseg_amd.utils.miou import MeanIoU
    seen = {}
    marker = torch.full((1, 16, 32), 7, dtype=torch.int64)

    def stage2(feats, logits, targets, spmasks, superpixels, include_onehot=True, threshold_method='median', expand=True):
        seen['stage2'] = dict(include_onehot=include_onehot, expand=expand, feats=tuple(feats.shape), logits=tuple(logits.shape))
        return marker

    def candidate(logits_q, size, spmask, **kw):
        seen['candidate'] = dict(kw, logits=tuple(logits_q.shape), size=tuple(size))
        return marker + 1
    monkeypatch.setattr(ops, "stage2_pseudo_labels", stage2)
    monkeypatch.setattr(ops, "candidate_pseudo_labels", candidate)
    cls = _module(name).ActiveTrainer
    tr = object.__new__(cls)
    tr.args = types.SimpleNamespace(plbl_th=0.3, ce_temp=0.1, ignore_idx=255)
    tr.net, tr.device, saved = _Net(), 'cpu', []
    tr.after_batch = lambda batch, plbl: saved.append(plbl)
    meter = MeanIoU(20, 255)
    meter._before_epoch()
    if name == 'eval_save_cosplbl':                     # (the inherited loop step: the meter counts the returned map)
        meter._after_step = lambda d: seen.update(counted=d['outputs'])
    tr.generate_batch(_batch(), meter)
    if name == 'eval_save_cosplbl':
        assert seen.pop('counted') is marker
        assert seen['stage2'] == dict(include_onehot=True, expand=False, feats=(1, 16, 4, 8), logits=(1, 20, 16, 32))
        assert 'candidate' not in seen and saved[0] is marker and tr.net.calls == [('lowres',)]
        return
    c = seen['candidate']
    assert c['logits'] == (1, 20, 4, 8) and c['size'] == (16, 32)                   # the network stopped at quarter resolution
    assert c['counts'] is meter._counts and c['num_classes'] == 20 and c['ignore_label'] == 255 and c['targets'].shape == (1, 16, 32)
    assert torch.equal(saved[0], marker + 1)
    if name == 'eval_save_cosplbl_naiveprop':
        assert seen['stage2'] == dict(include_onehot=True, expand=False, feats=(1, 16, 4, 8), logits=(1, 20, 16, 32))
        assert c['inner'] is marker and c['fallback'] is True and (c['th'], c['ce_temp']) == (0.3, 0.1) and 'targets_rows' not in c
        assert tr.net.calls == [('quarter',)]
    else:
        assert 'stage2' not in seen and 'inner' not in c and c['targets_rows'].shape == (1, 4, 20) and c['superpixels'].shape == (1, 16, 32)
        assert c['fallback'] is (name == 'eval_save_candidateplbl_prop') and (c['th'], c['ce_temp']) == (0.3, 0.1)
        assert tr.net.calls == [('forward', True)]
    seen.clear()
    tr.pseudo_labels(*[_batch()[k] for k in ('images', 'labels', 'target', 'spmask', 'spx')])     # without a meter: no counters
    assert 'counts' not in seen['candidate']
