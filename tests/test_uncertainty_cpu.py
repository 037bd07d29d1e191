"""Acquisition measures beyond BvSB (csrc/uncertainty.h, csrc/uncertainty.hip) without a GPU: the library's host entry
``mas_uncertainty_reference`` -- the CPU-side statement of the arithmetic the kernel is compared with bit for bit in
tests/test_uncertainty_gpu.py -- against float64 numpy definitions, the accumulator contract, the six BvSB-family selectors on the
new pass, and the ``--uncertainty`` flag."""
import importlib

import numpy as np
import pytest
import torch

from helpers import FakePool, OracleBackend, fake_trainer, selector_args

MEASURES = ('bvsb', 'margin', 'least_confidence', 'entropy')
NEW_MEASURES = MEASURES[1:]
PREDIGNORE, PLAIN = 'active_joint_multi_predignore_lossdecomp', 'active_joint_multi_lossdecomp'
# (module, num_classes, method): every one reads the tiny pool's 20-channel logits (my_bvsb strips the last channel under predignore)
SELECTORS = (('my_bvsb', 19, PREDIGNORE), ('my_bvsb_banignore', 19, PREDIGNORE), ('my_bvsb_predclsbal_pwr', 20, PLAIN),
             ('my_bvsb_predclsbal_pwr_banignore', 19, PREDIGNORE), ('my_bvsb_clsbal_v2', 20, PLAIN),
             ('my_bvsb_clsbal_v2_banignore', 19, PREDIGNORE))


def ops():
    from mulactseg_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------
# float64 definitions
# ------------------------------------------------------------------------------------------------
def measures_f64(z, invT):
    """z f32 [N, C] -> {measure: f64 [N]}, arg-max [N]: softmax(z * invT) in float64, the table of the measures, + 1e-8."""
    t = z.astype(np.float64) * np.float64(np.float32(invT))
    t -= t.max(axis=1, keepdims=True)
    e = np.exp(t)
    p = e / e.sum(axis=1, keepdims=True)
    top = np.sort(p, axis=1)
    p1, p2 = top[:, -1], top[:, -2]
    with np.errstate(divide='ignore', invalid='ignore'):
        plogp = np.where(p > 0, p * np.log(p), 0.0)
    ent = np.clip(-plogp.sum(axis=1) / np.log(z.shape[1]), 0.0, 1.0)
    return ({'bvsb': p2 / p1 + 1e-8, 'margin': 1.0 - (p1 - p2) + 1e-8, 'least_confidence': 1.0 - p1 + 1e-8, 'entropy': ent + 1e-8},
            np.argmax(z, axis=1))


def per_pixel(z, invT, measure):
    """The host entry through one-pixel regions: (u f64 [N] = the pixel's 40-bit quantum, arg-max [N], prob_sum)."""
    N, C = z.shape
    zt = torch.from_numpy(np.ascontiguousarray(z.T).reshape(1, C, 1, N))
    spx = torch.arange(N, dtype=torch.int32).reshape(1, 1, N)
    ps, cs, hh = ops().uncertainty_reference(zt, spx, N, invT, measure)
    assert int(hh.sum()) == N and bool((hh.sum(-1) == 1).all())
    return cs[0].sum(-1).numpy().astype(np.float64) / 2.0 ** 40, hh[0].argmax(-1).numpy(), ps


def edge_rows(C, invT):
    rows = np.full((3, C), -1.0, dtype=np.float32)
    i, j = (0, 1) if C == 2 else (1, C - 2)
    rows[0, i] = rows[0, j] = 2.5                    # two equal maxima: the first one is the arg-max, p2 / p1 = 1
    rows[1, :] = 0.75                                # all equal: entropy clamps to 1
    rows[2, 0] = rows[2, 1] + np.float32(100.0 / invT)      # a gap above 86 / invT: e saturates at exp(-86)
    return rows


@pytest.mark.parametrize("invT", [1.0, 10.0])
@pytest.mark.parametrize("C", [2, 19, 32])
def test_host_entry_matches_the_float64_definitions(C, invT):
    """Bound 2e-6 absolute: every value is at most 1 and carries a handful of 2^-24 roundings plus the 1-ulp exp / log (about 3e-7
    for entropy at C = 32), the fixed-point floor adds 2^-40.  Observed maxima over these cases: 1.8e-7 at invT = 1 (entropy, C = 32); at invT = 10
    bvsb 1.37e-6, margin 1.42e-6, least_confidence 1.42e-6, entropy 1.7e-7 -- there the rounding of z * invT (|t| up to ~50, so 3e-6
    absolute on t), which mas_bvsb has always carried, dominates: the margin under the bound is 1.4x there, not the 5x of the plain
    rounding count, and other seeds or larger |z * invT| may cross it -- that would be this arithmetic's known error, not a new one."""
    rs = np.random.RandomState(100 * C + int(invT))
    z = np.concatenate([rs.randn(400, C).astype(np.float32), (rs.randn(200, C) * 0.2).astype(np.float32), edge_rows(C, invT)])
    ref, arg = measures_f64(z, invT)
    worst = {}
    for m in MEASURES:
        u, a, _ = per_pixel(z, np.float32(invT), m)
        worst[m] = float(np.abs(u - ref[m]).max())
        assert np.array_equal(a, arg), m
        assert u.min() > 0.0 and u.max() <= 1.0000001, m
    print("max |host - f64| at C=%d invT=%g: %s" % (C, invT, worst))
    assert max(worst.values()) <= 2e-6, worst
    n = z.shape[0]
    tie, flat, gap = n - 3, n - 2, n - 1
    assert arg[tie] == (0 if C == 2 else 1)
    assert per_pixel(z, np.float32(invT), 'bvsb')[0][tie] == pytest.approx(1.0 + 1e-8, abs=1e-7)
    assert per_pixel(z, np.float32(invT), 'entropy')[0][flat] == pytest.approx(1.0 + 1e-8, abs=1e-7)
    for m in MEASURES:
        assert ref[m][gap] < 1e-6 and per_pixel(z, np.float32(invT), m)[0][gap] == pytest.approx(1e-8, abs=2e-6)


def test_bvsb_measure_and_class_prior_equal_the_c_oracle_of_the_headline_scan():
    """measure = bvsb is the yardstick: all three accumulators equal oracle/exact.c's restatement of mas_single_pass_accum."""
    from oracle import exact
    rs = np.random.RandomState(4)
    B, C, H, W, S = 2, 20, 11, 17, 5
    z = (rs.randn(B, C, H, W) * 0.4).astype(np.float32)
    spx = rs.randint(-1, S + 1, (B, H, W)).astype(np.int64)
    invT = ops().inv_temperature(0.1)
    ps, cs, hh = ops().uncertainty_reference(torch.from_numpy(z), torch.from_numpy(spx), S, invT, 'bvsb')
    eps, ecs, eh = exact.single_pass_accum(z, spx, S, np.float32(invT))
    assert np.array_equal(ps.numpy().view(np.uint64), eps)
    assert np.array_equal(cs.numpy().view(np.uint64), ecs)
    assert np.array_equal(hh.numpy().view(np.uint32), eh)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.int16])
def test_accumulator_semantics(dtype):
    rs = np.random.RandomState(7)
    B, C, H, W, S = 2, 7, 9, 14, 6
    z = torch.from_numpy(rs.randn(B, C, H, W).astype(np.float32))
    ids = rs.randint(0, S - 1, (B, H, W))                # id S - 1 is never used
    if dtype != torch.int16:                              # (the 16-bit ids are unsigned: no -1)
        ids[:, 0, :] = -1
    ids[:, 1, :] = S
    spx = torch.from_numpy(ids).to(dtype)
    out = {m: ops().uncertainty_reference(z, spx, S, 1.0, m) for m in MEASURES}
    ps, cs, hh = out['bvsb']
    counted = int(((ids >= 0) & (ids < S)).sum())
    assert int(hh.sum()) == counted                                                   # ids -1 and S are skipped
    assert int(hh[:, S - 1].sum()) == 0 and int(cs[:, S - 1].abs().sum()) == 0        # an empty region stays 0
    assert bool(((cs != 0) == (hh != 0)).all())                                       # a present (region, class) never sums to 0
    assert abs(int(ps.sum()) - B * H * W * 2 ** 23) <= B * H * W * C                  # every pixel enters the class prior
    for m in NEW_MEASURES:
        assert torch.equal(out[m][0], ps) and torch.equal(out[m][2], hh), m           # prior and histogram ignore the measure
        assert not torch.equal(out[m][1], cs), m
    for m in MEASURES:                                                                # += : a second call doubles everything
        p2, c2, h2 = (t.clone() for t in out[m])
        ops().uncertainty_reference(z, spx, S, 1.0, m, prob_sum=p2, class_sum=c2, hist=h2)
        assert torch.equal(p2, 2 * out[m][0]) and torch.equal(c2, 2 * out[m][1]) and torch.equal(h2, 2 * out[m][2]), m


def test_arguments_are_refused():
    from mulactseg_amd import _lib
    z = torch.zeros((1, 3, 2, 2))
    spx = torch.zeros((1, 2, 2), dtype=torch.int64)
    with pytest.raises(ValueError):
        ops().uncertainty_reference(z, spx, 2, 1.0, 'variance')
    with pytest.raises(_lib.MulActSegHipError, match="class count"):
        ops().uncertainty_reference(torch.zeros((1, 33, 2, 2)), spx, 2, 1.0, 'entropy')
    lib = _lib.load()
    assert lib.mas_uncertainty_reference(z.data_ptr(), spx.data_ptr(), 0, 1, 3, 2, 2, 2, 1.0, 4, z.data_ptr(), z.data_ptr(), z.data_ptr()) == -6
    assert lib.mas_uncertainty_accum(None, None, 0, 1, 3, 2, 2, 2, 1.0, 1, None, None, None, None) == -1
    assert ops().UNCERTAINTY == {'bvsb': 0, 'margin': 1, 'least_confidence': 2, 'entropy': 3}


# ------------------------------------------------------------------------------------------------
# the selectors on the new pass
# ------------------------------------------------------------------------------------------------
class UncertaintyOracleBackend(OracleBackend):
    """The CPU stand-in with ``uncertainty_pass`` backed by the library's host entry; records which scans ran."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def region_accum(self, *a):
        self.calls.append('region_accum')
        return super().region_accum(*a)

    def class_prob_sum(self, *a):
        self.calls.append('class_prob_sum')
        return super().class_prob_sum(*a)

    def single_pass(self, *a):
        self.calls.append('single_pass')
        return super().single_pass(*a)

    def uncertainty_pass(self, logits, spx, S, invT, measure, prob_sum, class_sum, hist):
        self.calls.append('uncertainty_pass:' + measure)
        ps, cs, hh = ops().uncertainty_reference(logits.contiguous(), spx.contiguous(), S, invT, measure)
        prob_sum += ps
        class_sum += cs
        hist += hh


N_IMG, BATCH, S, C, H, W = 5, 2, 6, 20, 33, 47


def tiny_pool():
    """5 pictures of 33 x 47 with 6 block regions and 20 channels, scored at T = 0.1.  Every region has a main class (some the last
    channel, for the ban) under pixel noise and is fairly confident -- except two regions of picture 0 the measures order
    differently: region 0 is split 0.5 / 0.5 between two classes (p2 / p1 = 1, entropy ln 2 / ln C), region 1 is near-uniform over
    ten classes (p2 / p1 ~ 0.8, entropy ~ ln 10 / ln C)."""
    rs = np.random.RandomState(11)
    yy, xx = np.mgrid[0:H, 0:W]
    block = ((yy // 12) * 2 + xx // 24).astype(np.int64)               # ids 0..5
    z = (rs.randn(N_IMG, C, H, W) * 0.05).astype(np.float32)
    spx = np.stack([block] * N_IMG)
    for i in range(N_IMG):
        main = (3 * i + 5 * block) % C
        cls = np.where(rs.rand(H, W) < 0.2, rs.randint(0, C, (H, W)), main)
        z[i][cls, yy, xx] += np.float32(0.6)
    a, b = block == 0, block == 1
    z[0][:, a] = -1.0
    z[0][2][a] = z[0][3][a] = 0.5
    z[0][:, b] = -1.0
    z[0][5:15][:, b] = 0.5
    z[0][5][b] += np.float32(0.02)
    spx[1][0, :5] = -1                                                  # a few pixels outside every region
    im_idx = [["i/%03d.png" % i, "l/%03d.png" % i, "s/spx_%04d.pkl" % i] for i in range(N_IMG)]
    suppix = {k[2]: list(range(S)) for k in im_idx}
    return z, spx, im_idx, suppix


class RecordingActiveSet:
    """What ``select_next_batch`` needs of an active set: the pool, and a sink for the consumed prefix."""

    def __init__(self, pool):
        self.trg_pool_dataset = pool
        self.prefix = None

    def expand_training_set(self, sample_region, selection_count, selection_method):
        self.prefix = sample_region.tuples()


def make_selector(modname, ncls, method, measure, backend=None, **kw):
    opts = dict(val_batch_size=BATCH, nseg=S, num_classes=ncls, method=method, fair_counting=False, or_labeling=False)
    opts.update(kw)
    args = selector_args(**opts)
    if measure is not None:
        args.uncertainty = measure
    sel = importlib.import_module("mulactseg_amd.active_selection." + modname).RegionSelector(args)
    if backend is not None:
        sel.backend = backend
    return sel


def run_round(sel, trainer, pool_arrays, budget=7):
    """(scores [n_img, S] numpy, consumed prefix) of one round through ``select_next_batch`` (one scan: the scores are captured)."""
    box = {}
    scan = sel.calculate_scores_tensor

    def capture(tr, pool_set):
        box['scores'] = scan(tr, pool_set)
        return box['scores']
    sel.calculate_scores_tensor = capture
    active = RecordingActiveSet(FakePool(*pool_arrays))
    sel.select_next_batch(trainer, active, budget)
    return box['scores'].cpu().numpy().copy(), active.prefix


_CPU_ROUNDS = {}


def cpu_round(modname, ncls, method, measure):
    """The CPU stand-in's round, computed once per (selector, measure) and shared (tests/test_uncertainty_gpu.py reads it too)."""
    key = (modname, measure)
    if key not in _CPU_ROUNDS:
        sel = make_selector(modname, ncls, method, measure, UncertaintyOracleBackend())
        _CPU_ROUNDS[key] = run_round(sel, fake_trainer(), tiny_pool()) + (sel.backend.calls,)
    return _CPU_ROUNDS[key]


def region_means_f64(z, spx, invT, measure):
    n_img, Cz = z.shape[:2]
    out = np.zeros((n_img, S))
    for i in range(n_img):
        u = measures_f64(z[i].reshape(Cz, -1).T, invT)[0][measure]
        ids = spx[i].ravel()
        for s in range(S):
            out[i, s] = u[ids == s].mean()
    return out


@pytest.mark.parametrize("measure", NEW_MEASURES)
@pytest.mark.parametrize("modname,ncls,method", SELECTORS)
def test_selectors_run_on_the_new_pass_and_select_in_score_order(modname, ncls, method, measure):
    scores, prefix, calls = cpu_round(modname, ncls, method, measure)
    assert set(calls) == {'uncertainty_pass:' + measure} and len(calls) == (N_IMG + BATCH - 1) // BATCH
    assert scores.shape == (N_IMG, S) and np.isfinite(scores).all()
    # the consumed prefix is the head of the reference's descending (score, path, id) tuple order
    z, spx, im_idx, suppix = tiny_pool()
    tuples = sorted(((float(scores[i, s]), ','.join(im_idx[i]), s) for i in range(N_IMG) for s in range(S)), reverse=True)
    assert len(prefix) in (7, 8) and prefix == tuples[:len(prefix)]
    if 'banignore' in modname:       # regions whose main class is the "undefined" channel score 0
        assert (scores == 0).any()
    if modname == 'my_bvsb':
        # min-max normalised float64 region means: 2e-6 per value (above), twice for the subtracted minimum, over a range >= 0.4
        ref = region_means_f64(z[:, :-1], spx, np.float32(10.0), measure)
        ref = (ref - ref.min()) / (ref.max() - ref.min())
        assert np.abs(scores - ref).max() <= 1e-5


def test_bvsb_and_entropy_pick_opposite_regions():
    """Budget 0 consumes exactly the top region: the 0.5 / 0.5 region under BvSB (the selector's own kernels), the ten-way region
    under entropy."""
    picks = {}
    for measure in (None, 'bvsb', 'entropy', 'margin', 'least_confidence'):
        sel = make_selector('my_bvsb', 20, PLAIN, measure, UncertaintyOracleBackend())      # (all 20 channels: no region is left flat)
        scores, prefix = run_round(sel, fake_trainer(), tiny_pool(), budget=0)
        picks[measure] = prefix[0][1:]
        assert (scores[0, 0] > scores[0, 1]) == (measure in (None, 'bvsb', 'margin'))
    two_way, ten_way = ("i/000.png,l/000.png,s/spx_0000.pkl", 0), ("i/000.png,l/000.png,s/spx_0000.pkl", 1)
    assert picks[None] == picks['bvsb'] == two_way
    assert picks['entropy'] == ten_way
    assert picks['least_confidence'] == ten_way and picks['margin'] == two_way


@pytest.mark.parametrize("modname,ncls,method", SELECTORS)
def test_default_measure_leaves_the_selectors_on_their_old_calls(modname, ncls, method):
    want = {'my_bvsb': {'region_accum'}, 'my_bvsb_banignore': {'region_accum'}, 'my_bvsb_clsbal_v2': {'region_accum'},
            'my_bvsb_clsbal_v2_banignore': {'region_accum'}, 'my_bvsb_predclsbal_pwr': {'single_pass'},
            'my_bvsb_predclsbal_pwr_banignore': {'single_pass'}}[modname]
    got = []
    for measure in (None, 'bvsb'):              # no flag at all (an args object from before it existed), and the default value
        sel = make_selector(modname, ncls, method, measure, UncertaintyOracleBackend())
        scores, prefix = run_round(sel, fake_trainer(), tiny_pool())
        assert set(sel.backend.calls) == want
        got.append((scores, prefix))
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]


def test_two_pass_scoring_refuses_another_measure():
    sel = make_selector('my_bvsb_predclsbal_pwr', 20, PLAIN, 'entropy', UncertaintyOracleBackend(), two_pass_scoring=True)
    with pytest.raises(ValueError, match="single-pass"):
        sel.calculate_scores_tensor(fake_trainer(), FakePool(*tiny_pool()))
    sel = make_selector('my_bvsb_predclsbal_pwr', 20, PLAIN, 'bvsb', UncertaintyOracleBackend(), two_pass_scoring=True)
    sel.calculate_scores_tensor(fake_trainer(), FakePool(*tiny_pool()))
    assert set(sel.backend.calls) == {'class_prob_sum', 'region_accum'}


def test_random_and_dummy_selectors_ignore_the_flag():
    from mulactseg_amd.active_selection import dummy, my_random
    for mod in (dummy, my_random):
        mod.RegionSelector(selector_args(uncertainty='entropy'))


# ------------------------------------------------------------------------------------------------
# flags
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modname", ['common', 'common_voc'])
def test_uncertainty_flag_parses(modname):
    mod = importlib.import_module("mulactseg_amd.utils." + modname)
    p = mod.get_parser()
    assert p.parse_args([]).uncertainty == 'bvsb'
    for m in MEASURES:
        assert p.parse_args(['--uncertainty', m]).uncertainty == m
    with pytest.raises(SystemExit):
        p.parse_args(['--uncertainty', 'variance'])


def test_arg_assert_refuses_another_measure_with_two_pass_scoring():
    from mulactseg_amd.utils import common
    args = common.get_parser().parse_args(['--uncertainty', 'entropy', '--nseg', '2048'])
    args.trg_datalist, args.region_dict = 'lists/train_2048.txt', 'lists/train_2048.dict'
    common.arg_assert(args)                                  # the single-pass round (the default) takes every measure
    args.two_pass_scoring = True
    with pytest.raises(ValueError, match="two_pass_scoring"):
        common.arg_assert(args)
    args.uncertainty = 'bvsb'
    common.arg_assert(args)
