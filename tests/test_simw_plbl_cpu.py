"""The similarity-weighted online pseudo labels without a GPU: the library's host loops (``ops.online_plbl_reference`` with
``weight_sim`` / ``signed``, ``ops.simw_plbl_reference``; csrc/online_plbl.h) against the executed reference
(tests/golden/g16_simw_plbl.npz) and the float64 restatement (tests/simw_plbl_restated.py), ``simw_temp_at``, the two arguments and the
refusals, the registry entries, and the ABI."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import online_plbl_restated as R
import simw_plbl_restated as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ('active_onlinesimwplbl_multi_predignore', 'active_pwce_multi_predignore')
NAMES = ('zq_p', 'featq', 'zq', 'tgt', 'spx', 'msk')


def golden():
    return np.load(os.path.join(GOLDEN, "g16_simw_plbl.npz"))


def golden_inputs():
    g = golden()
    assert (int(g['seed']), int(g['N']), int(g['C']), int(g['Ch']), int(g['H']), int(g['W']), int(g['hq']), int(g['wq']), int(g['S'])) == \
        (R.SEED, R.N, R.C, R.CH, R.H, R.W, R.HQ, R.WQ, R.S) and float(g['temp']) == R.T
    return dict(zip(NAMES, [torch.from_numpy(np.ascontiguousarray(a)) for a in R.inputs()]))


def tensors(case):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])) for k in NAMES}


def golden_softw(g, k):
    """the reference's soft weights of tau k as the library lays them out: f32 [N,C,H,W], NaN off the candidates of the valid pixels"""
    valid = g['labels'] != 255
    tgt = R.inputs()[3]
    spx = R.inputs()[4]
    full = np.full((R.N, R.H, R.W, R.C), np.nan, dtype=np.float32)
    full[valid] = np.where(tgt[np.nonzero(valid)[0], spx[valid]] != 0, g['softw'][k], np.nan)
    return np.ascontiguousarray(np.moveaxis(full, -1, 1))


def _ops():
    from mulactseg_amd import ops
    return ops


def _host_labels(t, size, **kw):
    ops = _ops()
    return ops.online_plbl_reference(t['zq_p'], t['featq'], size, t['spx'], t['msk'], targets=t['tgt'], invT=ops.inv_temperature(R.T), **kw)


def _host_soft(t, size, tau, **kw):
    ops = _ops()
    invT = ops.inv_temperature(R.T)
    return ops.simw_plbl_reference(size, t['spx'], t['msk'], targets=t['tgt'], zq_p=t['zq_p'], featq=t['featq'], invT=invT,
                                   inv_tau=ops.inv_temperature(tau), invT_ce=invT, **kw)


def test_labels_equal_the_parents_and_similarity_weights_match_the_executed_reference():
    g, t = golden(), golden_inputs()
    size = (R.H, R.W)
    parent, out = _host_labels(t, size), _host_labels(t, size, weight_sim=True)
    assert torch.equal(parent['labels'], out['labels']) and torch.equal(parent['gmax'], out['gmax'])
    lab, wgt = out['labels'].numpy(), out['weight'].numpy()
    valid = g['labels'] != 255
    bound = 8 * float(g['sim_err_ref'])
    decided = g['gap64'] > bound
    assert valid.sum() > 500 and 200 * int((~decided).sum()) <= int(valid.sum())
    assert np.array_equal(lab != 255, valid) and np.array_equal(lab[valid][decided], g['labels'][valid][decided])
    agree = lab[valid] == g['labels'][valid]
    err = float(np.abs(wgt[valid] - g['simw'])[agree].max())
    print("similarity weights: max error %.3e, bound %.3e, negative %d of %d" % (err, bound, (g['simw'] < 0).sum(), valid.sum()))
    assert err <= bound
    assert np.all(wgt[~valid] == 0) and int((wgt < 0).sum()) >= 1 and np.array_equal(wgt[valid] < 0, g['simw'] < 0)
    assert not np.array_equal(wgt, parent['weight'].numpy())


@pytest.mark.parametrize("k", [0, 1])
def test_soft_weights_match_the_executed_reference(k):
    g, t = golden(), golden_inputs()
    tau, size = float(g['taus'][k]), (R.H, R.W)
    out = _host_soft(t, size, tau)
    got, ref = out['softw'].numpy(), golden_softw(g, k)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and out['live'].tolist() == [1, 1]
    d = Q.similarities(R.upsample(t['zq_p'], size), R.upsample(t['featq'], size), t['tgt'], t['spx'], t['msk'], R.T, near=1e-5)
    valid = g['labels'] != 255
    left_out = int((d['loose'] & valid).sum())
    assert 200 * left_out <= int(valid.sum())                                    # at most 0.5 % (the recorder proves the reference meets it)
    keep = ~np.isnan(ref) & ~d['loose'][:, None]
    err, bound = float(np.abs(got - ref)[keep].max()), 8 * float(g['softw_err_ref'][k])
    print("tau %g: soft weights max error %.3e, bound %.3e, left out %d of %d" % (tau, err, bound, left_out, valid.sum()))
    assert err <= bound
    sums = np.nansum(got, axis=1)[valid]
    assert np.abs(sums - 1).max() <= 1e-6


def _pushed_error(zq, dzq_fix, want):
    got = dzq_fix.double() * 2.0 ** -44
    want = torch.from_numpy(np.asarray(want)).double()
    return float((got - want).abs().max()), float(want.abs().max())


@pytest.mark.parametrize("k", [0, 1])
def test_soft_ce_on_the_golden_weights_matches_the_executed_reference(k):
    """the value on the reference's own soft weights, the gradient against the reference's pushed through the transpose of the bilinear
    upsampling"""
    ops, g, t = _ops(), golden(), golden_inputs()
    softw = torch.from_numpy(golden_softw(g, k))
    out = ops.simw_plbl_reference((R.H, R.W), t['spx'], t['msk'], targets=t['tgt'], softw=softw, live=torch.ones(R.N, dtype=torch.int32),
                                  zq=t['zq'], invT_ce=ops.inv_temperature(R.T), grad=torch.ones(1))
    ref = float(g['pwce_loss'][k])
    print("pwce tau %g: %.7f against %.7f, counted %d" % (float(g['taus'][k]), float(out['loss']), ref, int(out['acc'][1])))
    assert int(out['acc'][1]) == int(g['pwce_count']) and abs(float(out['loss']) - ref) <= 2e-6 * abs(ref)
    err, scale = _pushed_error(t['zq'], out['dzq_fix'], g['pwce_gradq'][k])
    print("gradient: max error %.3e of max|ref| %.3e" % (err, scale))
    assert scale > 0 and err <= 1e-4 * scale


@pytest.mark.parametrize("name,mode,signed", [('simw', 1, True), ('simw_th', 2, False)])
def test_signed_ce_on_the_golden_maps_matches_the_executed_reference(name, mode, signed):
    """a signed sum may cancel, so the mass (the mean |weight * CE|) is the scale of the bound"""
    ops, g, t = _ops(), golden(), golden_inputs()
    valid = g['labels'] != 255
    weight = np.zeros(valid.shape, dtype=np.float32)
    weight[valid] = g['simw']
    out = ops.online_plbl_reference(None, None, (R.H, R.W), None, None, zq=t['zq'], invT_ce=ops.inv_temperature(R.T), mode=mode,
                                    th=float(g['th']), signed=signed, grad=torch.ones(1), labels=torch.from_numpy(g['labels']),
                                    weight=torch.from_numpy(weight))
    ref, mass = float(g[name + '_loss']), float(g[name + '_abs'])
    print("%s: %.7f against %.7f (mass %.7f), counted %d" % (name, float(out['loss']), ref, mass, int(out['acc'][1])))
    assert abs(float(out['loss']) - ref) <= 2e-6 * mass
    assert int(out['acc'][1]) == (int(valid.sum()) if signed else int(g['simw_th_count']))
    err, scale = _pushed_error(t['zq'], out['dzq_fix'], g[name + '_gradq'])
    print("gradient: max error %.3e of max|ref| %.3e" % (err, scale))
    assert scale > 0 and err <= 1e-4 * scale


def test_unsigned_modes_compute_what_they_computed():
    """without the flag a negative term still adds 0 and is still counted: the value on the similarity weights is the positive part"""
    ops, t = _ops(), golden_inputs()
    size, invT = (R.H, R.W), _ops().inv_temperature(R.T)
    sim = _host_labels(t, size, weight_sim=True)
    kw = dict(zq=t['zq'], invT_ce=invT, mode=1, grad=torch.ones(1), labels=sim['labels'], weight=sim['weight'])
    s = ops.online_plbl_reference(None, None, size, None, None, signed=True, **kw)
    u = ops.online_plbl_reference(None, None, size, None, None, **kw)
    pos = ops.online_plbl_reference(None, None, size, None, None, **dict(kw, weight=sim['weight'].clamp(min=0)))
    assert int(u['acc'][1]) == int(s['acc'][1]) and int(u['acc'][0]) == int(pos['acc'][0]) and int(s['acc'][0]) < int(u['acc'][0])
    assert torch.equal(s['dzq_fix'], u['dzq_fix'])                              # k = scale * wgt carries the sign in both


def test_edge_case_against_the_restatement():
    """37 x 45 from 10 x 12: picture 1 (nothing selected) and picture 2 (642 selected one-hot pixels, no multi-hot one) add nothing to
    the sum or the count of the soft CE; the signed loss has its negative terms"""
    ops = _ops()
    e = R.edge_case()
    t, size = tensors(e), e['size']
    up = {k: R.upsample_f32(e[k], size) for k in ('zq_p', 'featq', 'zq')}
    d = Q.similarities(up['zq_p'], up['featq'], e['tgt'], e['spx'], e['msk'], R.T, near=1e-5)
    assert d['live'].tolist() == [True, False, False, True] and int(e['msk'][2].sum()) == 642
    tau = 0.1
    out = _host_soft(t, size, tau, zq=t['zq'], grad=torch.ones(1))
    assert out['live'].tolist() == [1, 0, 0, 1] and int(out['acc'][1]) == 2293 == int(e['msk'][0].sum()) + int(e['msk'][3].sum())
    assert not out['dzq_fix'][1].any() and not out['dzq_fix'][2].any() and out['dzq_fix'][0].any()
    # the restatement on the library's own soft weights (a prototype pick that depends on rounding moves a weight, not this check)
    val, grad, cnt = Q.soft_loss(up['zq'], e['tgt'], e['spx'], e['msk'], out['softw'].numpy(), out['live'].numpy(), R.T)
    print("soft CE: %.7f against %.7f, counted %d" % (float(out['loss']), val, cnt))
    assert cnt == 2293 and abs(float(out['loss']) - val) <= 2e-6
    got = out['softw'].numpy()
    sw64 = Q.soft_weights(d['sims'], tau)
    assert np.array_equal(np.isnan(got), np.isnan(sw64))
    keep = ~np.isnan(sw64) & ~d['loose'][:, None]
    assert keep.sum() >= 0.9 * (~np.isnan(sw64)).sum() and np.abs(got - sw64)[keep].max() <= 1e-5
    # picture 2 alone: no live picture, an empty loss
    one = {k: v[2:3].contiguous() for k, v in t.items()}
    alone = _host_soft(one, size, tau, zq=one['zq'], grad=torch.ones(1))
    assert alone['live'].tolist() == [0] and alone['acc'].tolist() == [0, 0] and float(alone['loss']) == 0.0 and not alone['dzq_fix'].any()
    # the similarity-weighted hard labels
    sim = _host_labels(t, size, weight_sim=True)
    wgt = sim['weight'].numpy()
    assert int((wgt < 0).sum()) >= 1
    kw = dict(zq=t['zq'], invT_ce=ops.inv_temperature(R.T), mode=1, labels=sim['labels'], weight=sim['weight'])
    s = ops.online_plbl_reference(None, None, size, None, None, signed=True, **kw)
    u = ops.online_plbl_reference(None, None, size, None, None, **kw)
    val, _, cnt, mass = Q.signed_loss(up['zq'], sim['labels'].numpy(), wgt, R.T)
    print("signed: %.7f, unsigned %.7f, restated %.7f, negative weights %d of %d" % (float(s['loss']), float(u['loss']), val,
                                                                                     (wgt < 0).sum(), (sim['labels'] != 255).sum()))
    assert float(s['loss']) != float(u['loss']) and int(s['acc'][1]) == cnt and abs(float(s['loss']) - val) <= 2e-6 * mass


def negated_tensors():
    """tests/simw_plbl_restated.py: negated_case on the library's own prototype pixels"""
    base = Q.negated_case()
    gmax = _host_labels(tensors(base), base['size'])['gmax'].numpy()
    case = Q.negated_case(gmax=gmax)
    return case, tensors(case)


def test_negated_features_give_negative_weights_a_negative_loss_and_the_opposite_gradient():
    """Every non-prototype valid pixel carries the negation of its superpixel's prototype feature: its weight is -1 (a prototype pixel's own
    weight is its squared norm, +1, and cannot be negative).  The loss is below 0.  Against the run with the features not negated (every
    weight +1) the gradient is the opposite at every non-prototype pixel and the same at the prototypes: the quarter map has the picture's
    size, so every pixel's gradient lands on its own element."""
    ops = _ops()
    case, t = negated_tensors()
    size, invT = case['size'], ops.inv_temperature(R.T)
    proto = case['proto']
    neg = _host_labels(t, size, weight_sim=True)
    pos = _host_labels(dict(t, featq=torch.where(torch.from_numpy(proto)[:, None], t['featq'], -t['featq']).contiguous()), size,
                       weight_sim=True)
    assert torch.equal(neg['gmax'], pos['gmax']) and torch.equal(neg['labels'], pos['labels'])
    lab, wn, wp = neg['labels'].numpy(), neg['weight'].numpy(), pos['weight'].numpy()
    valid = lab != 255
    assert valid.sum() > 200 and proto.sum() > 4 and np.all(valid[proto])
    assert np.all(wn[valid & ~proto] < 0) and np.abs(wn[valid & ~proto] + 1).max() <= 1e-5
    assert np.abs(wn[proto] - 1).max() <= 1e-5 and np.abs(wp[valid] - 1).max() <= 1e-5
    kw = dict(zq=t['zq'], invT_ce=invT, mode=1, grad=torch.ones(1))
    sn = ops.online_plbl_reference(None, None, size, None, None, signed=True, labels=neg['labels'], weight=neg['weight'], **kw)
    un = ops.online_plbl_reference(None, None, size, None, None, labels=neg['labels'], weight=neg['weight'], **kw)
    sp = ops.online_plbl_reference(None, None, size, None, None, signed=True, labels=pos['labels'], weight=pos['weight'], **kw)
    print("negated: signed %.6f, unsigned %.6f; not negated %.6f" % (float(sn['loss']), float(un['loss']), float(sp['loss'])))
    assert float(sn['loss']) < 0 < float(sp['loss']) and float(un['loss']) >= 0 and sn['acc'][1] == sp['acc'][1] == int(valid.sum())
    gn, gp = sn['dzq_fix'].double().numpy(), sp['dzq_fix'].double().numpy()
    off = np.broadcast_to((valid & ~proto)[:, None], gn.shape)
    on = np.broadcast_to(proto[:, None], gn.shape)
    assert np.abs(gp[off]).max() > 0 and np.abs(gn[off] + gp[off]).max() <= 2e-5 * np.abs(gp[off]).max()
    assert np.abs(gn[on] - gp[on]).max() <= 2e-5 * np.abs(gp[on]).max() and not gn[np.broadcast_to(~valid[:, None], gn.shape)].any()


def test_simw_temp_schedule():
    mod = importlib.import_module("mulactseg_amd.trainer.active_pwce_multi_predignore")
    tr = mod.ActiveTrainer.__new__(mod.ActiveTrainer)
    tr.args = types.SimpleNamespace(simw_temp=0.05, simw_temp_schedule=True)
    tr.simw_temp_orig = 0.05
    assert (tr.simw_temp_at(0), tr.simw_temp_at(19999), tr.simw_temp_at(20000)) == (1000.0, 1000.0, 0.05)
    assert tr.args.simw_temp == 0.05                                            # the schedule does not write into args
    tr.args.simw_temp_schedule = False
    assert (tr.simw_temp_at(0), tr.simw_temp_at(19999), tr.simw_temp_at(20000)) == (0.05, 0.05, 0.05)


def _checked(extra, method):
    from mulactseg_amd.utils import common
    args = common.get_parser().parse_args(extra + ['--nseg', '2048', '--method', method])
    args.trg_datalist, args.region_dict = 'train_seed2048.txt', 'train_seed2048.dict'
    common.arg_assert(args)


def test_arguments_defaults_and_refusals():
    from mulactseg_amd.utils import common
    for module in ("common", "common_voc"):
        p = importlib.import_module("mulactseg_amd.utils." + module).get_parser()
        a = p.parse_args([])
        assert (a.simw_temp, a.simw_temp_schedule) == (0.1, False)
        a = p.parse_args(['--simw_temp', '0.02', '--simw_temp_schedule'])
        assert (a.simw_temp, a.simw_temp_schedule) == (0.02, True)
    online = (['--lamparam', '0.2'], ['--lamscale', '2'], ['--dorampup'], ['--th_wplbl', '0.7'])
    simw = (['--simw_temp', '0.02'], ['--simw_temp_schedule'])
    for extra in online:
        _checked(extra, METHODS[0])
    for extra in (['--weight_wo_proto'],) + simw:
        with pytest.raises(NotImplementedError, match=extra[0][2:]):
            _checked(extra, METHODS[0])
    for extra in simw:
        _checked(extra, METHODS[1])
    for extra in online + (['--weight_wo_proto'],):
        with pytest.raises(NotImplementedError, match=extra[0][2:]):
            _checked(extra, METHODS[1])
    for method in ('active_joint_multi_predignore', 'active') + common.ONLINE_PLBL_METHODS:
        for extra in simw:
            with pytest.raises(NotImplementedError, match=extra[0][2:]):
                _checked(extra, method)
        _checked([], method)
    assert common.SIMW_PLBL_METHODS == METHODS
    assert common.ONLINE_PLBL_METHODS == ('active_onlineplbl_multi_predignore', 'active_onlinewplbl_multi_predignore',
                                          'active_onlinewplblonly_multi_predignore')


def test_registry_entries_and_loss_classes():
    import mulactseg_amd
    from mulactseg_amd import _lib
    from mulactseg_amd.utils import loss as L
    from mulactseg_amd.trainer import active_joint_multi_predignore as base, active_onlineplbl_multi_predignore as online
    simw = importlib.import_module("mulactseg_amd.trainer." + METHODS[0]).ActiveTrainer
    pwce = importlib.import_module("mulactseg_amd.trainer." + METHODS[1]).ActiveTrainer
    assert issubclass(simw, online.ActiveTrainer) and simw.proto_loss_class is L.LocalsimWProtoCE and simw.uses_pos_loss
    assert simw.proto_meter == 'local-proto-loss' and simw.train_impl is online.ActiveTrainer.train_impl
    assert issubclass(pwce, base.ActiveTrainer) and not issubclass(pwce, online.ActiveTrainer) and pwce.predicts_ignore
    assert pwce.pseudo_label_forward is online.ActiveTrainer.pseudo_label_forward and pwce.update is base.ActiveTrainer.update
    assert issubclass(L.LocalsimWProtoCE, L.LocalProtoCE) and L.LocalsimWProtoCE._weight_sim and not L.LocalProtoCE._weight_sim
    assert not L.LocalWProtoCE._weight_sim and not L.LocalsimWProtoCE._honours_weight_wo_proto and not L.LocalsimWProtoCE._empty_nan
    a = types.SimpleNamespace(nseg=8, th_wplbl=None, weight_wo_proto=True, ce_temp=0.1, simw_temp=0.3)
    assert L.LocalsimWProtoCE(a, 8, 0.1)._mode_th() == (_lib.LCE_WEIGHTED, 0.0)
    a.th_wplbl = 0.25
    assert L.LocalsimWProtoCE(a, 8, 0.1)._mode_th() == (_lib.LCE_THRESHOLD, 0.25)
    crit = L.JointLocalProtoWeightingCE(a, 8, temperature=0.7)
    assert crit.ce_temp == 0.1 and crit.temp == 0.7                              # the constructed temperature is stored and ignored
    with pytest.raises(NotImplementedError):
        L.JointLocalProtoWeightingCE(a, 8, reduction='none')
    import sys
    saved = dict(sys.modules)
    try:
        mulactseg_amd.install_aliases()
        for m in METHODS:
            assert importlib.import_module("trainer." + m) is importlib.import_module("mulactseg_amd.trainer." + m)
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)


def test_abi_is_still_9_with_the_new_symbols():
    from mulactseg_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.mas_abi_version() == 9
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "mulactseg_hip.h")).read()
    assert "#define MAS_ABI_VERSION 9" in header
    for name in ("mas_online_soft_weights", "mas_soft_ce_fwd_lowres", "mas_soft_ce_bwd_lowres", "mas_simw_plbl_reference"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert "#define MAS_OPL_WEIGHT_SIM 2" in header and "#define MAS_LCE_SIGNED 8" in header
    assert (_lib.OPL_WEIGHT_SIM, _lib.LCE_SIGNED) == (2, 8)


def test_bad_arguments_are_refused_by_the_host_entries():
    ops, t = _ops(), golden_inputs()
    from mulactseg_amd._lib import MulActSegHipError
    size = (R.H, R.W)
    with pytest.raises(MulActSegHipError):          # both weight flags at once
        _host_labels(t, size, weight_sim=True, weight_wo_proto=True)
    zq = torch.zeros((1, 20, 3, 3))
    labels, weight = torch.full((1, 12, 12), 255, dtype=torch.uint8), torch.zeros((1, 12, 12))
    for mode in (0, 2, 3):                          # the signed sum belongs to the weighted mode; mode 3 does not exist
        with pytest.raises(MulActSegHipError):
            ops.online_plbl_reference(None, None, (12, 12), None, None, zq=zq, mode=mode, signed=True, labels=labels, weight=weight)
    out = ops.online_plbl_reference(None, None, (12, 12), None, None, zq=zq, mode=1, signed=True, labels=labels, weight=weight)
    assert float(out['loss']) == 0.0 and int(out['acc'][1]) == 0
    with pytest.raises(MulActSegHipError):          # a temperature of the similarity softmax that is not positive
        ops.simw_plbl_reference(size, t['spx'], t['msk'], targets=t['tgt'], zq_p=t['zq_p'], featq=t['featq'], inv_tau=0.0)
    with pytest.raises(MulActSegHipError):          # the quarter map is larger than the picture
        ops.simw_plbl_reference((R.HQ - 1, R.WQ - 1), t['spx'][:, :R.HQ - 1, :R.WQ - 1].contiguous(),
                                t['msk'][:, :R.HQ - 1, :R.WQ - 1].contiguous(), targets=t['tgt'], zq_p=t['zq_p'], featq=t['featq'])
