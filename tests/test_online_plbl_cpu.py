"""The online local-prototype pseudo labels without a GPU: the library's host loop (``ops.online_plbl_reference``, csrc/online_plbl.h)
against the executed reference (tests/golden/g15_online_plbl.npz) and the float64 restatement, ``ramp_up``, the five arguments and their
refusal, the registry entries, and the ABI."""
import importlib
import os

import numpy as np
import pytest
import torch

import online_plbl_restated as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ('active_onlineplbl_multi_predignore', 'active_onlinewplbl_multi_predignore', 'active_onlinewplblonly_multi_predignore')


def golden():
    return np.load(os.path.join(GOLDEN, "g15_online_plbl.npz"))


def golden_inputs():
    g = golden()
    assert (int(g['seed']), int(g['N']), int(g['C']), int(g['Ch']), int(g['H']), int(g['W']), int(g['hq']), int(g['wq']), int(g['S'])) == \
        (R.SEED, R.N, R.C, R.CH, R.H, R.W, R.HQ, R.WQ, R.S) and float(g['temp']) == R.T and float(g['th']) == R.TH
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in R.inputs()]


def _ops():
    from mulactseg_amd import ops
    return ops


def test_host_labels_and_weights_match_the_executed_reference():
    ops, g = _ops(), golden()
    zq_p, featq, zq, tgt, spx, msk = golden_inputs()
    invT = ops.inv_temperature(R.T)
    bound = 8 * float(g['sim_err_ref'])
    valid = g['labels'] != 255
    decided = valid & (g['gap64'] > bound)
    skipped = int(valid.sum()) - int(decided.sum())
    print("valid pixels %d, skipped as near ties %d, sim_err_ref %.3e" % (valid.sum(), skipped, float(g['sim_err_ref'])))
    assert valid.sum() > 500 and 200 * skipped <= int(valid.sum())               # at most 0.5 % (the recorder proves the reference meets it)
    for wo, key in ((False, 'weight'), (True, 'weight_wo')):
        out = ops.online_plbl_reference(zq_p, featq, (R.H, R.W), spx, msk, targets=tgt, invT=invT, weight_wo_proto=wo)
        lab, wgt = out['labels'].numpy(), out['weight'].numpy()
        assert np.array_equal(lab != 255, valid) and np.array_equal(lab[decided], g['labels'][decided])
        agree = valid & (lab == g['labels'])
        err = float(np.max(np.abs(wgt[agree] - g[key][agree])))
        print("%s: max error %.3e of max %.3e" % (key, err, float(g[key].max())))
        assert err <= 2e-6 * float(g[key].max())
        assert np.all(wgt[~valid] == 0)
    assert np.any(g['weight_wo'] != g['weight'])


@pytest.mark.parametrize("name,mode,th,wkey,nan", [('plain', 0, 0.0, 'weight', False), ('w', 1, 0.0, 'weight', False),
                                                   ('wo', 1, 0.0, 'weight_wo', False), ('th', 2, R.TH, 'weight', False),
                                                   ('joint', 1, 0.0, 'weight', True)])
def test_host_loss_on_the_golden_maps_matches_the_executed_reference(name, mode, th, wkey, nan):
    """values on the golden's own label and weight maps, gradients against the golden gradient pushed through the transpose of the
    bilinear upsampling"""
    ops, g = _ops(), golden()
    _, _, zq, _, _, _ = golden_inputs()
    labels, weight = torch.from_numpy(g['labels']), torch.from_numpy(g[wkey])
    out = ops.online_plbl_reference(None, None, (R.H, R.W), None, None, zq=zq, invT_ce=ops.inv_temperature(R.T), mode=mode, th=th,
                                    empty_nan=nan, grad=torch.ones(1), labels=labels, weight=weight)
    ref = float(g[name + '_loss'])
    print("%s: %.7f against %.7f" % (name, float(out['loss']), ref))
    assert abs(float(out['loss']) - ref) <= 2e-6 * abs(ref)
    if name == 'joint':
        return
    zt = zq.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(R.upsample(zt, (R.H, R.W)), zt, grad_outputs=torch.from_numpy(g[name + '_grad']))
    got = out['dzq_fix'].double() * 2.0 ** -44
    err, scale = float((got - want.double()).abs().max()), float(want.abs().max())
    print("%s gradient: max error %.3e of max|ref| %.3e" % (name, err, scale))
    assert scale > 0 and err <= 1e-4 * scale


def test_host_reference_matches_the_restatement_on_the_edge_case():
    ops = _ops()
    e = R.edge_case()
    t = {k: torch.from_numpy(np.ascontiguousarray(e[k])) for k in ('zq_p', 'featq', 'zq', 'tgt', 'spx', 'msk')}
    out = ops.online_plbl_reference(t['zq_p'], t['featq'], e['size'], t['spx'], t['msk'], targets=t['tgt'], invT=ops.inv_temperature(R.T))
    lab = out['labels'].numpy()
    lab64, w64, gap, loose = R.generate(R.upsample_f32(e['zq_p'], e['size']), R.upsample_f32(e['featq'], e['size']), e['tgt'], e['spx'],
                                        e['msk'], R.T, near=1e-5)
    lab64, gap = lab64.numpy(), gap.numpy()
    assert np.array_equal(lab != 255, lab64 != 255)
    # compared: the valid pixels whose label depends neither on the rounding of a similarity nor on that of a prototype pick (on the
    # bottom and right border rows the clamped taps give plateaus of logits equal up to rounding)
    decided = (lab64 != 255) & (gap > 1e-5) & ~loose.numpy()
    print("valid %d, compared %d" % ((lab64 != 255).sum(), decided.sum()))
    assert decided.sum() >= 0.9 * (lab64 != 255).sum() and np.array_equal(lab[decided], lab64[decided])
    assert np.all(lab[1] == 255) and np.all(lab[2] == 255) and np.any(lab[0] != 255)
    assert np.abs(out['weight'].numpy()[decided] - w64.numpy()[decided]).max() <= 2e-6
    # picture 3: the shared prototype resolves to the lower class, prototypes lie on the border, out-of-range ids stay unlabelled
    in_pair = e['spx'][3] == e['pair']
    assert in_pair.any() and np.all(lab[3][in_pair] == 3)
    gm = out['gmax'].numpy().view(np.uint64)[3]
    pix = (0xffffffff - (gm[gm != 0] & np.uint64(0xffffffff))).astype(np.int64)
    H, W = e['size']
    assert 0 in pix and pix.max() >= (H - 3) * W                # pixel 0: first row AND first column; and one at the far end
    assert np.all(lab[3][e['spx'][3] >= e['S']] == 255) and len(set(lab[3][e['spx'][3] == e['full']].tolist())) > 1


def test_ramp_up_values():
    import math
    from mulactseg_amd.utils.scheduler import ramp_up, sigmoid_ramp_up
    assert ramp_up(0.3, dorampup=False) == 1.0 and ramp_up(0.3, lamparam=0.1, scale=5.0, dorampup=False) == 1.0
    assert ramp_up(1.5, lamparam=0.1, scale=5.0, dorampup=True) == 1.0
    assert ramp_up(0.0) == 0.0
    for x, lam, sc in ((0.1, 0.1, 1.0), (0.5, 0.2, 3.0), (1.0, 0.1, 2.0)):
        want = (2.0 / (1.0 + math.exp(-x / lam)) - 1.0) * sc
        assert ramp_up(x, lamparam=lam, scale=sc, dorampup=True) == want == sigmoid_ramp_up(x, lam, sc)
    assert abs(ramp_up(0.1) - 0.46211715726000974) < 1e-15


def test_arguments_defaults_and_refusal():
    from mulactseg_amd.utils import common
    for module in ("common", "common_voc"):
        p = importlib.import_module("mulactseg_amd.utils." + module).get_parser()
        a = p.parse_args([])
        assert (a.lamparam, a.lamscale, a.dorampup, a.th_wplbl, a.weight_wo_proto) == (0.1, 1.0, False, None, False)
        a = p.parse_args(['--lamparam', '0.2', '--lamscale', '2', '--dorampup', '--th_wplbl', '0.7', '--weight_wo_proto'])
        assert (a.lamparam, a.lamscale, a.dorampup, a.th_wplbl, a.weight_wo_proto) == (0.2, 2.0, True, 0.7, True)
    for extra in (['--lamparam', '0.2'], ['--lamscale', '2'], ['--dorampup'], ['--th_wplbl', '0.7'], ['--weight_wo_proto']):
        args = common.get_parser().parse_args(extra + ['--nseg', '2048', '--method', 'active_joint_multi_predignore'])
        args.trg_datalist, args.region_dict = 'train_seed2048.txt', 'train_seed2048.dict'
        with pytest.raises(NotImplementedError, match=extra[0][2:]):
            common.arg_assert(args)
        for method in METHODS:
            args.method = method
            common.arg_assert(args)
    args = common.get_parser().parse_args(['--nseg', '2048', '--method', 'active'])
    args.trg_datalist, args.region_dict = 'train_seed2048.txt', 'train_seed2048.dict'
    common.arg_assert(args)
    assert common.ONLINE_PLBL_METHODS == METHODS


def test_registry_entries_and_loss_classes():
    from mulactseg_amd import _lib
    from mulactseg_amd.utils import loss as L
    from mulactseg_amd.trainer import active_joint_multi_predignore as base
    want = {METHODS[0]: (L.LocalProtoCE, True), METHODS[1]: (L.LocalWProtoCE, True), METHODS[2]: (L.JointLocalProtoCE, False)}
    for method, (cls, pos) in want.items():
        tr = importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer
        assert issubclass(tr, base.ActiveTrainer) and tr.predicts_ignore and tr.uses_pos_loss == pos
        assert tr.update is base.ActiveTrainer.update and tr.update_average_meter is base.ActiveTrainer.update_average_meter
    assert (L.LocalProtoCE._mode, L.LocalWProtoCE._mode, L.JointLocalProtoCE._mode) == (_lib.LCE_UNWEIGHTED, _lib.LCE_WEIGHTED, _lib.LCE_WEIGHTED)
    assert L.JointLocalProtoCE._empty_nan and not L.LocalWProtoCE._empty_nan and not L.LocalProtoCE._empty_nan
    import types
    a = types.SimpleNamespace(nseg=8, th_wplbl=0.25, weight_wo_proto=True)
    assert L.LocalWProtoCE(a, 8, 0.1)._mode_th() == (_lib.LCE_THRESHOLD, 0.25)
    assert L.JointLocalProtoCE(a, 8, 0.1)._mode_th() == (_lib.LCE_WEIGHTED, 0.0) and not L.JointLocalProtoCE._honours_weight_wo_proto
    with pytest.raises(NotImplementedError):
        L.LocalProtoCE(a, 8, 0.1, reduction='none')


def test_abi_is_still_9_with_the_new_symbols():
    from mulactseg_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.mas_abi_version() == 9
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "mulactseg_hip.h")).read()
    assert "#define MAS_ABI_VERSION 9" in header
    for name in ("mas_online_plbl_work_bytes", "mas_online_plbl_labels", "mas_label_ce_fwd_lowres", "mas_label_ce_value",
                 "mas_label_ce_bwd_lowres", "mas_online_plbl_reference"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert lib.mas_online_plbl_work_bytes(2, 16, 20) == (8 + 2 * 16 * 20) * 8


def test_bad_arguments_are_refused_by_the_host_entry():
    """the checks the device entry points share (check_geometry / check_ce), reached here through the host loop"""
    ops = _ops()
    zq = torch.zeros((1, 20, 3, 3))
    labels, weight = torch.full((1, 12, 12), 255, dtype=torch.uint8), torch.zeros((1, 12, 12))
    from mulactseg_amd._lib import MulActSegHipError
    with pytest.raises(MulActSegHipError):          # mode 3 does not exist
        ops.online_plbl_reference(None, None, (12, 12), None, None, zq=zq, mode=3, labels=labels, weight=weight)
    with pytest.raises(MulActSegHipError):          # the quarter map is larger than the picture
        ops.online_plbl_reference(None, None, (2, 2), None, None, zq=zq, labels=labels[:, :2, :2].contiguous(), weight=None)
    out = ops.online_plbl_reference(None, None, (12, 12), None, None, zq=zq, mode=1, empty_nan=True, labels=labels, weight=weight)
    assert np.isnan(float(out['loss'])) and int(out['acc'][1]) == 0
    out = ops.online_plbl_reference(None, None, (12, 12), None, None, zq=zq, mode=1, labels=labels, weight=weight)
    assert float(out['loss']) == 0.0
