"""The evaluation of the local-prototype labels inside the queried superpixels without a GPU: the library's host loop
(``ops.within_multihot_reference``, csrc/within_eval.h) against the executed reference (tests/golden/g21_within_multihot.npz) and the
float64 restatement, the counters, the printed tables, the registry entries, and the ABI."""
import contextlib
import importlib
import io
import os
import re

import numpy as np
import pytest
import torch

import online_plbl_restated as O
import within_eval_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g21_within_multihot.npz")
METHODS = {'cosplbl': 'eval_cosplbl_within_multihot', 'filt': 'eval_cosplbl_filt_within_multihot',
           'maxcos': 'eval_maxcosplbl_within_multihot', 'ensemble': 'eval_ensemble_plbl_within_multihot'}
MODES = (('proto', 'plbl_proto', 'gap64'), ('filt', 'plbl_filt', 'gap64_filt'))


def _ops():
    from mulactseg_amd import ops
    return ops


def golden():
    g = np.load(GOLDEN)
    assert tuple(int(g[k]) for k in ('seed', 'N', 'C', 'Ch', 'H', 'W', 'hq', 'wq', 'S')) == \
        (R.SEED, R.N, R.C, R.CH, R.H, R.W, R.HQ, R.WQ, R.S)
    return g


def tensors(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


@pytest.fixture(scope="module")
def host_runs():
    """the host statement on the golden inputs, once per mode"""
    ops = _ops()
    zq, featq, tgt, spx, msk, gt = tensors(R.inputs())
    return {mode: ops.within_multihot_reference(zq, featq, (R.H, R.W), spx, msk, gt, targets=tgt, mode=mode) for mode, _, _ in MODES}


def test_golden_inputs_are_the_recorded_ones():
    from oracle.gen_golden import digest
    assert str(golden()['input_digest']) == str(digest(*R.inputs()))


@pytest.mark.parametrize("mode,key,gapkey", MODES)
def test_host_labels_match_the_executed_reference(host_runs, mode, key, gapkey):
    g = golden()
    bound = 8 * float(g['sim_err_ref'])
    valid = g['plbl_proto'] != 255                       # (the reference labels every valid pixel before the filter)
    decided = valid & (g[gapkey] > bound)
    skipped = int(valid.sum()) - int(decided.sum())
    lab = host_runs[mode]['labels'].numpy()
    diag = host_runs[mode]['diag'].tolist()
    print("%s: valid pixels %d, skipped as near ties %d, sim_err_ref %.3e, diag %s" % (mode, valid.sum(), skipped, float(g['sim_err_ref']), diag))
    assert valid.sum() >= 500 and 200 * skipped <= int(valid.sum())          # at most 0.5 % (the generator proves the reference meets it)
    assert diag[0] == int(valid.sum())
    assert np.array_equal(host_runs['proto']['labels'].numpy() != 255, valid)
    assert np.all(lab[~valid] == 255) and np.array_equal(lab[decided], g[key][decided])
    assert not valid[2].any() and (g[key][valid] != 255).any()
    if mode == 'filt':
        assert diag[3] == int((host_runs['proto']['labels'].numpy() != 255).sum()) - int((lab != 255).sum()) > 0
    else:
        assert diag[3] == 0


def test_host_maxcos_count_matches_the_printed_one(host_runs):
    """the reference prints the count per picture; the generator has asserted that no winning similarity lies within 8 * sim_err_ref of
    the threshold it is compared with, so the count does not depend on rounding"""
    g = golden()
    zq, featq, tgt, spx, msk, gt = R.inputs()
    r = R.generate(O.upsample_f32(zq, (R.H, R.W)), O.upsample_f32(featq, (R.H, R.W)), tgt, spx, msk)
    assert float(g['maxcos_margin64']) > 8 * float(g['sim_err_ref'])
    printed = int(g['maxcos_counts'].sum())
    got = int(host_runs['proto']['diag'][2])
    print("maxcos: printed %s, host statement %d, float64 %s" % (g['maxcos_counts'].tolist(), got, r['below'].tolist()))
    assert printed > 0 and got == printed == int(r['below'].sum())
    assert int(host_runs['proto']['diag'][1]) == r['nproto'] > 0


@pytest.mark.parametrize("mode,key,gapkey", MODES)
def test_host_counters_are_mean_iou_of_its_own_map(host_runs, mode, key, gapkey):
    gt = R.inputs()[5]
    out = host_runs[mode]
    want = R.counts(out['labels'].numpy(), gt, R.C)
    assert np.array_equal(out['counts'].numpy(), want) and want[:R.C].sum() > 0 and want[R.C:2 * R.C].sum() > 0
    # a wider meter, and accumulation into given counters
    ops = _ops()
    zq, featq, tgt, spx, msk, gtt = tensors(R.inputs())
    again = ops.within_multihot_reference(zq, featq, (R.H, R.W), spx, msk, gtt, targets=tgt, mode=mode, num_classes=R.C + 3,
                                          counts=torch.from_numpy(R.counts(out['labels'].numpy(), gt, R.C + 3)), diag=out['diag'].clone())
    assert np.array_equal(again['counts'].numpy(), 2 * R.counts(out['labels'].numpy(), gt, R.C + 3))
    assert again['diag'].tolist() == [2 * v for v in out['diag'].tolist()]


def _report(name, label_map, gt, below=()):
    """what the project's trainer prints for the counters of ``label_map``"""
    from mulactseg_amd.utils.miou import WithinMultihotIoU
    cls = importlib.import_module("mulactseg_amd.trainer." + METHODS[name]).ActiveTrainer
    tr = object.__new__(cls)
    tr.selection_iter, tr.num_classes = 0, R.C - 1
    tr._below = [torch.tensor([v]) for v in np.cumsum(below)]
    meter = WithinMultihotIoU(R.C, R.IGNORE)
    meter._counts = torch.from_numpy(R.counts(label_map, gt, R.C))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        _, table = tr.report(meter, 'evaluation')
    return table, buf.getvalue()


@pytest.mark.parametrize("name", sorted(METHODS))
def test_tables_equal_the_printed_ones_on_the_golden_maps(name):
    g = golden()
    gt = R.inputs()[5]
    counts = g['maxcos_counts'].tolist() if name == 'maxcos' else ()
    with np.errstate(all='ignore'):
        table, printed = _report(name, g['plbl_filt' if name == 'filt' else 'plbl_proto'], gt, counts)
    want = str(g['stdout_' + name])
    assert table == str(g['table_' + name])
    assert re.sub(r"tensor\((\d+)\)", r"\1", want) == printed
    assert printed.count('[AL 0-round]') == (3 if name == 'cosplbl' else 1)
    if name == 'maxcos':
        assert printed.startswith("%d\n%d\n" % tuple(counts))


def test_host_reference_matches_the_restatement_on_the_edge_case():
    ops = _ops()
    e = R.edge_case()
    zq, featq, tgt, spx, msk, gt = tensors([e[k] for k in ('zq_p', 'featq', 'tgt', 'spx', 'msk', 'gt')])
    up_z, up_f = O.upsample_f32(e['zq_p'], e['size']), O.upsample_f32(e['featq'], e['size'])
    maps = {}
    for mode in ('proto', 'filt'):
        out = ops.within_multihot_reference(zq, featq, e['size'], spx, msk, gt, targets=tgt, mode=mode)
        lab = maps[mode] = out['labels'].numpy()
        r = R.generate(up_z, up_f, e['tgt'], e['spx'], e['msk'], mode)
        # compared: the valid pixels whose label depends neither on the rounding of a similarity nor on that of a prototype pick (on the
        # bottom and right border rows the clamped taps give plateaus of logits equal up to rounding)
        decided = r['valid'] & (r['gap_sim'] > 1e-5) & ~r['loose']
        print("%s: valid %d, compared %d, diag %s" % (mode, r['valid'].sum(), decided.sum(), out['diag'].tolist()))
        assert int(out['diag'][0]) == int(r['valid'].sum()) and np.all(lab[~r['valid']] == 255)
        # (not vacuous: only the superpixels that touch the bottom row or the right column can hold such a plateau, 12 of the 5 x 8
        #  cells of this picture, so at least 0.7 of the valid pixels are compared)
        assert decided.sum() >= 0.7 * r['valid'].sum() and np.array_equal(lab[decided], r['labels'][decided])
        assert np.array_equal(out['counts'].numpy(), R.counts(lab, e['gt'], e['C']))
        if mode == 'proto':
            assert np.array_equal(lab != 255, r['valid'])
    proto, filt = maps['proto'], maps['filt']
    # picture 0: the emptied row and the ids outside [0, S) stay unlabelled although their pixels are selected
    assert (e['msk'][0] & (e['spx'][0] == e['empty'])).any() and np.all(proto[0][e['spx'][0] == e['empty']] == 255)
    assert e['stray'].sum() == 3 and e['msk'][0][e['stray']].all() and np.all(proto[0][e['stray']] == 255)
    # picture 1 has nothing selected, picture 2 only one-hot rows: labelled here (not by the training kernels), each with its only class
    assert np.all(proto[1] == 255) and np.any(proto[2] != 255)
    sel2 = proto[2] != 255
    assert np.array_equal(proto[2][sel2], e['tgt'][2].argmax(axis=1)[e['spx'][2][sel2]])
    # picture 3: classes 3 and 11 share their prototype pixel in `pair`: every pixel takes the lower class, the filter gives the
    # prototype pixel the higher one
    in_pair = e['spx'][3] == e['pair']
    assert in_pair.any() and np.all(proto[3][in_pair] == 3)
    gm = out['gmax'].numpy().view(np.uint64)[3, e['pair']]
    pix = (0xffffffff - (gm[[3, 11]] & np.uint64(0xffffffff))).astype(np.int64)
    assert pix[0] == pix[1] and in_pair.reshape(-1)[pix[0]]
    assert filt[3].reshape(-1)[pix[0]] == 11 and set(np.unique(filt[3][in_pair]).tolist()) <= {3, 11, 255}
    assert np.all(proto[3][e['spx'][3] >= e['S']] == 255)


def test_aten_chain_matches_the_executed_reference_on_the_cpu():
    """``pseudo_label_generation`` (the MAS_WITHIN_EVAL=aten chain) restates the reference's lines: on the reference's own inputs it
    gives the reference's maps outside the near ties"""
    g = golden()
    zq, featq, tgt, spx, msk, gt = R.inputs()
    feats, logits = O.upsample(featq, (R.H, R.W)), O.upsample(zq, (R.H, R.W))
    bound = 8 * float(g['sim_err_ref'])
    for name, key, gapkey in (('cosplbl', 'plbl_proto', 'gap64'), ('filt', 'plbl_filt', 'gap64_filt')):
        tr = object.__new__(importlib.import_module("mulactseg_amd.trainer." + METHODS[name]).ActiveTrainer)
        lab, below = tr.pseudo_label_generation(torch.from_numpy(gt), feats, logits, torch.from_numpy(tgt), torch.from_numpy(msk),
                                                torch.from_numpy(spx), with_below=True)
        decided = g[gapkey] > bound
        if name == 'cosplbl':
            assert np.array_equal(lab.numpy() != 255, g[key] != 255)
        assert np.array_equal(lab.numpy()[decided], g[key][decided].astype(np.int64)) and np.all(lab.numpy()[g['plbl_proto'] == 255] == 255)
        assert int(below) == int(g['maxcos_counts'].sum())


def test_the_four_methods_resolve_through_the_registry():
    import mulactseg_amd
    from mulactseg_amd.trainer import eval_within_multihot
    from mulactseg_amd.utils.miou import MeanIoU, WithinMultihotIoU
    mulactseg_amd.install_aliases()
    for name, method in METHODS.items():
        mod = importlib.import_module("trainer." + method)                      # the name the reference's drivers import
        assert mod is importlib.import_module("mulactseg_amd.trainer." + method)
        cls = mod.ActiveTrainer
        assert issubclass(cls, eval_within_multihot.ActiveTrainer) and cls.meter_class is WithinMultihotIoU
        assert cls.eval is eval_within_multihot.ActiveTrainer.eval                  # rank sharding and all_reduce come from the base
        assert cls.generate_batch is not eval_within_multihot.ActiveTrainer.generate_batch
        assert cls.mode == ('filt' if name == 'filt' else 'proto') and cls.counts_below is (name == 'maxcos')
        assert len(cls.tables) == (3 if name == 'cosplbl' else 1)
    assert eval_within_multihot.ActiveTrainer.meter_class is MeanIoU and issubclass(WithinMultihotIoU, MeanIoU)


def test_arguments_are_checked():
    ops = _ops()
    zq, featq, tgt, spx, msk, gt = tensors(R.inputs())
    with pytest.raises(ValueError, match="mode"):
        ops.within_multihot_reference(zq, featq, (R.H, R.W), spx, msk, gt, targets=tgt, mode='other')
    with pytest.raises(ValueError, match="num_classes"):
        ops.within_multihot_reference(zq, featq, (R.H, R.W), spx, msk, gt, targets=tgt, num_classes=R.C - 1)
    with pytest.raises(ValueError, match="ground truth"):
        ops.within_multihot_reference(zq, featq, (R.H, R.W), spx, msk, gt[:, :-1].contiguous(), targets=tgt)
    with pytest.raises(ops._lib.MulActSegHipError):
        ops.within_multihot_eval(zq, featq, (R.H, R.W), spx, msk, gt, targets=tgt)          # host tensors: there is no CPU path


def test_header_exports_and_ctypes_table_agree():
    import ctypes
    from mulactseg_amd import _lib
    lib = _lib.load()
    names = ("mas_within_eval_work_bytes", "mas_within_eval_counts", "mas_within_eval_reference")
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(raw, name)
    assert lib.mas_within_eval_work_bytes(2, 16, 20) == (8 + 2 * 16 * 20) * 8 and lib.mas_within_eval_work_bytes(0, 16, 20) == 0
    assert len(_lib.SIGNATURES["mas_within_eval_counts"][1]) == 24 and len(_lib.SIGNATURES["mas_within_eval_reference"][1]) == 22
    with open(os.path.join(ROOT, "include", "mulactseg_hip.h")) as f:
        text = f.read()
    for name in names:
        assert re.search(r"\b%s\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "#define MAS_ABI_VERSION 9" in text and _lib.ABI_VERSION == 9 and lib.mas_abi_version() == 9
    assert "#define MAS_WE_PROTO 0" in text and "#define MAS_WE_FILT 1" in text and (_lib.WE_PROTO, _lib.WE_FILT) == (0, 1)
    with open(os.path.join(ROOT, "mulactseg_amd", "csrc", "Makefile")) as f:
        assert "within_eval.hip" in f.read()
    # the host statement refuses bad arguments as the device entry does
    assert lib.mas_within_eval_reference(None, None, 1, 1, 1, None, 0, None, None, 1, 20, 4, 4, 1, None, 0, 20, 255, None, None, None, None) == -1
