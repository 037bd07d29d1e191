"""--cosprop_threshold_method without a GPU: the restatement of the threshold kernels against the plain definition and torch, the way the
flag travels from the parsers to ops.stage2_pseudo_labels, and the two new rows of the C ABI."""
import os
import re
import types

import numpy as np
import pytest
import torch

import stage2_threshold_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("HW,n_proto,pattern", R.CASES)
def test_restatement_equals_the_definition_and_torch(HW, n_proto, pattern, method):
    nn, sim = R.case(HW, n_proto, pattern)
    got = R.thresholds(nn, sim, n_proto, method)
    assert np.array_equal(got, R.thresholds_plain(nn, sim, n_proto, method))
    pick = torch.median if method == 'median' else torch.min
    counts = np.bincount(nn[nn >= 0], minlength=n_proto)
    for k in range(n_proto):
        sel = sim[nn == k]
        assert sel.size == counts[k]
        if sel.size:
            assert got[k] == pick(torch.from_numpy(sel)).item()
            assert got[k] in sel or got[k] == 0.0                      # one of the inputs (-0.0 is returned as +0.0)
        else:
            assert got[k] == 1.0


def test_cases_cover_the_counts_and_the_masked_third():
    nn, _ = R.case(64 * 96, 300, 'uniform')
    counts = np.bincount(nn[nn >= 0], minlength=300)
    assert set(R.SMALL_COUNTS) <= set(counts.tolist()) and counts[299] == 0
    assert 0.30 < (nn < 0).mean() < 0.36
    nn, _ = R.case(50 * 77, 1, 'uniform')
    assert (nn == 0).sum() == nn.size - nn.size // 3
    _, sim = R.case(50 * 77, 7, 'signs')
    assert np.signbit(sim[sim == 0]).any() and not np.signbit(sim[sim == 0]).all() and (sim < 0).any() and (sim > 0).any()


def test_keys_order_as_the_floats_and_round_trip():
    v = np.array([-np.inf, -1.0, -1e-30, -0.0, 0.0, 1e-45, 1e-30, 0.5, 1.0, np.inf], dtype=np.float32)
    k = R.keys(v)
    assert np.all(np.diff(k.astype(np.int64)) >= 0) and k[3] == k[4] == 0x80000000
    assert np.array_equal(R.key_to_float(k), v)                        # (-0.0 == 0.0)


def test_unknown_method_is_refused_before_any_other_check(monkeypatch):
    from mulactseg_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    t = torch.zeros((1, 4, 8, 8))
    args = (t, torch.zeros((1, 3, 8, 8)), torch.zeros((1, 2, 3), dtype=torch.uint8), torch.zeros((1, 8, 8), dtype=torch.bool),
            torch.zeros((1, 8, 8), dtype=torch.int64))
    for bad in ('mean', 'Median', '', None):
        with pytest.raises(NotImplementedError):
            ops.stage2_pseudo_labels(*args, include_onehot=True, threshold_method=bad)
        with pytest.raises(NotImplementedError):
            ops.stage2_thresholds(torch.zeros(4, dtype=torch.int32), torch.zeros(4), 1, bad)
    for good in R.METHODS:                                              # a known method reaches the next check: CPU tensors
        with pytest.raises(_lib.MulActSegHipError, match="must live on the GPU"):
            ops.stage2_pseudo_labels(*args, include_onehot=True, threshold_method=good)
    with pytest.raises(_lib.MulActSegHipError, match="must live on the GPU"):
        ops.stage2_pseudo_labels(*args)


GENERATORS = ("eval_save_cosplbl_prop", "eval_save_cosplbl_prop_includeonehot", "eval_save_cosplbl_prop_onehotignore",
              "eval_save_cosplbl_prop_includeonehot_slide", "eval_save_cosplbl_prop_includeonehot_voc",
              "eval_save_cosplbl_prop_includeonehot_voc_ms")


@pytest.mark.parametrize("name", GENERATORS)
def test_every_generator_hands_the_flag_to_ops(name, monkeypatch):
    import importlib
    from mulactseg_amd import ops
    mod = importlib.import_module("mulactseg_amd.trainer." + name)
    seen = []

    def fake(feats, logits, targets, spmasks, superpixels, include_onehot=True, threshold_method='median'):
        seen.append((include_onehot, threshold_method))
        return torch.zeros(1)
    monkeypatch.setattr(ops, "stage2_pseudo_labels", fake)
    t = torch.zeros(1)
    for ns, want in ((types.SimpleNamespace(cosprop_threshold_method='min'), 'min'),
                     (types.SimpleNamespace(cosprop_threshold_method='median'), 'median'),
                     (types.SimpleNamespace(), 'median')):                 # (a trainer built by hand, without the flag)
        tr = object.__new__(mod.ActiveTrainer)
        tr.args = ns
        tr.pseudo_label_generation(t, t, t, t, t, t)
        assert seen[-1] == (mod.ActiveTrainer.include_onehot, want)
    object.__new__(mod.ActiveTrainer).pseudo_label_generation(t, t, t, t, t, t)      # (and without a namespace at all)
    assert seen[-1] == (mod.ActiveTrainer.include_onehot, 'median')


def test_parsers_accept_the_flag_and_start_up_rejects_an_unknown_method():
    from mulactseg_amd.utils import common, common_voc
    for mod in (common, common_voc):
        p = mod.get_parser()
        assert p.parse_args([]).cosprop_threshold_method == 'median'
        assert p.parse_args(['--cosprop_threshold_method', 'min']).cosprop_threshold_method == 'min'
    a = common.get_parser().parse_args([])
    common.arg_assert(a)
    a.cosprop_threshold_method = 'min'
    common.arg_assert(a)
    a.cosprop_threshold_method = 'mean'
    with pytest.raises(NotImplementedError, match="cosprop_threshold_method"):
        common.arg_assert(a)


def test_trainer_constructor_rejects_an_unknown_method(monkeypatch):
    """A driver that skips arg_assert still stops before the first picture."""
    from mulactseg_amd.trainer import eval_save_cosplbl_prop_includeonehot as G
    from mulactseg_amd.trainer import eval_within_multihot

    def parent_init(self, args, logger, selection_iter):
        self.args = args
    monkeypatch.setattr(eval_within_multihot.ActiveTrainer, "__init__", parent_init)
    assert G.ActiveTrainer(types.SimpleNamespace(val_batch_size=1, cosprop_threshold_method='min'), None, 1).save_dir is None
    assert G.ActiveTrainer(types.SimpleNamespace(val_batch_size=1), None, 1).save_dir is None
    with pytest.raises(NotImplementedError):
        G.ActiveTrainer(types.SimpleNamespace(val_batch_size=1, cosprop_threshold_method='mean'), None, 1)


def test_abi_declares_the_two_entry_points_and_keeps_version_9():
    from mulactseg_amd import _lib
    header = open(os.path.join(ROOT, "include", "mulactseg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+mas_stage2_thresholds\s*\(\s*const int32_t\*\s*nn_proto,\s*const float\*\s*nn_sim,\s*int HW,\s*int n_proto,\s*int method,"
                     r"\s*void\*\s*scratch,\s*int64_t scratch_bytes,\s*float\*\s*thr,\s*void\*\s*stream\s*\)\s*;", code)
    assert re.search(r"\bint64_t\s+mas_stage2_thresholds_scratch_bytes\s*\(\s*int n_proto,\s*int method\s*\)\s*;", code)
    assert len(_lib.SIGNATURES["mas_stage2_thresholds"][1]) == 9 and len(_lib.SIGNATURES["mas_stage2_thresholds_scratch_bytes"][1]) == 2
    assert int(re.search(r"#define MAS_ABI_VERSION (\d+)", header).group(1)) == 9 == _lib.ABI_VERSION
    for name, value in (("MEDIAN", _lib.STAGE2_THR_MEDIAN), ("MIN", _lib.STAGE2_THR_MIN)):
        assert int(re.search(r"#define MAS_STAGE2_THR_%s (\d+)" % name, header).group(1)) == value
    assert (_lib.STAGE2_THR_MEDIAN, _lib.STAGE2_THR_MIN) == (0, 1)


def test_argument_errors_launch_nothing():
    """The entry point refuses an unknown method, missing pointers and a short or misaligned scratch before it touches a device
    (this machine may have none)."""
    from mulactseg_amd import _lib
    lib = _lib.load()
    size = lib.mas_stage2_thresholds_scratch_bytes
    assert size(7, _lib.STAGE2_THR_MIN) >= 7 * 4 and size(7, _lib.STAGE2_THR_MEDIAN) >= 7 * (256 + 2) * 4
    assert size(7, 2) == -2 and size(7, -1) == -2 and size(0, 0) == -6 and size(1 << 23, 0) == -6
    assert lib.mas_stage2_thresholds(None, None, 16, 1, 2, None, 0, None, None) == -2            # the method first
    assert lib.mas_stage2_thresholds(None, None, 16, 1, 0, None, 0, None, None) == -1
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    assert lib.mas_stage2_thresholds(p, p, 0, 1, 0, p, 2048, p, None) == -2
    assert lib.mas_stage2_thresholds(p, p, 16, 0, 0, p, 2048, p, None) == -6
    assert lib.mas_stage2_thresholds(p, p, 16, 1, 0, p, size(1, 0) - 1, p, None) == -7
    assert lib.mas_stage2_thresholds(p, p, 16, 1, 0, p + 4, 2048, p, None) == -5
