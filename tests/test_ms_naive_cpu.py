"""The naive arg-max pseudo labels of VOC (the reference README's "Naive Inference", single-scale and multi-scale + flip) without a GPU:
the two generator modules and their save directories, the ``eval_spx_identity`` transform, the ABI row of ``mas_ms_naive_plbl``, the
wrapper's argument checks, the CPU op against the reference's chain, and the numpy restatement (tests/ms_naive_restated.py) against
float64 compositions and the reference's MeanIoU loop."""
import os
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ms_ensemble_restated as E
import ms_naive_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_generator_modules_import_and_are_threaded():
    import importlib
    from mulactseg_amd.trainer import eval_save_cosplbl_prop_includeonehot_voc as base
    for name in ("eval_save_cosplbl_naive_voc", "eval_save_cosplbl_naive_voc_ms"):
        mod = importlib.import_module("mulactseg_amd.trainer." + name)
        assert issubclass(mod.ActiveTrainer, base.ActiveTrainer)
        assert mod.ActiveTrainer.threaded_generation is True
        assert mod.ActiveTrainer.vis_fill == 21 and mod.ActiveTrainer.extra_channels == 0


@pytest.mark.parametrize("name, ptype, want", [("eval_save_cosplbl_naive_voc", "naive_argmax", "plbl_gen_naive_argmax"),
                                               ("eval_save_cosplbl_naive_voc", None, "plbl_gen"),
                                               ("eval_save_cosplbl_naive_voc_ms", None, "plbl_gen_ms"),
                                               ("eval_save_cosplbl_naive_voc_ms", "naive_argmax", "plbl_gen_naive_argmax")])
def test_the_generators_write_where_the_reference_does(tmp_path, name, ptype, want):
    import importlib
    mod = importlib.import_module("mulactseg_amd.trainer." + name)
    tr = object.__new__(mod.ActiveTrainer)
    tr.save_dir = None
    tr.args = types.SimpleNamespace(init_checkpoint=str(tmp_path / 'run' / 'checkpoint01.tar'), plbl_type=ptype)
    assert tr._save_dir() == str(tmp_path / 'run' / want / 'round_01')
    assert os.path.isdir(tr._save_dir())


def test_the_identity_transform_is_offered_with_two_maps():
    from mulactseg_amd.dataloader import transform
    from mulactseg_amd.dataloader.device_transforms import DeviceIdentity, DeviceTrainAugment
    args = types.SimpleNamespace(ignore_idx=255, nseg=32, load_smaller_spx=False)
    t = transform.get_train_transform_voc(args, 'eval_spx_identity')
    assert isinstance(t, DeviceIdentity) and isinstance(t, DeviceTrainAugment) and t.n_maps == 2
    assert t.pad_values == [255, 32] and t.scale_range == (1.0, 1.0)
    assert transform.get_train_transform_voc(args, 'eval_spx_identity_ms').n_maps == 0        # (its twin is unchanged)


def _f64_mean(lq, sizes, flips, H, W):
    acc = 0
    for q, (Hs, Ws), fl in zip(lq, sizes, flips):
        s = F.interpolate(torch.from_numpy(q).double()[None], size=(Hs, Ws), mode='bilinear', align_corners=False)
        if fl:
            s = s.flip(-1)
        acc = acc + F.interpolate(s, size=(H, W), mode='bilinear', align_corners=False)
    return (acc / len(lq))[0].numpy()


def _logits(rs, sizes, C):
    return [(rs.uniform(-1, 1, (C, 1, 1)) + 0.3 * rs.uniform(-1, 1, (C, E.quarter_size(Hs), E.quarter_size(Ws)))).astype(np.float32)
            for Hs, Ws in sizes]


@pytest.mark.parametrize("H, W, which", [(20, 28, range(10)), (37, 23, [3, 8]), (9, 13, [2])])
def test_the_restatement_equals_float64_compositions_away_from_ties(H, W, which):
    rs = np.random.RandomState(H * 31 + W)
    sizes, flips = E.tta_sizes(H, W)
    sizes, flips = [sizes[i] for i in which], [flips[i] for i in which]
    lq = _logits(rs, sizes, 21)
    m64 = _f64_mean(lq, sizes, flips, H, W)
    top = np.sort(m64, axis=0)
    clear = top[-1] - top[-2] > 1e-5
    got = R.labels(lq, sizes, flips, (H, W))
    assert got.dtype == np.int64 and got.shape == (H, W) and got.min() >= 0 and got.max() < 21
    assert np.array_equal(got[clear], m64.argmax(axis=0)[clear]) and clear.mean() > 0.95
    assert np.array_equal(got, np.argmax(E.ms_ensemble([q[:1] for q in lq], lq, sizes, flips, (H, W))[1], axis=0))


def test_ties_take_the_first_channel_and_nan_follows_the_torch_rule():
    m = np.zeros((5, 2, 4), dtype=np.float32)
    m[1, 0, 0] = m[3, 0, 0] = 2.0                              # tie 1 / 3 -> 1
    m[:, 0, 1] = [np.nan, 5.0, np.nan, 0.0, 0.0]              # first NaN -> 0
    m[:, 0, 2] = [1.0, 9.0, np.nan, np.nan, 0.0]              # -> 2
    m[:, 0, 3] = -np.inf                                       # all equal -> 0
    got = R.first_argmax(m)
    assert np.array_equal(got, torch.from_numpy(m).max(dim=0)[1].numpy())
    assert got[0].tolist() == [1, 0, 2, 0] and got[1].tolist() == [0, 0, 0, 0]
    # the division by n can make two different sums equal: the comparison is on the mean, so the first channel wins
    n = np.float32(10)
    a = next(v for v in (np.float32(1.5) + np.float32(k) * np.float32(2 ** -22) for k in range(64))
             if np.nextafter(v, np.float32(2)) / n == v / n)
    b = np.nextafter(a, np.float32(2))
    lq = [np.asarray([a, b], dtype=np.float32).reshape(2, 1, 1)] + [np.zeros((2, 1, 1), np.float32)] * 9
    m = R.mean_logits(lq, [(1, 1)] * 10, [False] * 10, (1, 1))
    assert m[0, 0, 0] == m[1, 0, 0] and R.labels(lq, [(1, 1)] * 10, [False] * 10, (1, 1))[0, 0] == 0


def test_the_restated_counters_equal_the_reference_loop_with_the_void_class():
    from mulactseg_amd.utils.miou import MeanIoU
    rs = np.random.RandomState(4)
    H, W, K = 40, 56, 22
    lab = rs.randint(0, 21, size=(H, W))                        # 21 channels: class 21 is never predicted
    t = lab.copy()
    t[rs.uniform(size=t.shape) < 0.3] = 5
    t[:, :7] = 21                                               # the loader's void 255 -> 21
    t[0, :] = 255                                               # (an ignore label would be skipped; the VOC loader leaves none)
    got = R.counts(lab, t, K, 255)
    assert np.array_equal(got, R.meaniou_loop(lab, t, K, 255)) and got[3 * K:].tolist() == [0, 0, 0]
    m = MeanIoU(K, 255)
    m._counts = torch.from_numpy(got)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ious, precs, recs = m._after_epoch_ipr()
        mprec = np.mean(precs)
    assert ious[21] == 0.0 and recs[21] == 0.0 and np.isnan(precs[21]) and np.isnan(mprec)
    assert '%.2f' % mprec == 'nan'


def test_the_entry_point_is_declared_bound_and_built():
    from mulactseg_amd import _lib
    assert _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "mulactseg_hip.h")) as f:
        text = f.read()
    assert "int mas_ms_naive_plbl(" in text and "#define MAS_ABI_VERSION 9" in text
    assert len(_lib.SIGNATURES["mas_ms_naive_plbl"][1]) == 12
    with open(os.path.join(ROOT, "mulactseg_amd", "csrc", "Makefile")) as f:
        assert "ms_naive.hip" in f.read()


def test_the_wrapper_rejects_bad_sources_before_touching_a_device():
    from mulactseg_amd import ops
    z = torch.zeros(1, 21, 3, 4)
    with pytest.raises(ValueError):
        ops.ms_naive_labels([], [], [], (10, 14))
    with pytest.raises(ValueError):
        ops.ms_naive_labels([z] * 17, [(12, 16)] * 17, [False] * 17, (10, 14))
    with pytest.raises(ValueError):
        ops.ms_naive_labels([z], [(12, 16), (12, 16)], [False], (10, 14))
    with pytest.raises(ValueError):
        ops.ms_naive_labels([z], [(16, 16)], [False], (10, 14))                  # 16 x 16 emits 4 x 4, not 3 x 4
    with pytest.raises(ValueError):
        ops.ms_naive_labels([z], [(12, 16)], [False], (0, 14))
    with pytest.raises(ValueError):
        ops.ms_naive_labels([z, z[:, :20]], [(12, 16)] * 2, [False] * 2, (10, 14))
    with pytest.raises(TypeError):
        ops.ms_naive_labels([z.double()], [(12, 16)], [False], (10, 14))
    with pytest.raises(ValueError):
        ops.ms_naive_labels([torch.zeros(1, 256, 3, 4)], [(12, 16)], [False], (10, 14))
    t = torch.zeros(1, 10, 14, dtype=torch.int64)
    with pytest.raises(ValueError):                                               # counts need num_classes
        ops.ms_naive_labels([z], [(12, 16)], [False], (10, 14), targets=t, counts=torch.zeros(69, dtype=torch.int64))
    with pytest.raises(ValueError):                                               # K < C
        ops.ms_naive_labels([z], [(12, 16)], [False], (10, 14), targets=t, counts=torch.zeros(63, dtype=torch.int64), num_classes=20)
    with pytest.raises(ValueError):                                               # counts of another K
        ops.ms_naive_labels([z], [(12, 16)], [False], (10, 14), targets=t, counts=torch.zeros(63, dtype=torch.int64), num_classes=22)
    with pytest.raises(ValueError):                                               # targets of another size
        ops.ms_naive_labels([z], [(12, 16)], [False], (10, 14), targets=t[:, :9], counts=torch.zeros(69, dtype=torch.int64),
                            num_classes=22)


def test_the_cpu_op_is_the_reference_chain():
    from mulactseg_amd import ops
    rs = np.random.RandomState(6)
    H, W = 23, 31
    sizes, flips = E.tta_sizes(H, W)
    lq = [torch.from_numpy(q)[None] for q in _logits(rs, sizes, 21)]
    t = torch.from_numpy(rs.randint(0, 22, size=(1, H, W)))
    counts = torch.zeros(3 * 22 + 3, dtype=torch.int64)
    got = ops.ms_naive_labels(lq, sizes, flips, (H, W), targets=t, counts=counts, num_classes=22)
    # eval_save_cosplbl_naive_voc_ms.py:59-87: feat_forward's F.interpolate, flip, tF.resize (bilinear, no antialias), mean, max
    outs = []
    for z, (Hs, Ws), fl in zip(lq, sizes, flips):
        o = F.interpolate(z, size=(Hs, Ws), mode='bilinear', align_corners=False)
        if fl:
            o = o.flip(-1)
        outs.append(F.interpolate(o, size=(H, W), mode='bilinear', align_corners=False))
    acc = outs[0]
    for o in outs[1:]:
        acc = acc + o
    want = (acc / len(outs)).max(dim=1)[1]
    assert got.dtype == torch.int64 and tuple(got.shape) == (1, H, W) and torch.equal(got, want)
    ref = torch.stack(outs).mean(dim=0).max(dim=1)[1]                            # (the reference's stack().mean(): away from ties)
    assert (got == ref).float().mean() > 0.99
    assert np.array_equal(counts.numpy(), R.meaniou_loop(got.numpy(), t.numpy(), 22, 255))
    again = ops.ms_naive_labels(lq, sizes, flips, (H, W), targets=t, counts=counts, num_classes=22)
    assert torch.equal(again, got) and np.array_equal(counts.numpy(), 2 * R.meaniou_loop(got.numpy(), t.numpy(), 22, 255))
    one = ops.ms_naive_labels(lq[2:3], sizes[2:3], flips[2:3], (H, W))           # n = 1, the identity geometry: the upsampling's arg-max
    assert torch.equal(one, F.interpolate(lq[2], size=(H, W), mode='bilinear', align_corners=False).max(dim=1)[1])
