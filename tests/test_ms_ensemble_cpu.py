"""The multi-scale + flip stage-2 pseudo labels of VOC without a GPU: the ``eval_spx_identity_ms`` transform, the
``eval_region_voc_all_ms`` loader, the save directory of the ``_ms`` generator, the ABI row of ``mas_ms_ensemble`` and the numpy
restatement of its arithmetic (tests/ms_ensemble_restated.py) against float64 ``F.interpolate`` compositions."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ms_ensemble_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_multiscale_transform_is_offered_with_the_reference_factors_and_order():
    from mulactseg_amd.dataloader import transform
    from mulactseg_amd.dataloader.device_transforms import DeviceMultiScaleFlip
    args = types.SimpleNamespace(ignore_idx=255, nseg=32, load_smaller_spx=False)
    t = transform.get_train_transform_voc(args, 'eval_spx_identity_ms')
    assert isinstance(t, DeviceMultiScaleFlip) and t.n_maps == 0
    assert t.factors == (0.5, 0.75, 1.0, 1.25, 1.5)
    g = t.geometry(375, 500)
    assert [(th, tw) for th, tw, _ in g] == [(int(f * 375), int(f * 500)) for f in t.factors] * 2
    assert [fl for _, _, fl in g] == [False] * 5 + [True] * 5
    assert g[2] == (375, 500, False) and g[7] == (375, 500, True)


def test_the_multiscale_loader_module_exists():
    from mulactseg_amd.dataloader import eval_region_voc_all, eval_region_voc_all_ms
    assert issubclass(eval_region_voc_all_ms.RegionVOCOr, eval_region_voc_all.RegionVOCOr)
    assert eval_region_voc_all_ms.RegionVOCOr.__getitem__ is not eval_region_voc_all.RegionVOCOr.__getitem__


@pytest.mark.parametrize("ptype, want", [(None, 'plbl_gen_ms'), ('ms', 'plbl_gen_ms'), ('foo', 'plbl_gen_foo')])
def test_the_ms_generator_writes_where_the_reference_does(tmp_path, ptype, want):
    from mulactseg_amd.trainer import eval_save_cosplbl_prop_includeonehot_voc_ms as mod
    tr = object.__new__(mod.ActiveTrainer)
    tr.save_dir = None
    tr.args = types.SimpleNamespace(init_checkpoint=str(tmp_path / 'run' / 'checkpoint03.tar'), plbl_type=ptype)
    assert tr._save_dir() == str(tmp_path / 'run' / want / 'round_03')
    assert os.path.isdir(tr._save_dir())


def test_the_entry_point_is_bound_and_declared():
    from mulactseg_amd import _lib
    assert "mas_ms_ensemble" in _lib.SIGNATURES and _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "mulactseg_hip.h")) as f:
        text = f.read()
    assert "int mas_ms_ensemble(" in text and "#define MAS_ABI_VERSION 9" in text and "#define MAS_MS_MAX_SOURCES 16" in text
    with open(os.path.join(ROOT, "mulactseg_amd", "csrc", "Makefile")) as f:
        assert "ms_ensemble.hip" in f.read()


def test_the_wrapper_rejects_source_counts_before_touching_a_device():
    from mulactseg_amd import ops
    with pytest.raises(ValueError):
        ops.ms_ensemble([], [], [], [], (4, 4))
    q = torch.zeros(1, 2, 1, 1)
    with pytest.raises(ValueError):
        ops.ms_ensemble([q] * 17, [q] * 17, [(4, 4)] * 17, [False] * 17, (4, 4))
    assert ops.quarter_size(513) == 129 and ops.quarter_size(4) == 1 and ops.quarter_size(5) == 2
    assert all(ops.quarter_size(n) == R.quarter_size(n) == -(-n // 4) for n in range(1, 200))


def _f64_reference(qs, sizes, flips, H, W, normalise):
    acc = 0
    for q, (Hs, Ws), fl in zip(qs, sizes, flips):
        s = F.interpolate(torch.from_numpy(q).double()[None], size=(Hs, Ws), mode='bilinear', align_corners=False)
        if fl:
            s = s.flip(-1)
        acc = acc + F.interpolate(s, size=(H, W), mode='bilinear', align_corners=False)
    m = acc / len(qs)
    return (F.normalize(m, dim=1) if normalise else m)[0].numpy()


@pytest.mark.parametrize("H, W, n", [(20, 28, 10), (37, 23, 2), (9, 13, 1)])
def test_the_restatement_equals_float64_interpolate_compositions(H, W, n):
    rs = np.random.RandomState(H * 100 + W)
    sizes, flips = R.tta_sizes(H, W)
    sizes, flips = sizes[:n] if n != 2 else [sizes[3], sizes[8]], flips[:n] if n != 2 else [flips[3], flips[8]]
    Ch, C = 16, 21
    fq, lq = [], []
    for Hs, Ws in sizes:
        # (a per-channel level plus a small random texture: the f32 scales of the taps move the sample points by ~1e-7 of the size,
        # which a white-noise map would turn into differences above 1e-6)
        f = (rs.standard_normal((Ch, 1, 1)) + 0.2 * rs.standard_normal((Ch, R.quarter_size(Hs), R.quarter_size(Ws)))).astype(np.float32)
        fq.append((f / np.sqrt((f.astype(np.float64) ** 2).sum(0))).astype(np.float32))
        lq.append((rs.uniform(-1, 1, (C, 1, 1)) + 0.2 * rs.uniform(-1, 1, (C, R.quarter_size(Hs), R.quarter_size(Ws)))).astype(np.float32))
    feat, logit = R.ms_ensemble(fq, lq, sizes, flips, (H, W))
    assert feat.dtype == np.float32 and feat.shape == (Ch, H, W) and logit.shape == (C, H, W)
    assert np.abs(feat - _f64_reference(fq, sizes, flips, H, W, True)).max() <= 1e-6
    assert np.abs(logit - _f64_reference(lq, sizes, flips, H, W, False)).max() <= 1e-6
    assert np.allclose(np.sqrt((feat.astype(np.float64) ** 2).sum(0)), 1.0, atol=1e-6)


def test_identity_geometry_returns_the_input_normalised():
    rs = np.random.RandomState(1)
    x = rs.standard_normal((8, 6, 7)).astype(np.float32)
    assert np.array_equal(R.resize(x, 6, 7), x)                  # every weight is exactly 1 or 0
    feat, logit = R.ms_ensemble([x], [x[:3]], [(6, 7)], [False], (6, 7))
    assert np.array_equal(logit, x[:3])
    assert np.array_equal(feat, R.normalise(x))
    assert np.abs(feat - x / np.sqrt((x.astype(np.float64) ** 2).sum(0))).max() <= 1e-6


def test_a_flipped_source_equals_the_explicit_flip():
    rs = np.random.RandomState(2)
    q = rs.standard_normal((5, 4, 6)).astype(np.float32)
    Hs, Ws, H, W = 13, 21, 11, 17
    want = R.resize(np.ascontiguousarray(R.resize(q, Hs, Ws)[:, :, ::-1]), H, W)
    assert np.array_equal(R.source(q, Hs, Ws, True, H, W), want)
    assert not np.array_equal(R.source(q, Hs, Ws, False, H, W), want)
    ref = F.interpolate(torch.from_numpy(R.stage1(q, Hs, Ws)).double()[None].flip(-1), size=(H, W), mode='bilinear', align_corners=False)
    assert np.abs(R.source(q, Hs, Ws, True, H, W) - ref[0].numpy()).max() <= 1e-6


def test_a_zero_feature_vector_stays_zero_through_the_clamp():
    m = np.zeros((4, 3, 3), dtype=np.float32)
    m[:, 1, 1] = [3, 4, 0, 0]
    out = R.normalise(m)
    assert np.array_equal(out[:, 0, 0], np.zeros(4, np.float32)) and np.isfinite(out).all()
    assert np.array_equal(out[:, 1, 1], np.asarray([0.6, 0.8, 0, 0], np.float32))
    tiny = np.full((2, 1, 1), 1e-30, dtype=np.float32)      # sqrt(2e-60) underflows to 0 in f32: the clamp keeps the division finite
    assert np.isfinite(R.normalise(tiny)).all()
