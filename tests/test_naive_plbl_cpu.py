"""The two stage-2 ablations of paper Fig. 7 without a GPU: the numpy restatement of the naive top-1 labeller (csrc/naive_plbl.hip)
against the reference's torch lines and float64, the scatter_max -> one-hot restatement (k_spx_max_onehot) against a per-id loop,
the flags, save directories, pred_ignore rule, transform and the trainers' choice of generation loop."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import naive_plbl_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMS = [(32, 64, 128, 256), (33, 41, 129, 161), (16, 32, 16, 32)]


def _gap64(zq, H, W):
    """float64 interpolation of the logits and the gap between the two largest values per pixel."""
    z = torch.from_numpy(np.asarray(zq, dtype=np.float64))
    if tuple(z.shape[2:]) != (H, W):
        z = F.interpolate(z, size=(H, W), mode='bilinear', align_corners=False)
    top = torch.topk(z, 2, dim=1)[0]
    return z.numpy(), (top[:, 0] - top[:, 1]).numpy()


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("C", [20, 21])
def test_restatement_agrees_with_the_reference_lines_and_float64(geom, C):
    h, w, H, W = geom
    rs = np.random.RandomState(h + C)
    zq = rs.randn(2, C, h, w).astype(np.float32)
    mask = rs.uniform(size=(2, H, W)) < 0.6
    z64, gap = _gap64(zq, H, W)
    clear = gap > 1e-4                                        # (float32 rounding of the interpolation moves values by <= 1e-5)
    got = R.naive_labels(zq, H, W, mask, 0.0)
    ref = R.reference_lines(zq, H, W, mask, 0.0)
    assert np.array_equal(got[clear], ref[clear])
    assert np.array_equal(got == 255, ~mask)
    want64 = np.where(mask, z64.argmax(axis=1), 255)
    assert np.array_equal(got[clear], want64[clear])
    assert clear.mean() > 0.99
    if (h, w) == (H, W):                                       # identity: the logits themselves, every pixel exact
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("th", [0.3, 0.5])
def test_threshold_mode_replaces_the_mask_everywhere(th):
    h, w, H, W = 32, 64, 128, 256
    rs = np.random.RandomState(7)
    zq = (2.0 * rs.randn(1, 20, h, w)).astype(np.float32)
    mask = np.zeros((1, H, W), dtype=bool)                     # ignored: th > 0 labels every confident pixel
    z64, _ = _gap64(zq, H, W)
    p64 = 1.0 / np.exp(z64 - z64.max(axis=1, keepdims=True)).sum(axis=1)
    got = R.naive_labels(zq, H, W, mask, th)
    ref = R.reference_lines(zq, H, W, mask, th)
    far = np.abs(p64 - th) > 1e-5
    assert np.array_equal(got[far] != 255, p64[far] > th)
    assert np.array_equal(got[far] != 255, ref[far] != 255)
    assert 0 < (got != 255).mean() < 1


def test_ties_take_the_first_channel_and_nan_the_first_nan():
    C, H, W = 5, 4, 8
    z = np.zeros((1, C, H, W), dtype=np.float32)
    z[0, 1] = z[0, 3] = 2.0                                    # tie between 1 and 3 -> 1
    z[0, :, 0, 1] = [np.nan, 5.0, np.nan, 0.0, 0.0]           # first NaN -> 0
    z[0, :, 0, 2] = [1.0, 9.0, np.nan, np.nan, 0.0]           # -> 2
    z[0, :, 0, 3] = [-np.inf, -np.inf, -np.inf, -np.inf, -np.inf]      # all equal -> 0
    mask = np.ones((1, H, W), dtype=bool)
    got = R.naive_labels(z, H, W, mask, 0.0)
    ref = torch.from_numpy(z).max(dim=1)[1].numpy()
    assert np.array_equal(got, ref)
    assert got[0, 1, 1] == 1 and got[0, 0, 1] == 0 and got[0, 0, 2] == 2 and got[0, 0, 3] == 0
    th = R.naive_labels(z, H, W, mask, 0.1)
    assert th[0, 0, 1] == 255 and th[0, 0, 2] == 255          # NaN -> p_max NaN -> not kept (as the reference)
    assert np.array_equal(th[0, 0, 1:3], R.reference_lines(z, H, W, mask, 0.1)[0, 0, 1:3])


def test_the_cpu_op_is_the_reference_chain():
    from mulactseg_amd import ops
    rs = np.random.RandomState(3)
    zq = torch.from_numpy(rs.randn(1, 20, 16, 32).astype(np.float32))
    mask = torch.from_numpy(rs.uniform(size=(1, 64, 128)) < 0.5)
    for th in (0.0, 0.4):
        got = ops.naive_pseudo_labels(zq, (64, 128), mask, th)
        assert np.array_equal(got.numpy(), R.reference_lines(zq.numpy(), 64, 128, mask.numpy(), th))


def _target_and_ids(seed, H=64, W=96, nseg=40, holes=(3, 17, 39)):
    rs = np.random.RandomState(seed)
    spx = rs.randint(0, nseg, size=(H, W))
    for hole in holes:
        spx[spx == hole] = (hole + 1) % nseg
    dom = rs.randint(0, 20, size=nseg)
    t = dom[spx]
    t[rs.uniform(size=t.shape) < 0.05] = 255
    t[np.isin(spx, rs.choice(nseg, 10, replace=False))] = 255      # unselected superpixels
    return t, spx


def test_scatter_max_onehot_restatement_against_the_per_id_loop():
    for seed in range(4):
        t, spx = _target_and_ids(seed)
        rows, mask = R.spx_max_onehot(t, spx, 40, 20)
        loop = R.spx_max_onehot_loop(t, spx, 20)
        n = loop.shape[0]
        assert np.array_equal(rows[:n], loop)
        assert np.array_equal(mask, t != 255)
        for hole in (3, 17):                                   # an id with no pixel: the row of value 0
            assert rows[hole].tolist() == [1] + [0] * 19
        assert np.all(rows.sum(axis=1) == 1)


def test_rows_sized_nseg_extend_the_max_plus_one_table_with_unused_rows():
    t, spx = _target_and_ids(5, nseg=40, holes=(3, 36, 37, 38, 39))
    loop = R.spx_max_onehot_loop(t, spx, 20)
    rows, mask = R.spx_max_onehot(t, spx, 40, 20)
    assert loop.shape[0] == 36 and rows.shape[0] == 40
    assert np.array_equal(rows[:36], loop)
    # the extra rows belong to ids no pixel carries, so no masked pixel ever looks one up
    assert not np.isin(spx[mask], np.arange(36, 40)).any()


def test_plbl_th_default_save_dirs_and_the_pred_ignore_rule():
    from mulactseg_amd.dataloader.region_cityscapes_dom_w_gt import pred_ignore_of
    from mulactseg_amd.trainer import eval_save_cosplbl_prop_onehotignore as B
    from mulactseg_amd.trainer import eval_save_naiveplbl as A
    from mulactseg_amd.utils.common import get_parser
    a = get_parser().parse_args([])
    assert a.plbl_th == 0.0 and isinstance(a.plbl_th, float)
    assert get_parser().parse_args(['--plbl_th', '0.9']).plbl_th == 0.9
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        for cls, ptype, want in ((A.ActiveTrainer, 'naive', 'plbl_gen_naive'), (B.ActiveTrainer, None, 'plbl_gen'),
                                 (A.ActiveTrainer, None, 'plbl_gen')):
            fake = types.SimpleNamespace(args=types.SimpleNamespace(init_checkpoint='%s/run/checkpoint05.tar' % d, plbl_type=ptype),
                                         save_dir=None)
            assert cls._save_dir(fake) == '%s/run/%s/round_05' % (d, want)
    assert pred_ignore_of(types.SimpleNamespace(init_checkpoint='checkpoint/x_method-active_joint_multi_predignore_lossdecomp-_/c.tar'))
    assert not pred_ignore_of(types.SimpleNamespace(init_checkpoint='checkpoint/deepstem50_do_ppredclsbal/checkpoint03.tar'))


def test_the_three_map_transform_is_registered():
    from mulactseg_amd.dataloader.device_transforms import DeviceResize, DeviceResizeThreeMaps
    from mulactseg_amd.dataloader.transform import get_train_transform
    a = types.SimpleNamespace(ignore_idx=255, nseg=2048, load_smaller_spx=False)
    t = get_train_transform(a, 'eval_dom_gt_spx')
    assert isinstance(t, DeviceResizeThreeMaps) and t.n_maps == 3 and t.target == (1024, 2048)
    assert t.pad_values == [255, 255] and t._third.pad_values == [2048]
    e = get_train_transform(a, 'eval_spx')
    assert type(e) is DeviceResize and e.n_maps == 2
    with pytest.raises(ValueError, match="three maps"):
        DeviceResizeThreeMaps((4, 4), pad_values=[255, 2048])


def test_every_generator_keeps_its_loop_and_the_new_ones_are_threaded():
    from mulactseg_amd.trainer import (eval_save_cosplbl_prop, eval_save_cosplbl_prop_includeonehot, eval_save_cosplbl_prop_includeonehot_slide,
                                       eval_save_cosplbl_prop_includeonehot_voc, eval_save_cosplbl_prop_onehotignore, eval_save_naiveplbl)
    base = eval_save_cosplbl_prop.ActiveTrainer

    def threaded(cls):
        t = cls.threaded_generation
        return (cls.pseudo_labels is base.pseudo_labels) if t is None else t
    for mod in (eval_save_cosplbl_prop, eval_save_cosplbl_prop_includeonehot, eval_save_cosplbl_prop_includeonehot_voc):
        assert threaded(mod.ActiveTrainer)
    assert not threaded(eval_save_cosplbl_prop_includeonehot_slide.ActiveTrainer)        # state between calls: one thread
    assert threaded(eval_save_naiveplbl.ActiveTrainer) and threaded(eval_save_cosplbl_prop_onehotignore.ActiveTrainer)


def test_the_entry_points_are_bound_and_declared():
    """mas_naive_plbl and mas_spx_max_onehot are declared, bound and built beside mas_ms_ensemble; adding them changes no existing
    signature, so the ABI version stays 9."""
    from mulactseg_amd import _lib
    assert _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "mulactseg_hip.h")) as f:
        text = f.read()
    assert "#define MAS_ABI_VERSION 9" in text and "#define MAS_MS_MAX_SOURCES 16" in text
    for name in ("mas_ms_ensemble", "mas_naive_plbl", "mas_spx_max_onehot"):
        assert name in _lib.SIGNATURES and ("int %s(" % name) in text
    with open(os.path.join(ROOT, "mulactseg_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "ms_ensemble.hip" in mk and "naive_plbl.hip" in mk and "labels.hip" in mk


def test_a_library_without_the_new_entry_points_is_refused(tmp_path, monkeypatch):
    """A version-9 library built before the two entry points existed: load() names the missing symbols instead of binding part of
    the table."""
    import subprocess
    from mulactseg_amd import _lib
    src = tmp_path / "old.c"
    src.write_text("int mas_abi_version(void) { return 9; }\n")
    so = tmp_path / "libold.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)])
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.MulActSegHipError, match="mas_naive_plbl.*stale build"):
        _lib.load()
