"""``eval_city_mul_res50.sh`` on the host: the numpy restatement of the low-resolution IoU counters (csrc/lowres_iou.hip) against the
oracle and against float64 interpolation, the per-region entries of ``region_cityscapes_all`` on hand-worked regions, the import
surface of ``--method eval_naive --loader region_cityscapes_all`` and the argument checks of ``mas_lowres_iou_counts``.  The kernel
itself runs in tests/test_eval_naive_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
import lowres_iou_restated as L
import naive_plbl_restated as R
import region_all_restated as RA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed, N, CH, h, w, H, W, C):
    """Logits with exact ties (a duplicated class channel; channel C equal to a class channel) and targets with 255 and values
    outside [0, C)."""
    rs = np.random.RandomState(seed)
    zq = (2.0 * rs.randn(N, CH, h, w)).astype(np.float32)
    zq[:, 4, : h // 2] = zq[:, 2, : h // 2]
    if CH > C:
        zq[:, C, h // 2:] = zq[:, 1, h // 2:]
    t = rs.randint(0, C, size=(N, H, W)).astype(np.int64)
    t[rs.uniform(size=t.shape) < 0.1] = 255
    t[rs.uniform(size=t.shape) < 0.02] = C + 3
    t[rs.uniform(size=t.shape) < 0.01] = -1
    return zq, t


CASES = [(1, 20, 32, 64, 128, 256, 19), (2, 19, 33, 65, 129, 257, 19), (2, 22, 33, 33, 129, 129, 21), (1, 21, 24, 40, 24, 40, 21)]


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_oracle_counters_on_the_restated_upsampling(case):
    from oracle import port
    N, CH, h, w, H, W, C = case
    zq, t = _case(sum(case), N, CH, h, w, H, W, C)
    got = L.lowres_iou_counts(zq, t, H, W, C, 255)
    z = torch.from_numpy(R.upsample(zq, H, W))
    tt = torch.from_numpy(t)
    seen, correct, positive = port.iou_counts(z[:, :C].max(dim=1)[1], tt, C, 255)
    want = np.concatenate([seen, correct, positive]).astype(np.int64)
    assert np.array_equal(got[:3 * C], want)
    if CH > C:
        assert tuple(got[3 * C:]) == port.ignore_iou_counts(z.max(dim=1)[1], tt, C, 255)
    else:
        assert not got[3 * C:].any()
    assert got[3 * C] == 0 or CH > C
    assert got[:C].sum() < t.size and got[2 * C:3 * C].sum() > got[:C].sum() * 0.5


@pytest.mark.parametrize("case", [(1, 20, 32, 64, 128, 256, 19), (1, 21, 33, 41, 129, 161, 21)])
def test_restatement_equals_float64_interpolation_away_from_ties(case):
    import torch.nn.functional as F
    N, CH, h, w, H, W, C = case
    rs = np.random.RandomState(7)
    zq = (2.0 * rs.randn(N, CH, h, w)).astype(np.float32)
    z64 = F.interpolate(torch.from_numpy(zq).double(), size=(H, W), mode='bilinear', align_corners=False).numpy()
    o_cls, o_all = L.argmaxes(R.upsample(zq, H, W), C)
    s = np.sort(z64[:, :C], axis=1)
    far_cls = s[:, -1] - s[:, -2] > 1e-5
    far_all = far_cls & (np.abs(z64[:, C] - s[:, -1]) > 1e-5) if CH > C else far_cls
    assert far_all.mean() > 0.999
    assert np.array_equal(o_cls[far_cls], np.argmax(z64[:, :C], axis=1)[far_cls])
    assert np.array_equal(o_all[far_all], np.argmax(z64, axis=1)[far_all])


def test_restated_tie_and_nan_rules_are_those_of_the_fused_counter():
    """k_logits_iou: strict '>' from channel 0 -- the first maximum wins, a NaN after channel 0 never wins, a NaN in channel 0 keeps
    the arg-max at 0; channel C takes o_all only when strictly above the class maximum."""
    nan = np.float32(np.nan)
    z = np.array([[1, 3, 3, 3], [2, nan, 1, 5], [nan, 4, 5, 9], [0, 1, 1, 0.5]], dtype=np.float32).T[None, :, :, None]  # [1,4,4,1]
    o_cls, o_all = L.argmaxes(z, 3)
    assert o_cls[0, :, 0].tolist() == [1, 0, 0, 1]
    assert o_all[0, :, 0].tolist() == [1, 3, 0, 1]


def test_tally_counts_out_of_range_targets_as_positives_only():
    o = np.array([0, 1, 2, 2, 1])
    oa = np.array([0, 3, 2, 3, 1])
    t = np.array([0, 255, 7, 2, -1])
    c = L.tally(o, oa, t, 3, 255, True)
    assert c.tolist() == [1, 0, 1,  1, 0, 1,  1, 1, 2,  1, 1, 2]


# -- region_cityscapes_all ------------------------------------------------------------------------------------------------------
def _hand_picture():
    """Five regions on a 4 x 6 picture: id 0 ties between classes 3 and 1 (2 pixels each) with one 255; id 1 only 255; id 2 three
    classes, no 255; id 3 one class and a 255; id 4 listed but without pixels."""
    spx = np.array([[0, 0, 0, 0, 0, 2],
                    [1, 1, 2, 2, 2, 2],
                    [3, 3, 3, 2, 2, 2],
                    [3, 3, 3, 3, 2, 2]])
    t = np.array([[3, 1, 255, 3, 1, 5],
                  [255, 255, 5, 5, 7, 7],
                  [4, 4, 255, 5, 0, 0],
                  [4, 4, 4, 4, 5, 7]])
    return t, spx


def test_region_restatement_on_hand_worked_regions():
    t, spx = _hand_picture()
    info = RA.superpixel_info(t, spx, [0, 1, 2, 3, 4])
    # a 255 in the region: allignore False, so the classes are listed; the tie 1 / 3 comes out as argsort()[::-1] puts it
    assert info[0] == {'cls': [3, 1], 'cpx': [2, 2], 'npx': 5, 'isignore': True, 'allignore': False}
    assert info[1] == {'cls': [], 'cpx': [], 'npx': 2, 'isignore': True, 'allignore': False}          # all ignore
    # no 255 at all: the inverted flag is True and the lists stay empty
    assert info[2] == {'cls': [], 'cpx': [], 'npx': 10, 'isignore': False, 'allignore': True}
    assert info[3] == {'cls': [4], 'cpx': [6], 'npx': 7, 'isignore': True, 'allignore': False}
    assert info[4] == {'cls': [], 'cpx': [], 'npx': 0, 'isignore': False, 'allignore': True}          # no pixel


def test_region_ties_follow_numpy_argsort_reversed():
    """Classes 2, 5, 9 with 3 pixels each and class 7 with 4: descending count, ties in the order of argsort()[::-1] over the
    classes in ascending order -- the order the loader's histograms give as well."""
    from mulactseg_amd.dataloader.region_cityscapes_all import region_info
    t = np.array([2, 2, 2, 5, 5, 5, 9, 9, 9, 7, 7, 7, 7, 255])
    spx = np.zeros_like(t)
    want_order = np.array([3, 3, 4, 3]).argsort()[::-1]                 # counts of classes 2, 5, 7, 9
    info = RA.superpixel_info(t, spx, [0])[0]
    assert info['cls'] == [[2, 5, 7, 9][i] for i in want_order] == [7, 9, 5, 2] and info['cpx'] == [4, 3, 3, 3]
    row = np.bincount(np.where(t == 255, 19, t), minlength=20).astype(np.int64)
    assert region_info(row, 19) == info


def test_loader_entries_equal_the_restatement_on_random_regions():
    """The host half of RegionCityscapesAll (entries from the per-id histograms the kernel returns) against the restated loop."""
    from mulactseg_amd.dataloader.region_cityscapes_all import region_info
    rs = np.random.RandomState(3)
    nseg, C = 40, 19
    spx = rs.randint(0, nseg - 2, size=(48, 64))
    t = rs.choice(np.array([0, 1, 2, 3, 18, 255]), size=spx.shape, p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.1])
    t[spx < 6] = np.where(t[spx < 6] == 255, 1, t[spx < 6])                # a few regions without 255
    t[spx == 7] = 255                                                       # an all-ignore region
    counts = np.zeros((nseg, C + 1), dtype=np.int64)
    np.add.at(counts, (spx.reshape(-1), np.where(t == 255, C, t).reshape(-1)), 1)
    ids = list(range(nseg))
    want = RA.superpixel_info(t, spx, ids)
    got = {p: region_info(counts[p], C) for p in ids}
    assert got == want
    assert any(v['allignore'] for v in want.values()) and any(v['cls'] for v in want.values())


# -- the import surface and the C entry point -----------------------------------------------------------------------------------
def test_eval_script_modules_import_under_the_reference_names():
    code = ("import mulactseg_amd, importlib\n"
            "mulactseg_amd.install_aliases()\n"
            "t = importlib.import_module('trainer.eval_naive')\n"
            "d = importlib.import_module('dataloader.region_cityscapes_all')\n"
            "from mulactseg_amd.dataloader import region_cityscapes\n"
            "assert d.RegionCityscapes is region_cityscapes.RegionCityscapes\n"
            "assert issubclass(d.RegionCityscapesAll, region_cityscapes.RegionCityscapes)\n"
            "assert t.ActiveTrainer.predicts_ignore is True\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_eval_naive_builds_the_predignore_model_and_meters():
    from mulactseg_amd.trainer import active_joint_multi_predignore, eval_naive
    from mulactseg_amd.utils.miou import LogitsIoU, LowresLogitsIoU
    assert issubclass(eval_naive.ActiveTrainer, active_joint_multi_predignore.ActiveTrainer)
    assert eval_naive.ActiveTrainer.get_al_model is active_joint_multi_predignore.ActiveTrainer.get_al_model
    assert issubclass(LowresLogitsIoU, LogitsIoU)


def test_get_active_dataset_builds_plain_region_sets_for_this_loader(tmp_path):
    from mulactseg_amd.dataloader import get_active_dataset, region_cityscapes
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=2, H=32, W=48, nseg=16)
    a = helpers.cityscapes_tree_args(tree, tmp_path / 'run', ['--stage2', '--method', 'eval_naive', '--loader', 'region_cityscapes_all',
                                                              '--train_transform', 'eval_spx', '--val_batch_size', '1'])
    a.or_labeling = False
    aset = get_active_dataset(a, train_transform=a.train_transform)
    assert type(aset.trg_pool_dataset) is region_cityscapes.RegionCityscapes
    assert type(aset.trg_label_dataset) is region_cityscapes.RegionCityscapes
    assert len(aset.trg_pool_dataset) == 2


def test_lowres_iou_argument_errors_are_reported_without_the_gpu():
    from mulactseg_amd import _lib, ops
    lib = _lib.load()
    fake = 256                                                   # never dereferenced: every call below fails its argument checks
    assert lib.mas_lowres_iou_counts(None, fake, 1, 20, 8, 8, 32, 32, 19, 255, fake, None) == -1
    assert lib.mas_lowres_iou_counts(fake, None, 1, 20, 8, 8, 32, 32, 19, 255, fake, None) == -1
    assert lib.mas_lowres_iou_counts(fake, fake, 1, 20, 8, 8, 32, 32, 19, 255, None, None) == -1
    assert lib.mas_lowres_iou_counts(fake, fake, 1, 21, 8, 8, 32, 32, 19, 255, fake, None) == -3          # channels not C, C + 1
    assert lib.mas_lowres_iou_counts(fake, fake, 1, 40, 8, 8, 32, 32, 39, 255, fake, None) == -3          # above MAS_MAX_CLASSES
    assert lib.mas_lowres_iou_counts(fake, fake, 1, 20, 64, 64, 32, 32, 19, 255, fake, None) == -2        # a downsampling
    assert lib.mas_lowres_iou_counts(fake, fake, 1, 20, 8, 8, 8, 64, 19, 255, fake, None) == -2           # wider than x6
    assert lib.mas_lowres_iou_counts(fake, fake, 0, 20, 8, 8, 32, 32, 19, 255, fake, None) == -2
    z = torch.zeros((1, 20, 8, 8))
    assert not ops.lowres_iou_supported(z, (32, 32))
    with pytest.raises(_lib.MulActSegHipError, match="GPU"):
        ops.lowres_iou_counts(z, torch.zeros((1, 32, 32), dtype=torch.int64), (32, 32), 19, 255)
