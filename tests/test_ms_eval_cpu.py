"""Multi-scale + flip evaluation (``--method eval_naive_ms``) without a GPU: the numpy restatement of the counters
(tests/ms_eval_restated.py) against the reference's meters on the ATen mean logits, the CPU form of ``ops.ms_iou_counts``, the inputs
of the GPU cases (that they exercise both arg-maxes), the flags, the own-size evaluation set on Cityscapes- and VOC-shaped trees, and
the ABI rows of the new entry points.  The kernel runs in tests/test_ms_eval_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
import ms_ensemble_restated as E
import ms_eval_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = [(20, 19), (22, 21), (21, 21)]             # (CH, K): the stage-2 models of Cityscapes and VOC, and a model without the extra channel


def _aten_mean(lq, sizes, flips, H, W):
    acc = None
    for q, (Hs, Ws), fl in zip(lq, sizes, flips):
        s = F.interpolate(torch.from_numpy(q)[None], size=(Hs, Ws), mode='bilinear', align_corners=False)
        v = F.interpolate(s.flip(-1) if fl else s, size=(H, W), mode='bilinear', align_corners=False)
        acc = v if acc is None else acc + v
    return acc / len(lq)


@pytest.mark.parametrize("CH, K", CHK)
def test_the_restatement_equals_the_reference_meters_on_the_aten_mean_logits(CH, K):
    """``MeanIoU(K)._after_step(m[:, :K].max(1)[1])`` and ``IoUIgnore(K)._after_step(m.max(1)[1])`` (trainer/eval_naive.py:61-63), the
    meters as the oracle ports them (the package's own count on the device)."""
    from oracle import port
    H, W = 37, 45
    sizes, flips = R.sources('ten', H, W)
    lq, t = R.make_case(CH + K, sizes, H, W, CH, K)
    m = _aten_mean(lq, sizes, flips, H, W)
    got = R.counts_from_mean(m[0].numpy(), t, K, 255)
    tt = torch.from_numpy(t)[None]
    seen, correct, positive = port.iou_counts(m[:, :K].max(1)[1], tt, K, 255)
    assert np.array_equal(got[:3 * K], np.concatenate([seen, correct, positive]).astype(np.int64))
    if CH > K:
        assert tuple(got[3 * K:]) == port.ignore_iou_counts(m.max(1)[1], tt, K, 255) and got[3 * K:].min() > 0
    else:
        assert not got[3 * K:].any()
    assert torch.isnan(m).any() and got[:K].sum() < t.size


def test_both_arg_maxes_follow_the_torch_rule():
    nan = np.float32(np.nan)
    # columns: a tie 1 / 2 below channel 3; a NaN in a class channel; a NaN in the last channel only; the last channel equal to the maximum
    m = np.array([[0, 1, 0, 2], [3, nan, 1, 2], [3, 5, 2, 0], [4, 9, nan, 2]], dtype=np.float32)[:, None, :]      # [CH=4, 1, 4]
    o_cls, o_all = R.argmaxes(m, 3)
    t = torch.from_numpy(m)
    assert np.array_equal(o_cls, t[:3].max(0)[1].numpy()) and np.array_equal(o_all, t.max(0)[1].numpy())
    assert o_cls[0].tolist() == [1, 1, 2, 0] and o_all[0].tolist() == [3, 1, 3, 0]


CASES = [(H, W, kind) for H, W in ((8, 32), (9, 33), (13, 17), (121, 161), (97, 129)) for kind in ('one', 'two', 'ten')] + [(97, 129, 'big')]


@pytest.mark.parametrize("H, W, kind", [c for c in CASES if c[0] < 100])
@pytest.mark.parametrize("CH, K", [(20, 19), (22, 21), (19, 19)])
def test_the_gpu_cases_exercise_both_arg_maxes(H, W, kind, CH, K):
    """The condition tests/test_ms_eval_gpu.py asserts before it compares, checked here on the restatement alone (the two larger
    sizes are checked there, where their restatement is computed anyway)."""
    sizes, flips = R.sources(kind, H, W)
    lq, t = R.make_case(H * 7 + W * 3 + CH, sizes, H, W, CH, K)
    cnt, o_cls, o_all, m = R.ms_iou_counts(lq, sizes, flips, (H, W), t, K, 255)
    assert R.exercised(m, o_cls, o_all, cnt, t, K) is None


@pytest.mark.parametrize("CH, K", CHK)
def test_the_cpu_op_equals_the_restated_counters(CH, K):
    from mulactseg_amd import ops
    H, W = 23, 31
    sizes, flips = R.sources('ten', H, W)
    lq, t = R.make_case(3 * CH + K, sizes, H, W, CH, K)
    zs = [torch.from_numpy(q)[None] for q in lq]
    tt = torch.from_numpy(t)[None]
    pred = torch.full((H, W), 0xAB, dtype=torch.uint8)
    got = ops.ms_iou_counts(zs, sizes, flips, (H, W), tt, K, 255, pred=pred)
    m = _aten_mean(lq, sizes, flips, H, W)[0].numpy()
    want = R.counts_from_mean(m, t, K, 255)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3 * K + 3,) and np.array_equal(got.numpy(), want)
    assert np.array_equal(pred.numpy(), R.argmaxes(m, K)[0])
    again = ops.ms_iou_counts(zs, sizes, flips, (H, W), tt[0], K, 255, counts=got)
    assert again is got and np.array_equal(got.numpy(), 2 * want)
    # away from near-ties the wholly restated chain (float32 taps, each operation rounded) counts the same pixels
    cnt, o_cls, _, mr = R.ms_iou_counts(lq, sizes, flips, (H, W), t, K, 255)
    assert (o_cls == R.argmaxes(m, K)[0]).mean() > 0.99 and np.allclose(mr, m, atol=1e-5, equal_nan=True)


def test_the_wrapper_rejects_bad_arguments_before_touching_a_device():
    from mulactseg_amd import ops
    z = torch.zeros(1, 20, 3, 4)
    t = torch.zeros(1, 10, 14, dtype=torch.int64)
    ok = ([z], [(12, 16)], [False], (10, 14))
    with pytest.raises(ValueError):
        ops.ms_iou_counts([], [], [], (10, 14), t, 19, 255)
    with pytest.raises(ValueError):
        ops.ms_iou_counts([z] * 17, [(12, 16)] * 17, [False] * 17, (10, 14), t, 19, 255)
    with pytest.raises(ValueError):
        ops.ms_iou_counts([z], [(16, 16)], [False], (10, 14), t, 19, 255)        # 16 x 16 emits 4 x 4, not 3 x 4
    with pytest.raises(ValueError):
        ops.ms_iou_counts(*ok, t, 21, 255)                                       # 20 channels: neither 21 nor 22
    with pytest.raises(ValueError):
        ops.ms_iou_counts(*ok, t, 18, 255)
    with pytest.raises(TypeError):
        ops.ms_iou_counts(*ok, t.int(), 19, 255)
    with pytest.raises(ValueError):
        ops.ms_iou_counts(*ok, t[:, :9], 19, 255)
    with pytest.raises(ValueError):
        ops.ms_iou_counts(*ok, t, 19, 255, counts=torch.zeros(3 * 20 + 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.ms_iou_counts(*ok, t, 19, 255, pred=torch.zeros(10, 14, dtype=torch.int64))
    assert not ops.ms_iou_supported(*ok)                                         # CPU tensors
    assert ops.ms_iou_counts(*ok, t, 19, 255).tolist()[:1] == [140]              # (and the valid call counts on the CPU)


def test_the_flags_parse_in_both_argument_sets():
    from mulactseg_amd.utils import common, common_voc
    for mod, classes, dataset in ((common, 19, 'cityscapes'), (common_voc, 21, 'voc')):
        a = mod.get_parser().parse_args(['--method', 'eval_naive_ms'])
        assert a.ms_factors == (0.5, 0.75, 1.0, 1.25, 1.5) and a.ms_noflip is False
        assert a.num_classes == classes and a.val_dataset == dataset
        a = mod.get_parser().parse_args(['--ms_factors', '1.0', '--ms_noflip'])
        assert a.ms_factors == (1.0,) and a.ms_noflip is True
        assert mod.get_parser().parse_args(['--ms_factors', '0.75, 2']).ms_factors == (0.75, 2.0)
        for bad in ('', 'x', '0', '1.0,-2'):
            with pytest.raises(SystemExit):
                mod.get_parser().parse_args(['--ms_factors', bad])


def test_the_trainer_module_subclasses_eval_naive():
    from mulactseg_amd.trainer import eval_naive, eval_naive_ms
    from mulactseg_amd.utils.miou import LogitsIoU, MultiScaleLogitsIoU
    assert issubclass(eval_naive_ms.ActiveTrainer, eval_naive.ActiveTrainer)
    assert eval_naive_ms.ActiveTrainer.predicts_ignore is True
    assert issubclass(MultiScaleLogitsIoU, LogitsIoU) and hasattr(MultiScaleLogitsIoU, 'step_ms')


class _HostStore:
    """``PictureStore`` without a device: the decoded files as CPU tensors."""

    def picture(self, path):
        from mulactseg_amd.dataloader.picture_store import decode_picture
        return torch.from_numpy(decode_picture(path))

    def labelmap(self, path):
        from mulactseg_amd.dataloader.picture_store import decode_map
        return torch.from_numpy(decode_map(path))


@pytest.mark.parametrize("name", ["cityscapes", "voc"])
def test_the_own_size_set_yields_the_copies_and_the_labels_at_the_picture_size(tmp_path, monkeypatch, name):
    """The set on a host store, with the augmentation kernel stood in for by its output shape (the pictures themselves are compared
    with Pillow in tests/test_ms_eval_gpu.py)."""
    from mulactseg_amd.dataloader import eval_ms
    from mulactseg_amd.dataloader.device_transforms import DeviceTrainAugment
    from mulactseg_amd.dataloader.utils import collate_fn
    calls = []

    def shape_only(self, img, maps=(), params=None):
        calls.append((params['th'], params['tw'], params['flip']))
        return torch.zeros((3,) + tuple(self.size)), []
    monkeypatch.setattr(DeviceTrainAugment, '__call__', shape_only)
    if name == 'cityscapes':
        tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=1, H=32, W=48, nseg=16, n_val=2)
        shapes = [(32, 48)] * 2
    else:
        tree = helpers.write_voc_tree(str(tmp_path / 'data'), n=2, sizes=((30, 44), (41, 27)))
        shapes = [(30, 44), (41, 27)]
    for factors, flip in (((0.5, 0.75, 1.0, 1.25, 1.5), True), ((1.0, 2.0), False), ((1.0,), False)):
        ds = eval_ms.get_ms_eval_dataset(name, tree['root'], tree['val_datalist'], factors=factors, flip=flip, store=_HostStore())
        assert len(ds) == 2 and ds.device_resident
        for i, (H, W) in enumerate(shapes):
            del calls[:]
            s = ds[i]
            want = [(int(f * H), int(f * W), fl) for fl in ((False, True) if flip else (False,)) for f in factors]
            assert calls == want and [tuple(x.shape) for x in s['image_list']] == [(3, th, tw) for th, tw, _ in want]
            assert s['labels'].dtype == torch.int64 and tuple(s['labels'].shape) == (H, W) and s['imsizes'] == (W, H)
            assert s['fnames'] == ds.im_idx[i]
            lab = s['labels'].numpy()
            if name == 'cityscapes':
                from PIL import Image
                raw = np.array(Image.open(s['fnames'][1]))
                lut = np.full(256, 255, dtype=np.int64)
                lut[helpers.CITY_TRAIN_IDS] = np.arange(19)
                assert np.array_equal(lab, lut[raw]) and (lab == 255).any() and lab[lab != 255].max() <= 18
            else:
                assert np.array_equal(lab, tree['classes'][i].astype(np.int64)) and (lab == 255).any()
            batch = collate_fn([s])
            assert len(batch['image_list'][0]) == len(want) and tuple(batch['labels'].shape) == (1, H, W)
    with pytest.raises(NotImplementedError):
        eval_ms.get_ms_eval_dataset('gta5', tree['root'], tree['val_datalist'])
    with pytest.raises(ValueError):
        eval_ms.get_ms_eval_dataset(name, tree['root'], tree['val_datalist'], factors=())


def test_the_entry_points_are_declared_bound_and_refuse_bad_arguments():
    from mulactseg_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "mulactseg_hip.h")) as f:
        text = f.read()
    assert "int mas_ms_iou_counts(" in text and "int64_t mas_ms_iou_lds_bytes(" in text and "#define MAS_ABI_VERSION 9" in text
    assert _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES["mas_ms_iou_counts"][1]) == 12 and len(_lib.SIGNATURES["mas_ms_iou_lds_bytes"][1]) == 4
    lib = _lib.load()
    assert hasattr(lib, "mas_ms_iou_counts") and hasattr(lib, "mas_ms_iou_lds_bytes")
    import ctypes
    fake = 256                                                   # never dereferenced: every call below fails its argument checks
    g = (ctypes.c_int32 * 5)(3, 4, 12, 16, 0)
    lp = (ctypes.c_void_p * 1)(fake)

    def call(geom=g, n=1, CH=20, H=10, W=14, K=19, logits=lp, tp=fake, cp=fake):
        return lib.mas_ms_iou_counts(logits, geom, n, CH, H, W, tp, K, 255, cp, None, None)
    assert call(logits=None) == -1 and call(geom=None) == -1 and call(tp=None) == -1 and call(cp=None) == -1
    assert call(logits=(ctypes.c_void_p * 1)(None)) == -1
    assert call(n=0) < 0 and call(n=17) < 0
    assert call(CH=21) == -3 and call(CH=18) == -3 and call(CH=34, K=33) == -3 and call(CH=1, K=0) == -3
    assert call(H=0) == -2 and call(geom=(ctypes.c_int32 * 5)(13, 4, 12, 16, 0)) == -2           # hq > hs
    # the sizing code: factor 2.0 at Cityscapes size fits, and the guard is where the bytes pass 64 KB
    H, W = 1024, 2048
    geom = lambda f: [ops.quarter_size(int(f * H)), ops.quarter_size(int(f * W)), int(f * H), int(f * W), 1]
    assert 0 < ops.ms_iou_lds_bytes(geom(2.0), (H, W)) <= ops.MS_MAX_LDS < ops.ms_iou_lds_bytes(geom(3.0), (H, W))
    big = (ctypes.c_int32 * 5)(*geom(3.0))
    assert call(geom=big, H=H, W=W) == lib.mas_ms_naive_plbl(lp, big, 1, 20, H, W, None, 0, 255, fake, None, None) < 0
    assert ops.ms_iou_lds_bytes([13, 4, 12, 16, 0], (10, 14)) == -2
