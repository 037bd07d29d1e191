"""Multi-scale + flip evaluation on the GPU: the evaluation mode of ``k_ms_naive`` (``ops.ms_iou_counts``, csrc/ms_naive.hip) counter for
counter against the numpy restatement (tests/ms_eval_restated.py), against ``LogitsIoU`` on the materialised ``ops.ms_ensemble`` logits
and against ``ops.lowres_iou_counts``; its argument checks and the LDS guard; the own-size evaluation set against Pillow; and
``--method eval_naive_ms`` end to end with the Cityscapes and the VOC argument sets, on the fused path and under ``MAS_MS_EVAL=aten``.
Counters are integers: every comparison is exact."""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

import helpers
import ms_ensemble_restated as E
import ms_eval_restated as R

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _run(ops, lq, sizes, flips, out_size, t, K, with_pred=True, counts=None):
    zs = [torch.from_numpy(q)[None].cuda() for q in lq]
    pred = torch.full(tuple(out_size), 0xAB, dtype=torch.uint8, device='cuda') if with_pred else None
    counts = ops.ms_iou_counts(zs, sizes, flips, out_size, torch.from_numpy(t)[None].cuda(), K, 255, counts=counts, pred=pred)
    torch.cuda.synchronize()
    return counts, pred


CASES = [(H, W, kind) for H, W in ((8, 32), (9, 33), (13, 17), (121, 161), (97, 129)) for kind in ('one', 'two', 'ten')] + [(97, 129, 'big')]


@pytest.mark.parametrize("H, W, kind", CASES)
@pytest.mark.parametrize("CH, K", [(20, 19), (22, 21), (19, 19)])
def test_counters_and_pred_equal_the_restatement(H, W, kind, CH, K):
    ops = _gpu()
    sizes, flips = R.sources(kind, H, W)
    lq, t = R.make_case(H * 7 + W * 3 + CH, sizes, H, W, CH, K)
    want, o_cls, o_all, m = R.ms_iou_counts(lq, sizes, flips, (H, W), t, K, 255)
    assert R.exercised(m, o_cls, o_all, want, t, K) is None                   # the case reaches both arg-maxes, ties, NaN, 255
    assert ops.ms_iou_supported([torch.from_numpy(q)[None].cuda() for q in lq], sizes, flips, (H, W))
    got, pred = _run(ops, lq, sizes, flips, (H, W), t, K)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3 * K + 3,)
    assert np.array_equal(pred.cpu().numpy(), o_cls.astype(np.uint8)), int((pred.cpu().numpy() != o_cls).sum())
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy() - want).tolist()


def _plain_case(seed, sizes, H, W, CH, K):
    """The inputs of the cases above without the NaNs (``k_logits_iou`` and ``k_lowres_iou`` never let a NaN win)."""
    lq, t = R.make_case(seed, sizes, H, W, CH, K)
    return [np.nan_to_num(q, nan=0.25) for q in lq], t


@pytest.mark.parametrize("H, W, CH, K", [(121, 161, 20, 19), (97, 129, 22, 21), (375, 500, 21, 21)])
def test_counters_equal_the_logits_meter_on_the_materialised_ensemble(H, W, CH, K):
    ops = _gpu()
    from mulactseg_amd.utils.miou import LogitsIoU, MultiScaleLogitsIoU
    sizes, flips = E.tta_sizes(H, W)
    lq, t = _plain_case(H + W, sizes, H, W, CH, K)
    zs = [torch.from_numpy(q)[None].cuda() for q in lq]
    tt = torch.from_numpy(t)[None].cuda()
    dummy = [torch.ones((1, 1) + tuple(z.shape[2:]), device='cuda') for z in zs]      # (one feature channel: the ensemble wants one)
    _, m = ops.ms_ensemble(dummy, zs, sizes, flips, (H, W))
    full, ms = LogitsIoU(K, 255), MultiScaleLogitsIoU(K, 255)
    full._before_epoch(), ms._before_epoch()
    for _ in range(2):
        full.step(m, tt)
        ms.step_ms(zs, sizes, flips, tt)
    assert torch.equal(ms._counts, full._counts) and int(ms._counts.sum()) > 0
    assert ms.ious() == full.ious() and ms.ignore_iou() == full.ignore_iou() and len(ms.ious()) == K
    assert (0 < ms.ignore_iou() < 100) == (CH > K)
    pred = torch.empty((H, W), dtype=torch.uint8, device='cuda')
    ops.ms_iou_counts(zs, sizes, flips, (H, W), tt, K, 255, pred=pred)
    assert torch.equal(pred.long(), m[0, :K].max(0)[1])


@pytest.mark.parametrize("H, W, CH, K", [(129, 161, 20, 19), (375, 500, 22, 21), (64, 96, 19, 19)])
def test_one_source_at_the_identity_geometry_equals_the_lowres_counters(H, W, CH, K):
    ops = _gpu()
    lq, t = _plain_case(H, [(H, W)], H, W, CH, K)
    zq = torch.from_numpy(lq[0])[None].cuda()
    tt = torch.from_numpy(t)[None].cuda()
    got = ops.ms_iou_counts([zq], [(H, W)], [False], (H, W), tt, K, 255)
    assert torch.equal(got, ops.lowres_iou_counts(zq, tt, (H, W), K, 255))
    assert torch.equal(got, ops.logits_iou_counts(ops.upsample_bilinear(zq, (H, W)), tt, K, 255))


def test_counters_accumulate_and_a_null_pred_writes_counters_only():
    ops = _gpu()
    H, W, CH, K = 121, 161, 20, 19
    sizes, flips = E.tta_sizes(H, W)
    lq, t = R.make_case(5, sizes, H, W, CH, K)
    want = R.ms_iou_counts(lq, sizes, flips, (H, W), t, K, 255)[0]
    once, pred = _run(ops, lq, sizes, flips, (H, W), t, K)
    twice, _ = _run(ops, lq, sizes, flips, (H, W), t, K, with_pred=False, counts=once.clone())
    alone, none = _run(ops, lq, sizes, flips, (H, W), t, K, with_pred=False)
    assert none is None and np.array_equal(once.cpu().numpy(), want)
    assert torch.equal(alone, once) and torch.equal(twice, 2 * once) and not (pred == 0xAB).all()


def test_bad_arguments_are_refused_and_nothing_is_written():
    _gpu()
    from mulactseg_amd import _lib
    lib = _lib.load()
    z = torch.zeros(20, 3, 4, device='cuda')
    t = torch.zeros(10, 14, dtype=torch.int64, device='cuda')
    pred = torch.full((10, 14), 0xAB, dtype=torch.uint8, device='cuda')
    counts = torch.full((60,), 7, dtype=torch.int64, device='cuda')
    lp = (ctypes.c_void_p * 17)(*([z.data_ptr()] * 17))
    ok = [3, 4, 12, 16, 0]

    def call(geom, n=1, CH=20, H=10, W=14, K=19, tp=t.data_ptr(), cp=counts.data_ptr(), logits=lp, pp=pred.data_ptr()):
        g = (ctypes.c_int32 * len(geom))(*geom) if geom is not None else None
        return lib.mas_ms_iou_counts(logits, g, n, CH, H, W, tp, K, 255, cp, pp, None)
    codes = [call(ok, n=0), call(ok * 17, n=17), call(ok, CH=21), call(ok, CH=18), call(ok, CH=34, K=33), call(ok, K=0, CH=1),
             call([13, 4, 12, 16, 0]), call([3, 17, 12, 16, 0]), call([0, 4, 12, 16, 0]), call([3, 4, 0, 16, 0]),
             call(ok, tp=None), call(ok, cp=None), call(None), call(ok, logits=None), call(ok, logits=(ctypes.c_void_p * 1)(None)),
             call(ok, H=0), call(ok, W=0)]
    torch.cuda.synchronize()
    assert all(c < 0 for c in codes), codes
    assert (pred == 0xAB).all() and (counts == 7).all()
    assert call(ok) == 0 and call(ok, pp=None) == 0
    torch.cuda.synchronize()
    assert (pred == 0).all() and counts[0] == 7 + 2 * 140 and counts[19] == 7 + 2 * 140 and counts[2 * 19] == 7 + 2 * 140
    assert (counts[1:19] == 7).all() and counts[57:].tolist() == [7, 7, 7]                     # 20 channels of zeros: o_all = o_cls = 0


def test_supported_agrees_with_the_entry_point_on_both_sides_of_the_lds_guard():
    ops = _gpu()
    from mulactseg_amd import _lib
    H, W, CH, K = 40, 72, 20, 19

    def geom(f):
        Hs, Ws = int(f * H), int(f * W)
        return [E.quarter_size(Hs), E.quarter_size(Ws), Hs, Ws, 1]
    # the first stage-2 downsample, in steps of a quarter, whose tile no longer fits: from the sizing code
    f = 2.0
    assert 0 < ops.ms_iou_lds_bytes(geom(f), (H, W)) <= ops.MS_MAX_LDS
    while ops.ms_iou_lds_bytes(geom(f + 0.25), (H, W)) <= ops.MS_MAX_LDS:
        f += 0.25
    assert f < 8
    for factor, fits in ((f, True), (f + 0.25, False)):
        sizes, flips = [(H, W), tuple(geom(factor)[2:4])], [False, True]
        lq, t = R.make_case(11, sizes, H, W, CH, K)
        zs = [torch.from_numpy(q)[None].cuda() for q in lq]
        tt = torch.from_numpy(t).cuda()
        counts = torch.full((3 * K + 3,), 7, dtype=torch.int64, device='cuda')
        assert ops.ms_iou_supported(zs, sizes, flips, (H, W)) == fits
        g = (ctypes.c_int32 * 10)(*(geom(1.0)[:4] + [0] + geom(factor)))
        lp = (ctypes.c_void_p * 2)(*[z.data_ptr() for z in zs])
        status = _lib.load().mas_ms_iou_counts(lp, g, 2, CH, H, W, tt.data_ptr(), K, 255, counts.data_ptr(), None, None)
        torch.cuda.synchronize()
        assert (status == 0) == fits
        if fits:
            want = R.ms_iou_counts(lq, sizes, flips, (H, W), t, K, 255)[0]
            assert np.array_equal(counts.cpu().numpy() - 7, want)
        else:
            assert status < 0 and (counts == 7).all()
            with pytest.raises(ValueError, match="LDS"):
                ops.ms_iou_counts(zs, sizes, flips, (H, W), tt, K, 255)


# -- the evaluation set and the trainer end to end ----------------------------------------------------------------------------------
def test_the_own_size_set_yields_pillow_copies_and_unresized_labels(tmp_path):
    _gpu()
    from PIL import Image
    from mulactseg_amd.dataloader.eval_ms import get_ms_eval_dataset
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=2, sizes=((61, 83), (70, 45)))
    factors = (0.5, 1.0, 1.75)
    ds = get_ms_eval_dataset('voc', tree['root'], tree['val_datalist'], factors=factors, flip=True)
    half = get_ms_eval_dataset('voc', tree['root'], tree['val_datalist'], factors=factors, flip=False)
    mean, std = np.asarray(MEAN, np.float32)[:, None, None], np.asarray(STD, np.float32)[:, None, None]
    for i, name in enumerate(tree['names'][:2]):
        s, h = ds[i], half[i]
        pic = Image.open(os.path.join(tree['root'], 'VOC2012/JPEGImages', name + '.jpg')).convert('RGB')
        W, H = pic.size
        assert len(s['image_list']) == 6 and len(h['image_list']) == 3 and s['imsizes'] == (W, H)
        for k, (fl, f) in enumerate([(fl, f) for fl in (False, True) for f in factors]):
            r = pic.resize((int(f * W), int(f * H)), Image.BILINEAR)
            want = np.asarray(r.transpose(Image.FLIP_LEFT_RIGHT) if fl else r).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
            assert np.array_equal(s['image_list'][k].cpu().numpy(), ((want - mean) / std).astype(np.float32))
            if not fl:
                assert torch.equal(h['image_list'][k], s['image_list'][k])
        assert np.array_equal(s['labels'].cpu().numpy(), tree['classes'][i].astype(np.int64)) and s['labels'].dtype == torch.int64


def _seeded_checkpoint(a, ckpt):
    from mulactseg_amd.models import get_model
    torch.manual_seed(0)
    net = get_model(model=a.model, num_classes=a.num_classes + 1, output_stride=a.output_stride, separable_conv=a.separable_conv,
                    pretrained_backbone=False)
    os.makedirs(os.path.dirname(ckpt), exist_ok=True)
    torch.save({'model_state_dict': net.state_dict()}, ckpt)


def _run_eval(a, ckpt, method):
    import importlib
    from mulactseg_amd import dataloader
    dataloader.register_dataset_factory(None)
    a.method = method
    trainer = importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer(a, logging.getLogger("test"), 0)
    trainer.load_checkpoint(ckpt)
    return trainer, trainer.eval(None, selection_iter=0)


def _city_args(tree, run, ckpt, extra=()):
    a = helpers.cityscapes_tree_args(tree, run, ['--init_checkpoint', ckpt, '--stage2', '--method', 'eval_naive_ms', '--loader',
                                                 'region_cityscapes_all', '--train_transform', 'eval_spx', '--val_batch_size', '1']
                                     + list(extra))
    a.or_labeling = False
    return a


def _own_size_table(trainer, ds, K):
    """The table of ``LogitsIoU`` over ``net(picture)`` on the pictures of ``ds`` at their own sizes, one scale, no flip."""
    from mulactseg_amd.utils.miou import LogitsIoU
    meter = LogitsIoU(K, 255)
    trainer.net.eval()
    with torch.no_grad():
        for i in range(len(ds)):
            s = ds[i]
            meter.step(trainer.net(s['image_list'][0][None].float()), s['labels'][None])
    ious = meter.ious()
    return ','.join(['%.2f' % np.mean(ious)] + ['%.2f' % v for v in ious] + ['%.2f' % meter.ignore_iou()])


def test_eval_naive_ms_on_a_cityscapes_tree_on_both_paths(tmp_path, monkeypatch, capsys):
    """The tree of 128 x 256 pictures with two evaluation pictures.  The factors (1.0, 1.5, 2.0) and their flips keep every plane of
    the network >= 8 x 8 (smaller planes run on MIOpen kernels that are not run-to-run identical, and the comparisons below need one
    forward to equal the next) and reach the 2.0 the kernel must accept."""
    ops = _gpu()
    from mulactseg_amd.dataloader.eval_ms import get_ms_eval_dataset
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=1, H=128, W=256, nseg=64, n_val=2)
    run = tmp_path / 'run'
    ckpt = str(run / 'stage2_checkpoint01.tar')
    a = _city_args(tree, run, ckpt, ['--ms_factors', '1.0,1.5,2.0'])
    _seeded_checkpoint(a, ckpt)
    calls = []
    real = ops.ms_iou_counts
    monkeypatch.setattr(ops, 'ms_iou_counts', lambda *args, **kw: calls.append((len(args[0]), list(args[2]), tuple(args[3]))) or real(*args, **kw))
    monkeypatch.delenv("MAS_MS_EVAL", raising=False)
    trainer, table = _run_eval(a, ckpt, 'eval_naive_ms')
    out = capsys.readouterr().out
    assert out.count("[AL 0-round]: evaluation") == 1 and table in out
    cells = table.split(',')
    assert len(cells) == 1 + 19 + 1 and all(c == '%.2f' % float(c) for c in cells)
    assert calls == [(6, [False] * 3 + [True] * 3, (128, 256))] * 2                  # the two pictures, each one fused launch
    monkeypatch.setenv("MAS_MS_EVAL", "aten")
    _, table_aten = _run_eval(a, ckpt, 'eval_naive_ms')
    monkeypatch.delenv("MAS_MS_EVAL")
    print("cityscapes tree, fused: %s\ncityscapes tree, aten:  %s" % (table, table_aten))
    assert table_aten == table
    # a model without quarter-resolution logits: full-resolution forwards, the average in ATen, LogitsIoU
    monkeypatch.setattr(type(trainer.net), 'lowres_logits', False)
    del calls[:]
    _, table_full = _run_eval(a, ckpt, 'eval_naive_ms')
    monkeypatch.setattr(type(trainer.net), 'lowres_logits', True)
    print("cityscapes tree, full:  %s" % table_full)
    assert not calls and table_full == table
    # one scale, no flip: the plain evaluation of whole pictures at their own size
    a1 = _city_args(tree, run, ckpt, ['--ms_factors', '1.0', '--ms_noflip'])
    _, table_one = _run_eval(a1, ckpt, 'eval_naive_ms')
    ds = get_ms_eval_dataset('cityscapes', a1.val_data_dir, a1.val_datalist, factors=(1.0,), flip=False)
    assert table_one == _own_size_table(trainer, ds, 19)


def test_one_scale_without_flip_prints_the_table_of_eval_naive_at_native_size(tmp_path, monkeypatch, capsys):
    """``eval_naive`` resizes every Cityscapes picture to 1024 x 2048 and ``eval_naive_ms`` keeps its own size, so the two tables can
    only agree where that resize is the identity: on pictures of the native size, which is what the real evaluation list holds.
    (On the 128 x 256 tree of the test above ``eval_naive`` evaluates 8x enlarged pictures; there the one-scale table is compared with
    ``LogitsIoU`` over the own-size forwards instead.)"""
    _gpu()
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=1, H=1024, W=2048, nseg=64, n_val=2)
    run = tmp_path / 'run'
    ckpt = str(run / 'stage2_checkpoint01.tar')
    a = _city_args(tree, run, ckpt, ['--ms_factors', '1.0', '--ms_noflip'])
    _seeded_checkpoint(a, ckpt)
    monkeypatch.delenv("MAS_MS_EVAL", raising=False)
    monkeypatch.delenv("MAS_EVAL_NAIVE", raising=False)
    _, table_ms = _run_eval(a, ckpt, 'eval_naive_ms')
    _, table_naive = _run_eval(a, ckpt, 'eval_naive')
    out = capsys.readouterr().out
    print("eval_naive_ms 1.0 noflip: %s\neval_naive:               %s" % (table_ms, table_naive))
    assert out.count("[AL 0-round]: evaluation") == 2 and table_ms == table_naive and len(table_ms.split(',')) == 21


def _voc_args(tree, run, extra):
    from mulactseg_amd.utils.common_voc import get_parser
    base = ['-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--nseg', str(tree['nseg']), '--trg_data_dir', tree['root'],
            '--trg_datalist', tree['trg_datalist'], '--region_dict', tree['region_dict'], '--val_data_dir', tree['root'],
            '--val_datalist', tree['val_datalist'], '--num_workers', '0', '--val_num_workers', '0', '--stage2', '--method', 'eval_naive_ms',
            '-p', str(run)]
    a = get_parser().parse_args(base + list(extra))
    a.pretrained_backbone = False
    return a


def test_eval_naive_ms_on_a_voc_tree_on_both_paths(tmp_path, monkeypatch, capsys):
    """The VOC argument set (21 classes, a 22-channel model, ``--val_dataset voc``) with the default ten copies on pictures of different
    sizes, each large enough for its half-size copy to keep the network's planes >= 8 x 8."""
    ops = _gpu()
    from mulactseg_amd.dataloader.eval_ms import get_ms_eval_dataset
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=2, sizes=((261, 341), (303, 265)))
    run = tmp_path / 'run'
    ckpt = str(run / 'stage2_checkpoint01.tar')
    a = _voc_args(tree, run, ['--init_checkpoint', ckpt])
    assert a.num_classes == 21 and a.val_dataset == 'voc' and len(a.ms_factors) == 5 and a.val_batch_size == 12
    _seeded_checkpoint(a, ckpt)
    calls = []
    real = ops.ms_iou_counts
    monkeypatch.setattr(ops, 'ms_iou_counts', lambda *args, **kw: calls.append((len(args[0]), tuple(args[3]))) or real(*args, **kw))
    monkeypatch.delenv("MAS_MS_EVAL", raising=False)
    trainer, table = _run_eval(a, ckpt, 'eval_naive_ms')
    out = capsys.readouterr().out
    assert out.count("[AL 0-round]: evaluation") == 1 and table in out and len(table.split(',')) == 1 + 21 + 1
    assert calls == [(10, (261, 341)), (10, (303, 265))]
    monkeypatch.setenv("MAS_MS_EVAL", "aten")
    _, table_aten = _run_eval(a, ckpt, 'eval_naive_ms')
    monkeypatch.delenv("MAS_MS_EVAL")
    print("voc tree, fused: %s\nvoc tree, aten:  %s" % (table, table_aten))
    assert table_aten == table
    a1 = _voc_args(tree, run, ['--init_checkpoint', ckpt, '--ms_factors', '1.0', '--ms_noflip'])
    _, table_one = _run_eval(a1, ckpt, 'eval_naive_ms')
    ds = get_ms_eval_dataset('voc', a1.val_data_dir, a1.val_datalist, factors=(1.0,), flip=False)
    assert table_one == _own_size_table(trainer, ds, 21)
