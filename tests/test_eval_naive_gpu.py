"""``eval_city_mul_res50.sh`` on the GPU: ``k_lowres_iou`` (csrc/lowres_iou.hip) against the fused counters on the materialised
upsampling and against the restatement; ``LowresLogitsIoU`` against ``LogitsIoU``; the ``eval_naive`` trainer end to end on a
Cityscapes-layout tree, on both paths; and the entries of ``RegionCityscapesAll`` against the restated loop."""
import logging
import os

import numpy as np
import pytest
import torch

import helpers
import lowres_iou_restated as L
import naive_plbl_restated as R
import region_all_restated as RA

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _case(seed, B, CH, h, w, H, W, C):
    """Logits with planted exact ties -- channels 2 and 4 equal and above the rest in one band, channel C equal to the class
    maximum in another -- and NaN logits in channel 0, a middle class channel and channel C; targets with 255 and values outside
    [0, C)."""
    rs = np.random.RandomState(seed)
    zq = (2.0 * rs.randn(B, CH, h, w)).astype(np.float32)
    b1, b2 = slice(0, h // 3), slice(h // 3, 2 * h // 3)
    zq[:, 2, b1] += 6.0
    zq[:, 4, b1] = zq[:, 2, b1]
    if CH > C:
        zq[:, 1, b2] += 6.0
        zq[:, C, b2] = zq[:, 1, b2]
    zq[0, 0, h - 2, w // 3] = np.nan
    zq[0, 5, h - 1, w // 2] = np.nan
    zq[-1, CH - 1, h // 2, w - 1] = np.nan
    t = rs.randint(0, C, size=(B, H, W)).astype(np.int64)
    t[rs.uniform(size=t.shape) < 0.1] = 255
    t[rs.uniform(size=t.shape) < 0.02] = C + 3
    t[rs.uniform(size=t.shape) < 0.01] = -1
    return zq, t


GEOMS = [(256, 512, 1024, 2048), (129, 129, 513, 513), (33, 65, 129, 257), (48, 80, 48, 80)]


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("C", [19, 21])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_kernel_equals_the_fused_counters_on_the_materialised_upsampling(geom, C, extra, B):
    ops = _gpu()
    h, w, H, W = geom
    CH = C + extra
    zq, t = _case(h + 3 * C + 7 * extra + 11 * B, B, CH, h, w, H, W, C)
    zt, tt = torch.from_numpy(zq).cuda(), torch.from_numpy(t).cuda()
    assert ops.lowres_iou_supported(zt, (H, W))
    got = ops.lowres_iou_counts(zt, tt, (H, W), C, 255)
    up = zt if (h, w) == (H, W) else ops.upsample_bilinear(zt, (H, W))
    want = ops.logits_iou_counts(up.contiguous(), tt, C, 255)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3 * C + 3,)
    assert torch.equal(got, want)
    assert torch.isnan(up).any()
    if extra:
        assert got[3 * C:].min() > 0
    else:
        assert not got[3 * C:].any()
    if B * H * W <= 600_000:                      # the numpy restatement (the large geometries take it in the accumulation test)
        assert np.array_equal(got.cpu().numpy(), L.lowres_iou_counts(zq, t, H, W, C, 255))
        assert np.array_equal(up.cpu().numpy(), R.upsample(zq, H, W), equal_nan=True)


def test_counts_accumulate_across_calls_and_equal_the_restatement_at_full_size():
    ops = _gpu()
    C, H, W = 19, 1024, 2048
    counts = None
    want = np.zeros(3 * C + 3, dtype=np.int64)
    for k in range(2):
        zq, t = _case(100 + k, 1, C + 1, 256, 512, H, W, C)
        counts = ops.lowres_iou_counts(torch.from_numpy(zq).cuda(), torch.from_numpy(t).cuda(), (H, W), C, 255, counts)
        want += L.lowres_iou_counts(zq, t, H, W, C, 255)
    assert np.array_equal(counts.cpu().numpy(), want)


def test_unsupported_geometries_and_shapes_are_refused():
    ops = _gpu()
    from mulactseg_amd import _lib
    z = torch.zeros((1, 20, 64, 64), device='cuda')
    t = torch.zeros((1, 32, 32), dtype=torch.int64, device='cuda')
    assert not ops.lowres_iou_supported(z, (32, 32))
    with pytest.raises(ValueError, match="cannot be upsampled"):
        ops.lowres_iou_counts(z, t, (32, 32), 19, 255)                        # a downsampling
    t7 = torch.zeros((1, 64, 7 * 64), dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError, match="cannot be upsampled"):
        ops.lowres_iou_counts(z, t7, (64, 7 * 64), 19, 255)                   # wider than x6
    with pytest.raises(ValueError, match="do not match"):
        ops.lowres_iou_counts(z, t, (128, 128), 19, 255)
    with pytest.raises(_lib.MulActSegHipError):
        ops.lowres_iou_counts(z, torch.zeros((1, 128, 128), dtype=torch.int64, device='cuda'), (128, 128), 17, 255)   # 20 != C, C + 1


def test_lowres_meter_equals_the_logits_meter_on_the_materialised_logits():
    ops = _gpu()
    from mulactseg_amd.utils.miou import LogitsIoU, LowresLogitsIoU
    C = 19
    lo, full = LowresLogitsIoU(C, 255), LogitsIoU(C, 255)
    lo._before_epoch(), full._before_epoch()
    for k in range(3):
        zq, t = _case(200 + k, 2, C + 1, 64, 128, 256, 512, C)
        t[t < 0] = 255
        t[t >= C] = 255
        zt, tt = torch.from_numpy(zq).cuda(), torch.from_numpy(t).cuda()
        lo.step_lowres(zt, tt)
        full.step(ops.upsample_bilinear(zt, (256, 512)), tt)
    assert torch.equal(lo._counts, full._counts)
    assert lo.ious() == full.ious() and lo.ignore_iou() == full.ignore_iou()
    assert 0 < lo.ignore_iou() < 100 and len(lo.ious()) == C


# -- the trainer end to end (script/open_source/eval_city_mul_res50.sh) ----------------------------------------------------------
def _eval_args(tree, run, ckpt):
    a = helpers.cityscapes_tree_args(tree, run, ['--init_checkpoint', ckpt, '--stage2', '--method', 'eval_naive', '--loader',
                                                 'region_cityscapes_all', '--train_transform', 'eval_spx', '--val_batch_size', '1'])
    a.or_labeling = False
    a.val_batch_size = 1
    return a


def _seeded_checkpoint(a, ckpt):
    from mulactseg_amd.models import get_model
    torch.manual_seed(0)
    net = get_model(model=a.model, num_classes=a.num_classes + 1, output_stride=a.output_stride, separable_conv=a.separable_conv,
                    pretrained_backbone=False)
    os.makedirs(os.path.dirname(ckpt), exist_ok=True)
    torch.save({'model_state_dict': net.state_dict()}, ckpt)


def _run_eval(a, ckpt):
    from mulactseg_amd import dataloader
    from mulactseg_amd.trainer import eval_naive
    dataloader.register_dataset_factory(None)
    active_set = dataloader.get_active_dataset(a, train_transform=a.train_transform)
    trainer = eval_naive.ActiveTrainer(a, logging.getLogger("test"), 0)
    trainer.load_checkpoint(ckpt)
    return trainer, trainer.eval(active_set, selection_iter=0)


def test_eval_naive_end_to_end_on_both_paths(tmp_path, monkeypatch, capsys):
    _gpu()
    from mulactseg_amd import dataloader, ops
    from mulactseg_amd.utils.miou import LogitsIoU
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=2, H=128, W=256, nseg=64)
    run = tmp_path / 'run'
    ckpt = str(run / 'stage2_checkpoint01.tar')
    a = _eval_args(tree, run, ckpt)
    _seeded_checkpoint(a, ckpt)
    calls = []
    real = ops.lowres_iou_counts
    monkeypatch.setattr(ops, 'lowres_iou_counts', lambda *args, **kw: calls.append(args[2]) or real(*args, **kw))
    monkeypatch.delenv("MAS_EVAL_NAIVE", raising=False)
    trainer, table = _run_eval(a, ckpt)
    out = capsys.readouterr().out
    assert out.count("[AL 0-round]: evaluation") == 1 and table in out
    cells = table.split(',')
    assert len(cells) == 1 + 19 + 1 and all(c == '%.2f' % float(c) for c in cells)
    assert len(calls) == 2 and all(tuple(s) == (1024, 2048) for s in calls)        # the two val pictures on the low-res path
    # the full-resolution path on the same checkpoint and data
    monkeypatch.setenv("MAS_EVAL_NAIVE", "full")
    _, table_full = _run_eval(a, ckpt)
    assert len(calls) == 2 and table_full == table
    # the table straight from LogitsIoU over net(images) on the val set
    ds = dataloader.get_dataset(a, name=a.val_dataset, data_root=a.val_data_dir, datalist=a.val_datalist, imageset='eval')
    loader = trainer.get_valloader(ds)
    meter = LogitsIoU(19, 255)
    trainer.net.eval()
    with torch.no_grad():
        for _ in range(len(loader)):
            batch = next(loader)
            meter.step(trainer.net(batch['images'].cuda().float()), batch['labels'].cuda().long())
    ious = meter.ious()
    want = ','.join(['%.2f' % np.mean(ious)] + ['%.2f' % v for v in ious] + ['%.2f' % meter.ignore_iou()])
    assert table == want


def test_region_cityscapes_all_equals_the_restated_loop(tmp_path):
    _gpu()
    from PIL import Image
    from mulactseg_amd.dataloader import region_cityscapes_all
    from mulactseg_amd.dataloader.formats import open_spx
    from mulactseg_amd.dataloader.transform import get_train_transform
    H, W, NSEG = 128, 256, 64
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=3, H=H, W=W, nseg=NSEG)
    root = tree['root']
    plain = os.path.join(root, 'lists', 'train_seed%d.txt' % NSEG)
    with open(plain, 'w') as f:
        f.write('\n'.join('\t'.join([l.split('\t')[0], 'gtFine/train/%s/%s_gtFine_labelIds.png' % (s.split('_')[0], s), l.split('\t')[2]])
                          for l, s in zip(tree['lines'], tree['stems'])) + '\n')
    a = _eval_args(tree, tmp_path / 'run', str(tmp_path / 'run' / 'x.tar'))
    ds = region_cityscapes_all.RegionCityscapesAll(a, root, plain, transform=get_train_transform(a, 'eval_spx'),
                                                   region_dict=tree['region_dict'])
    assert len(ds) == 3
    Hr, Wr = 1024, 2048
    near = lambda arr: np.asarray(Image.fromarray(arr.astype(np.int32)).resize((Wr, Hr), Image.NEAREST)).astype(np.int64)
    flags = set()
    for i in range(len(ds)):
        item = ds[i]
        img_f, lbl_f, spx_f = item['fname']
        assert item['fname'] == ds.im_idx[i]
        target = near(ds.encode_target(np.array(Image.open(lbl_f))))
        spx = near(open_spx(spx_f))
        ids = ds.suppix[spx_f]
        want = RA.superpixel_info(target, spx, ids)
        got = item['superpixel_info']
        assert list(got) == list(ids) and got == want
        flags |= {(v['isignore'], v['allignore'], bool(v['cls'])) for v in got.values()}
    assert (True, False, True) in flags
