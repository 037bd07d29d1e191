"""The naive arg-max pseudo labels of VOC on the GPU: the fused kernel (``ops.ms_naive_labels``, csrc/ms_naive.hip) bit for bit against the
numpy restatement (tests/ms_naive_restated.py), against ``ops.ms_ensemble`` + arg-max + ``MeanIoU`` and ``ops.naive_pseudo_labels``,
its argument checks, the fused path against ``MAS_MS_NAIVE=aten`` on a seeded network, and both generators end to end from the files
to a stage-2 training sample."""
import ctypes
import logging
import os
import random

import numpy as np
import pytest
import torch

import helpers
import ms_ensemble_restated as E
import ms_naive_restated as R
import render_restated as RR

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ODD_SIZES = ((121, 161), (153, 111), (97, 129))


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _logits(rs, sizes, C):
    return [rs.uniform(-1, 1, (C, E.quarter_size(Hs), E.quarter_size(Ws))).astype(np.float32) for Hs, Ws in sizes]


def _targets(rs, H, W, K):
    t = rs.randint(0, K, size=(H, W)).astype(np.int64)
    t[rs.uniform(size=t.shape) < 0.05] = 255
    return t


def _run(ops, lq, sizes, flips, out_size, t=None, K=None):
    zs = [torch.from_numpy(q)[None].cuda() for q in lq]
    counts = None
    if t is not None:
        counts = torch.zeros(3 * K + 3, dtype=torch.int64, device='cuda')
        t = torch.from_numpy(t)[None].cuda()
    lab = ops.ms_naive_labels(zs, sizes, flips, out_size, targets=t, counts=counts, num_classes=K)
    torch.cuda.synchronize()
    return lab[0].cpu().numpy(), None if counts is None else counts.cpu().numpy()


CASES = [  # (H, W, C, K, which sources of the TTA list)
    (375, 500, 21, 22, range(10)), (500, 375, 21, 22, range(10)), (121, 161, 21, 22, range(10)), (153, 111, 21, 22, range(10)),
    (97, 129, 13, 16, range(10)), (131, 130, 21, 22, [3, 8]), (120, 160, 21, 22, [2]), (375, 500, 40, None, range(10)),
    (333, 500, 7, 8, [0, 9]),
]


@pytest.mark.parametrize("H, W, C, K, which", CASES)
def test_labels_and_counters_are_bit_exact_to_the_restatement(H, W, C, K, which):
    ops = _gpu()
    rs = np.random.RandomState(H * 7 + W * 3 + C)
    sizes, flips = E.tta_sizes(H, W)
    sizes, flips = [sizes[i] for i in which], [flips[i] for i in which]
    lq = _logits(rs, sizes, C)
    t = None if K is None else _targets(rs, H, W, K)
    lab, cnt = _run(ops, lq, sizes, flips, (H, W), t, K)
    want = R.labels(lq, sizes, flips, (H, W))
    assert lab.dtype == np.int64 and np.array_equal(lab, want), int((lab != want).sum())
    if K is not None:
        assert np.array_equal(cnt, R.counts(want, t, K, 255)) and np.array_equal(cnt, R.meaniou_loop(want, t, K, 255))


@pytest.mark.parametrize("H, W", [(375, 500), (121, 161), (96, 128)])
def test_labels_are_the_arg_max_of_the_ensemble_and_counters_those_of_meaniou(H, W):
    ops = _gpu()
    from mulactseg_amd.utils.miou import MeanIoU
    rs = np.random.RandomState(H + W)
    sizes, flips = E.tta_sizes(H, W)
    zs = [torch.from_numpy(q)[None].cuda() for q in _logits(rs, sizes, 21)]
    dummy = [torch.ones((1, 1) + tuple(z.shape[2:]), device='cuda') for z in zs]      # (one feature channel: the ensemble wants one)
    t = torch.from_numpy(np.where(rs.uniform(size=(H, W)) < 0.2, 21, rs.randint(0, 21, size=(H, W))))[None].cuda()
    meter = MeanIoU(22, 255)
    meter._before_epoch()
    counts = meter._ensure(t.device)
    lab = ops.ms_naive_labels(zs, sizes, flips, (H, W), targets=t, counts=counts, num_classes=22)
    _, z = ops.ms_ensemble(dummy, zs, sizes, flips, (H, W))
    want = torch.max(z, 1)[1]
    assert torch.equal(lab, want)
    ref = MeanIoU(22, 255)
    ref._before_epoch()
    ref._after_step({'outputs': want, 'targets': t})
    assert torch.equal(counts, ref._counts) and int(counts[21]) > 0 and int(counts[2 * 22 + 21]) == 0


@pytest.mark.parametrize("h, w, H, W", [(94, 125, 375, 500), (33, 41, 129, 161), (32, 32, 128, 128)])
def test_one_source_at_the_identity_geometry_is_the_naive_labeller(h, w, H, W):
    ops = _gpu()
    rs = np.random.RandomState(h)
    zq = torch.from_numpy(rs.randn(1, 21, h, w).astype(np.float32)).cuda()
    # (hq, wq, H, W, 0): stage 1 to the picture itself, stage 2 the identity
    lq = [zq[0].cpu().numpy()]
    from mulactseg_amd import _lib
    lab = torch.empty((1, H, W), dtype=torch.uint8, device='cuda')
    g = (ctypes.c_int32 * 5)(h, w, H, W, 0)
    lp = (ctypes.c_void_p * 1)(zq.data_ptr())
    _lib.check(_lib.load().mas_ms_naive_plbl(lp, g, 1, 21, H, W, None, 0, 255, lab.data_ptr(), None, None), "mas_ms_naive_plbl")
    want = ops.naive_pseudo_labels(zq, (H, W), torch.ones((1, H, W), dtype=torch.bool, device='cuda'))
    assert torch.equal(lab.long(), want)
    assert torch.equal(want, torch.max(ops.upsample_bilinear(zq, (H, W)), 1)[1])
    assert np.array_equal(want[0].cpu().numpy(), np.argmax(E.resize(lq[0], H, W), axis=0))


def test_counters_accumulate_and_a_null_counts_pointer_gives_labels_only():
    ops = _gpu()
    rs = np.random.RandomState(9)
    H, W = 121, 161
    sizes, flips = E.tta_sizes(H, W)
    zs = [torch.from_numpy(q)[None].cuda() for q in _logits(rs, sizes, 21)]
    t = torch.from_numpy(_targets(rs, H, W, 22))[None].cuda()
    counts = torch.zeros(69, dtype=torch.int64, device='cuda')
    a = ops.ms_naive_labels(zs, sizes, flips, (H, W), targets=t, counts=counts, num_classes=22)
    once = counts.clone()
    b = ops.ms_naive_labels(zs, sizes, flips, (H, W), targets=t, counts=counts, num_classes=22)
    c = ops.ms_naive_labels(zs, sizes, flips, (H, W))
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(counts, 2 * once) and int(once.sum()) > 0
    assert np.array_equal(once.cpu().numpy(), R.counts(a[0].cpu().numpy(), t[0].cpu().numpy(), 22, 255))


def test_bad_arguments_are_refused_and_nothing_is_written():
    _gpu()
    from mulactseg_amd import _lib
    lib = _lib.load()
    z = torch.zeros(21, 3, 4, device='cuda')
    big = torch.zeros(21, 100, 100, device='cuda')
    t = torch.zeros(10, 14, dtype=torch.int64, device='cuda')
    lab = torch.full((10, 14), 0xAB, dtype=torch.uint8, device='cuda')
    counts = torch.full((69,), 7, dtype=torch.int64, device='cuda')
    lp = (ctypes.c_void_p * 17)(*([z.data_ptr()] * 17))
    ok = [3, 4, 12, 16, 0]

    def call(geom, n=1, C=21, H=10, W=14, K=22, tp=t.data_ptr(), cp=counts.data_ptr(), logits=lp):
        g = (ctypes.c_int32 * len(geom))(*geom)
        return lib.mas_ms_naive_plbl(logits, g, n, C, H, W, tp, K, 255, lab.data_ptr(), cp, None)
    codes = [call(ok, n=0), call(ok * 17, n=17), call(ok, C=256), call(ok, C=0), call(ok, K=33), call(ok, K=20),
             call([3, 4, 2, 16, 0]), call([3, 4, 12, 3, 0]), call([0, 4, 12, 16, 0]), call(ok, tp=None), call(ok, H=0),
             call(ok, logits=(ctypes.c_void_p * 1)(None)),
             call([100, 100, 400, 400, 0], logits=(ctypes.c_void_p * 1)(big.data_ptr()))]       # a x40 stage-2 downsample: LDS
    torch.cuda.synchronize()
    assert all(c < 0 for c in codes), codes
    assert (lab == 0xAB).all() and (counts == 7).all()
    z40 = torch.zeros(40, 3, 4, device='cuda')
    assert call(ok, K=0, tp=None, cp=None) == 0                                  # labels only: K and targets unused
    assert call(ok, C=40, K=0, tp=None, cp=None, logits=(ctypes.c_void_p * 1)(z40.data_ptr())) == 0
    torch.cuda.synchronize()
    assert (lab == 0).all() and (counts == 7).all()


# -- the generators ------------------------------------------------------------------------------------------------------------------
def _voc_args(tree, run, extra):
    from mulactseg_amd.utils.common import get_parser
    base = ['-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--src_dataset', 'voc', '--or_labeling', '--fair_counting',
            '--nseg', str(tree['nseg']), '--num_classes', '21', '--trim_multihot_boundary', '--trim_kernel_size', '5',
            '--trg_data_dir', tree['root'], '--trg_datalist', tree['trg_datalist'], '--region_dict', tree['region_dict'],
            '--val_dataset', 'voc', '--val_data_dir', tree['root'], '--val_datalist', tree['val_datalist'], '--val_batch_size', '1',
            '--train_batch_size', '1', '--num_workers', '0', '--val_num_workers', '0', '-p', str(run)]
    a = get_parser().parse_args(base + list(extra))
    a.pretrained_backbone = False
    return a


MS = ('eval_save_cosplbl_naive_voc_ms', 'eval_region_voc_all_ms', 'eval_spx_identity_ms')
SS = ('eval_save_cosplbl_naive_voc', 'eval_region_voc_all', 'eval_spx_identity')


def _set(tree, run, kind, extra=()):
    from mulactseg_amd import dataloader
    dataloader.register_dataset_factory(None)
    a = _voc_args(tree, run, ['--method', kind[0], '--loader', kind[1], '--train_transform', kind[2]] + list(extra))
    os.makedirs(a.model_save_dir, exist_ok=True)
    return a, dataloader.get_active_dataset(a, train_transform=a.train_transform)


def _select_all(aset, every=3):
    pool = aset.trg_pool_dataset
    regions = []
    for key in pool.im_idx:
        for i, s in enumerate(pool.suppix[key[2]][::every]):
            regions.append((1.0 - 1e-4 * len(regions), ','.join(key), s))
    aset.selection_iter = 1
    aset.expand_training_set(regions, 10 ** 9, 'x')


def _generator(kind, a, ckpt):
    import importlib
    G = importlib.import_module("mulactseg_amd.trainer." + kind[0])
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    gen = G.ActiveTrainer(a, logging.getLogger("test"), 0)
    torch.save({'model_state_dict': gen.net.state_dict()}, ckpt)
    gen.net.eval()
    return gen


def test_the_identity_loader_yields_pillow_pictures_and_original_size_maps(tmp_path):
    _gpu()
    from PIL import Image
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=3, sizes=ODD_SIZES)
    a, aset = _set(tree, tmp_path / 'run', SS)
    _select_all(aset)
    label = aset.trg_label_dataset
    assert label.transform.n_maps == 2
    for idx in range(len(label.im_idx)):
        s = label[idx]
        name = s['fnames'][0].split('/')[-1].split('.')[0]
        k = tree['names'].index(name)
        pic = np.array(Image.open(os.path.join(tree['root'], 'VOC2012/JPEGImages', name + '.jpg')).convert('RGB'))
        H, W = pic.shape[:2]
        want = pic.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
        want = (want - np.asarray(MEAN, np.float32)[:, None, None]) / np.asarray(STD, np.float32)[:, None, None]
        assert s['images'].dtype == torch.float32 and np.array_equal(s['images'].cpu().numpy(), want.astype(np.float32))
        cls = tree['classes'][k]
        assert np.array_equal(s['labels'].cpu().numpy(), np.where(cls == 255, 21, cls))
        assert np.array_equal(s['spx'].cpu().numpy(), tree['spx'][k]) and s['imsizes'] == (W, H)


def test_the_fused_labels_match_the_aten_chain_on_a_seeded_network(tmp_path, monkeypatch):
    ops = _gpu()
    from mulactseg_amd.dataloader.device_transforms import DeviceMultiScaleFlip
    run = tmp_path / 'run'
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=1)
    a = _voc_args(tree, run, ['--method', MS[0], '--init_checkpoint', str(run / 'checkpoint01.tar')])
    os.makedirs(a.model_save_dir, exist_ok=True)
    gen = _generator(MS, a, str(run / 'checkpoint01.tar'))
    for H, W in ((375, 500), (131, 97)):
        pic = torch.from_numpy(np.random.RandomState(H).randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda()
        images = DeviceMultiScaleFlip()(pic)
        with torch.no_grad():
            zs, sizes, flips = gen.sources({'image_list': [images]})
            monkeypatch.delenv("MAS_MS_NAIVE", raising=False)
            fused = ops.ms_naive_labels(zs, sizes, flips, (H, W))
            monkeypatch.setenv("MAS_MS_NAIVE", "aten")
            aten = ops.ms_naive_labels(zs, sizes, flips, (H, W))
            monkeypatch.delenv("MAS_MS_NAIVE")
            m = ops.ms_ensemble([torch.ones((1, 1) + tuple(z.shape[2:]), device='cuda') for z in zs], zs, sizes, flips, (H, W))[1]
        top = torch.topk(m, 2, dim=1)[0]
        gap = (top[:, 0] - top[:, 1])
        differ = fused != aten
        print("ms_naive vs aten at %dx%d: %d of %d labels differ, all at a top-2 gap <= 1e-5" % (W, H, int(differ.sum()), H * W))
        assert bool((gap[differ] <= 1e-5).all()) and int(differ.sum()) <= 1e-3 * H * W


def _pngs(d):
    from PIL import Image
    return {f: np.array(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("kind, ptype, sub", [(SS, 'naive_argmax', 'plbl_gen_naive_argmax'), (MS, None, 'plbl_gen_ms')])
def test_the_generator_end_to_end(tmp_path, monkeypatch, capsys, kind, ptype, sub):
    """eval_AL_voc.py --method eval_save_cosplbl_naive_voc[_ms] (the README's Naive Inference), then train_stage2_AL_voc.py's
    --loader region_voc_plbl reads the PNGs."""
    ops = _gpu()
    from PIL import Image
    from mulactseg_amd import dataloader
    from mulactseg_amd.dataloader.constant import voc_id_to_color_map
    from mulactseg_amd.dataloader.utils import collate_fn
    # (pictures whose half-size copies keep every plane of the network >= 8 x 8: smaller planes run on MIOpen kernels that are not
    # run-to-run identical, and the comparisons below need one forward to equal the next)
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=3, sizes=((261, 341), (303, 265), (277, 277)))
    run = tmp_path / 'run'
    ckpt = str(run / 'checkpoint01.tar')
    a, aset = _set(tree, run, kind, ['--init_checkpoint', ckpt] + ([] if ptype is None else ['--plbl_type', ptype]))
    _select_all(aset)
    aset.dump_datalist()
    datalist = os.path.join(a.model_save_dir, 'datalist_01.pkl')
    gen = _generator(kind, a, ckpt)
    png_dir = run / sub / 'round_01'
    monkeypatch.delenv("MAS_MS_NAIVE", raising=False)
    runs = {}
    for workers, save_vis in ((1, False), (4, True)):
        monkeypatch.setenv("MAS_STAGE2_WORKERS", str(workers))
        gen.args.save_vis = save_vis
        gen.save_dir = None
        set2 = dataloader.get_active_dataset(a, train_transform=a.train_transform)
        set2.selection_iter = 1
        set2.load_datalist(datalist)
        capsys.readouterr()
        table = gen.eval(set2, selection_iter=0)
        out = capsys.readouterr().out
        for name in ('IoU', 'Precision', 'Recall'):
            assert out.count("[AL 0-round] %s: evaluation" % name) == 1
            line = out.split("[AL 0-round] %s: evaluation\n" % name)[1].split('\n')[0]
            assert len(line.split(',')) == 1 + 22
        assert len(table.split(',')) == 1 + 22 and table.split(',')[-1] == '0.00'          # class 21: seen, never predicted
        assert out.split("[AL 0-round] Precision: evaluation\n")[1].split('\n')[0].startswith('nan,')
        assert os.path.exists(str(png_dir) + '_vis') == save_vis
        runs[workers] = (table, _pngs(str(png_dir)))
    one, four = runs[1][1], runs[4][1]
    assert runs[1][0] == runs[4][0] and sorted(one) == sorted(four) == sorted(n + '.png' for n in tree['names'])
    assert all(np.array_equal(one[f], four[f]) for f in one)
    vis = _pngs(str(png_dir) + '_vis')
    assert sorted(vis) == sorted(one)
    ds = set2.trg_label_dataset
    for idx in range(len(ds.im_idx)):
        batch = collate_fn([ds[idx]])
        name = batch['fnames'][0][1].split('/')[-1].split('.')[0]
        got = one[name + '.png']
        H, W = tree['classes'][tree['names'].index(name)].shape
        assert got.dtype == np.uint8 and got.shape == (H, W) and got.max() <= 20
        with torch.no_grad():
            zs, sizes, flips = gen.sources(batch)
        up = [ops.upsample_bilinear(z, s) for z, s in zip(zs, sizes)]
        m = None
        for u, fl in zip(up, flips):
            v = torch.nn.functional.interpolate(u.flip(-1) if fl else u, size=(H, W), mode='bilinear', align_corners=False)
            m = v if m is None else m + v
        m = m / len(up)
        want = torch.max(m, 1)[1][0]
        top = torch.topk(m, 2, dim=1)[0][0]
        differ = torch.from_numpy(got).cuda().long() != want
        assert bool((top[0] - top[1])[differ].le(1e-5).all())                       # (the ATen chain rounds otherwise than the kernel)
        exact = R.labels([z[0].cpu().numpy() for z in zs], sizes, flips, (H, W))
        assert np.array_equal(got, exact.astype(np.uint8))
        pal = voc_id_to_color_map.astype(np.uint8)
        assert np.array_equal(vis[name + '.png'], RR.render_labels(got[None], pal, 21, batch['spx'].cpu().numpy().astype(np.int64))[0])
    # train_stage2_AL_voc.py: region_voc_plbl finds the PNGs
    a3 = _voc_args(tree, run, ['--stage2', '--init_iteration', '1', '--datalist_path', datalist, '--resume_checkpoint', ckpt,
                               '--init_checkpoint', ckpt, '--method', 'active_voc', '--loader', 'region_voc_plbl',
                               '--train_transform', 'rescale_513_notrg', '--loss_type', 'cross_entropy']
                   + ['--plbl_type', ptype if ptype is not None else 'ms'])
    a3.or_labeling, a3.dominant_labeling, a3.fair_counting = False, False, False
    set3 = dataloader.get_active_dataset(a3, train_transform=a3.train_transform)
    set3.selection_iter = 1
    set3.load_datalist(datalist)
    train_set = set3.get_trainset()
    assert train_set.plbl_root == str(png_dir) and len(train_set) == 3
    train_set.transform.rng = random.Random(5)
    s = train_set[0]
    from oracle import augment
    name = s['fnames'][0].split('/')[-1].split('.')[0]
    pic = np.array(Image.open(os.path.join(tree['root'], 'VOC2012/JPEGImages', name + '.jpg')).convert('RGB'))
    p = augment.draw_params(random.Random(5), pic.shape[0], pic.shape[1], (513, 513))
    img, (lab,) = augment.train_augment(pic, [one[name + '.png']], [255], p, (513, 513), MEAN, STD)
    assert np.array_equal(s['images'].cpu().numpy(), img) and np.array_equal(s['labels'].cpu().numpy(), lab)
