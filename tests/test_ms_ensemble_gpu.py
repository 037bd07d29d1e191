"""The multi-scale + flip stage-2 pseudo labels of VOC on the GPU: the ``eval_spx_identity_ms`` pictures against Pillow, the fused
ensemble kernel (``ops.ms_ensemble``, csrc/ms_ensemble.hip) bit for bit against the numpy restatement (tests/ms_ensemble_restated.py),
the fused path against the ATen chain on a seeded network, and a generator run from the files to a stage-2 training sample."""
import logging
import os
import random
import sys

import numpy as np
import pytest
import torch

import helpers
import ms_ensemble_restated as R

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ODD_SIZES = ((121, 161), (153, 111), (97, 128), (131, 130))


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _pillow_tta(pic):
    """TestTimeAugmentation (ext_transforms.py:18-46) on the host: Image.resize(BILINEAR), flip, /255, (x - mean) / std."""
    from PIL import Image
    H, W = pic.shape[:2]
    out = []
    for flip in (False, True):
        for f in (0.5, 0.75, 1.0, 1.25, 1.5):
            im = Image.fromarray(pic).resize((int(f * W), int(f * H)), Image.BILINEAR)
            if flip:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            t = np.asarray(im).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
            t = (t - np.asarray(MEAN, np.float32)[:, None, None]) / np.asarray(STD, np.float32)[:, None, None]
            out.append(t.astype(np.float32))
    return out


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


def _ms_set(tree, run, extra=()):
    from mulactseg_amd import dataloader
    dataloader.register_dataset_factory(None)
    a = _voc_args(tree, run, ['--method', 'eval_save_cosplbl_prop_includeonehot_voc_ms', '--loader', 'eval_region_voc_all_ms',
                              '--train_transform', 'eval_spx_identity_ms'] + list(extra))
    os.makedirs(a.model_save_dir, exist_ok=True)
    return a, dataloader.get_active_dataset(a, train_transform=a.train_transform)


def _select_all(aset, every=3):
    """Put every third region of every picture into the labelled set (one round)."""
    pool = aset.trg_pool_dataset
    regions = []
    for key in pool.im_idx:
        for i, s in enumerate(pool.suppix[key[2]][::every]):
            regions.append((1.0 - 1e-4 * len(regions), ','.join(key), s))
    aset.selection_iter = 1
    aset.expand_training_set(regions, 10 ** 9, 'x')


# -- the transform and the loader ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [None, ODD_SIZES])
def test_the_ms_loader_yields_the_pillow_tta_and_original_size_maps(tmp_path, sizes):
    _gpu()
    from PIL import Image
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=4, **({} if sizes is None else {'sizes': sizes}))
    a, aset = _ms_set(tree, tmp_path / 'run')
    _select_all(aset)
    label = aset.trg_label_dataset
    assert label.transform.n_maps == 0
    for idx in range(len(label.im_idx)):
        s = label[idx]
        name = s['fnames'][0].split('/')[-1].split('.')[0]
        k = tree['names'].index(name)
        pic = np.array(Image.open(os.path.join(tree['root'], 'VOC2012/JPEGImages', name + '.jpg')).convert('RGB'))
        H, W = pic.shape[:2]
        want = _pillow_tta(pic)
        assert len(s['image_list']) == 10
        for got, w in zip(s['image_list'], want):
            assert got.dtype == torch.float32 and tuple(got.shape) == w.shape and np.array_equal(got.cpu().numpy(), w)
        cls = tree['classes'][k]
        assert s['labels'].dtype == torch.int64 and np.array_equal(s['labels'].cpu().numpy(), np.where(cls == 255, 21, cls))
        assert np.array_equal(s['spx'].cpu().numpy(), tree['spx'][k]) and s['imsizes'] == (W, H)
        sel = label.suppix[s['fnames'][2]]
        has_cls = tree['multi_hot'][k, :, :21].sum(axis=1) != 0
        assert np.array_equal(s['spmask'].cpu().numpy(), np.isin(tree['spx'][k], [i for i in sel if has_cls[i]]))


def test_the_tta_of_a_voc_sized_picture_equals_pillow():
    _gpu()
    from mulactseg_amd.dataloader.device_transforms import DeviceMultiScaleFlip
    pic = np.random.RandomState(3).randint(0, 256, size=(375, 500, 3)).astype(np.uint8)
    got = DeviceMultiScaleFlip()(torch.from_numpy(pic).cuda())
    want = _pillow_tta(pic)
    assert [tuple(g.shape) for g in got] == [w.shape for w in want]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    assert np.array_equal(got[2].cpu().numpy(), want[2])            # factor 1.0: the identity resize


# -- the kernel against the restatement --------------------------------------------------------------------------------------------
def _sources(rs, sizes, Ch, C):
    fq, lq = [], []
    for Hs, Ws in sizes:
        f = rs.standard_normal((Ch, R.quarter_size(Hs), R.quarter_size(Ws))).astype(np.float32)
        fq.append((f / np.sqrt((f.astype(np.float64) ** 2).sum(0))).astype(np.float32))
        lq.append(rs.uniform(-1, 1, (C, R.quarter_size(Hs), R.quarter_size(Ws))).astype(np.float32))
    return fq, lq


def _run(fq, lq, sizes, flips, out_size):
    from mulactseg_amd import ops
    f, z = ops.ms_ensemble([torch.from_numpy(q)[None].cuda() for q in fq], [torch.from_numpy(q)[None].cuda() for q in lq],
                           sizes, flips, out_size)
    torch.cuda.synchronize()
    return f[0].cpu().numpy(), z[0].cpu().numpy()


CASES = [  # (H, W, Ch, C, which sources of the TTA list)
    (120, 160, 256, 21, range(10)), (150, 110, 256, 22, range(10)), (96, 128, 16, 21, [2]), (131, 130, 256, 22, [2]),
    (121, 161, 16, 22, [0, 9]), (153, 111, 256, 21, [4, 5]), (97, 129, 16, 21, range(5, 10)), (130, 130, 16, 22, [7]),
    (375, 500, 64, 21, range(10)), (500, 333, 64, 22, range(10)), (375, 500, 16, 21, [3, 8]),
]


@pytest.mark.parametrize("H, W, Ch, C, which", CASES)
def test_the_kernel_is_bit_exact_to_the_restatement(H, W, Ch, C, which):
    _gpu()
    rs = np.random.RandomState(H * 7 + W * 3 + Ch + C)
    sizes, flips = R.tta_sizes(H, W)
    sizes, flips = [sizes[i] for i in which], [flips[i] for i in which]
    fq, lq = _sources(rs, sizes, Ch, C)
    got_f, got_z = _run(fq, lq, sizes, flips, (H, W))
    want_f, want_z = R.ms_ensemble(fq, lq, sizes, flips, (H, W))
    assert np.array_equal(got_z, want_z), np.abs(got_z - want_z).max()
    assert np.array_equal(got_f, want_f), np.abs(got_f - want_f).max()
    assert np.abs(np.sqrt((got_f.astype(np.float64) ** 2).sum(0)) - 1.0).max() < 1e-5


@pytest.mark.parametrize("Hs, Ws", [(187, 250), (375, 500), (563, 750), (61, 81)])
def test_stage1_alone_equals_the_upsampling_kernel(Hs, Ws):
    """One source, not flipped, resized to its own size (every stage-2 weight is exactly 1): the logits are stage 1 itself, which
    equals ops.upsample_bilinear on the materialised tensor bit for bit (and the restatement's stage 1)."""
    _gpu()
    from mulactseg_amd import ops
    rs = np.random.RandomState(Hs)
    fq, lq = _sources(rs, [(Hs, Ws)], 16, 21)
    _, got_z = _run(fq, lq, [(Hs, Ws)], [False], (Hs, Ws))
    up = ops.upsample_bilinear(torch.from_numpy(lq[0])[None].cuda(), (Hs, Ws))[0].cpu().numpy()
    assert np.array_equal(got_z, up) and np.array_equal(R.stage1(lq[0], Hs, Ws), up)


def test_a_zero_feature_vector_stays_zero_and_bad_geometry_is_refused():
    _gpu()
    from mulactseg_amd import ops, _lib
    fq = [np.zeros((8, 3, 4), np.float32)]
    lq = [np.ones((21, 3, 4), np.float32)]
    f, z = _run(fq, lq, [(12, 16)], [True], (10, 14))
    assert np.array_equal(f, np.zeros((8, 10, 14), np.float32)) and np.array_equal(z, np.ones((21, 10, 14), np.float32))
    q = torch.zeros(1, 8, 3, 4, device='cuda')
    z = torch.zeros(1, 21, 3, 4, device='cuda')
    with pytest.raises(ValueError):
        ops.ms_ensemble([q], [z], [(16, 16)], [False], (10, 14))         # 16 x 16 emits 4 x 4, not 3 x 4
    with pytest.raises(ValueError):
        ops.ms_ensemble([q], [z], [(0, 16)], [False], (10, 14))
    with pytest.raises(ValueError):
        ops.ms_ensemble([q], [z[:, :, :2]], [(12, 16)], [False], (10, 14))
    with pytest.raises(TypeError):
        ops.ms_ensemble([q.double()], [z], [(12, 16)], [False], (10, 14))
    with pytest.raises(ValueError):
        ops.ms_ensemble([q.transpose(2, 3).contiguous().transpose(2, 3)], [z], [(12, 16)], [False], (10, 14))
    # the C entry point refuses bad sizes without launching: hq > Hs, no source, too many sources
    import ctypes
    lib = _lib.load()
    fp, lp = (ctypes.c_void_p * 1)(q.data_ptr()), (ctypes.c_void_p * 1)(z.data_ptr())
    out_f, out_z = torch.empty(8, 10, 14, device='cuda'), torch.empty(21, 10, 14, device='cuda')
    for geom, n in (([3, 4, 2, 16, 0], 1), ([3, 4, 12, 16, 0], 0), ([3, 4, 12, 16, 0], 17)):
        g = (ctypes.c_int32 * 5)(*geom)
        assert lib.mas_ms_ensemble(fp, lp, g, n, 8, 21, 10, 14, out_f.data_ptr(), out_z.data_ptr(), None) != 0


# -- the fused path against the ATen chain, and the generator end to end ---------------------------------------------------------------
def _generator(a, ckpt):
    from mulactseg_amd.trainer import eval_save_cosplbl_prop_includeonehot_voc_ms as G
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    gen = G.ActiveTrainer(a, logging.getLogger("test"), 0)
    torch.save({'model_state_dict': gen.net.state_dict()}, ckpt)
    gen.net.eval()
    return gen


def test_the_fused_ensemble_matches_the_aten_chain_on_a_seeded_network(tmp_path, monkeypatch):
    _gpu()
    from mulactseg_amd.dataloader.device_transforms import DeviceMultiScaleFlip
    run = tmp_path / 'run'
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=1)
    a = _voc_args(tree, run, ['--method', 'eval_save_cosplbl_prop_includeonehot_voc_ms', '--init_checkpoint', str(run / 'checkpoint01.tar')])
    os.makedirs(a.model_save_dir, exist_ok=True)
    gen = _generator(a, str(run / 'checkpoint01.tar'))
    for H, W in ((375, 500), (131, 97)):
        pic = torch.from_numpy(np.random.RandomState(H).randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda()
        images = DeviceMultiScaleFlip()(pic)
        with torch.no_grad():
            monkeypatch.delenv("MAS_MS_ENSEMBLE", raising=False)
            f1, z1 = gen.ensemble(images, (H, W))
            monkeypatch.setenv("MAS_MS_ENSEMBLE", "aten")
            f0, z0 = gen.ensemble(images, (H, W))
        monkeypatch.delenv("MAS_MS_ENSEMBLE")
        assert f1.shape == f0.shape == (1, 256, H, W) and z1.shape == z0.shape == (1, 21, H, W)
        df = float((f1 - f0).abs().max())
        dz = float(((z1 - z0).abs() / z0.abs().clamp(min=1.0)).max())
        print("ms_ensemble vs aten at %dx%d: features max|d| %.3g, logits max rel %.3g" % (W, H, df, dz))
        assert df <= 1e-5 and dz <= 1e-5


def _assignment(feats, logits, batch):
    """K9's nearest-prototype assignment of one picture (ops.stage2_pseudo_labels up to the per-prototype medians) -> host arrays
    (nn [H*W], nn_sim [H*W], thr [n_proto])."""
    from mulactseg_amd import ops, _lib
    dev = logits.device
    spx, mask = batch['spx'].to(dev), ops._mask_u8(batch['spmask'].to(dev))
    bits = ops.target_bits(batch['target'].to(dev).to(torch.uint8).contiguous())
    _, C, H, W = logits.shape
    Ch = feats.shape[1]
    S = batch['target'].shape[1]
    _, _, gmax = ops.partial_loss_fwd(logits.contiguous(), spx, mask, bits, 1.0, _lib.LOSS_GROUP)
    g = gmax[0]
    nz = (g != 0).nonzero()
    proto_s, proto_c = nz[:, 0], nz[:, 1]
    proto_pix = (0xffffffff - (g[proto_s, proto_c] & 0xffffffff)).to(torch.int32)
    p_start = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    p_start[1:] = torch.cumsum(torch.bincount(proto_s, minlength=S), 0).to(torch.int32)
    P = torch.empty((nz.shape[0], Ch), dtype=torch.float32, device=dev)
    f = feats[0].contiguous()
    lib, st = _lib.load(), ops._stream(logits)
    _lib.check(lib.mas_stage2_gather_protos(f.data_ptr(), Ch, H, W, H, W, proto_pix.data_ptr(), nz.shape[0], P.data_ptr(), st), "gather")
    nn = torch.empty(H * W, dtype=torch.int32, device=dev)
    nn_sim = torch.empty(H * W, dtype=torch.float32, device=dev)
    _lib.check(lib.mas_stage2_assign(f.data_ptr(), Ch, H, W, H, W, spx[0].data_ptr(), mask[0].data_ptr(), S, p_start.data_ptr(), P.data_ptr(),
                                     nn.data_ptr(), nn_sim.data_ptr(), st), "assign")
    nn_h, sim_h = nn.cpu().numpy(), nn_sim.cpu().numpy().astype(np.float64)
    thr = np.ones(nz.shape[0])
    for j in range(nz.shape[0]):
        v = np.sort(sim_h[nn_h == j].astype(np.float32))
        if len(v):
            thr[j] = v[(len(v) - 1) // 2]
    return nn_h, sim_h, thr, P.double().cpu().numpy(), proto_s.cpu().numpy()


def _near_tie(feats, a, y, x, eps=1e-5):
    """K9's decision at pixel (y, x) is a tie at the scale eps: its own nearest-prototype similarity at a median threshold, or -- for
    the propagation from adjacent superpixels -- some similarity at a prototype's threshold, or two prototypes of one superpixel at
    the same similarity."""
    nn, sim, thr, P, owner = a
    W = feats.shape[-1]
    if nn[y * W + x] >= 0 and abs(sim[y * W + x] - thr[nn[y * W + x]]) <= eps:
        return True
    f = feats[0, :, y, x].double().cpu().numpy()
    s = P @ f
    if (np.abs(s - thr) <= eps).any():
        return True
    for g in np.unique(owner):
        Pg = np.unique(P[owner == g], axis=0)           # (prototypes at one pixel have one feature: the first maximum decides, no tie)
        v = np.sort(Pg @ f)
        if len(v) > 1 and (np.diff(v) <= eps).any():
            return True
    return False


def test_the_ms_generator_writes_pngs_a_stage2_loader_reads(tmp_path, monkeypatch, capsys):
    """eval_AL.py --method eval_save_cosplbl_prop_includeonehot_voc_ms --train_transform eval_spx_identity_ms --loader
    eval_region_voc_all_ms, then train_stage2_AL.py's --loader region_voc_plbl --plbl_type ms reads the PNGs."""
    _gpu()
    from PIL import Image
    from mulactseg_amd import dataloader
    from mulactseg_amd.dataloader.utils import collate_fn
    # (pictures whose half-size copies keep every plane of the network >= 8 x 8: smaller planes run on MIOpen kernels that are not
    # run-to-run identical, and the comparisons below need one forward to equal the next)
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=3, sizes=((261, 341), (303, 265), (277, 277)))
    run = tmp_path / 'run'
    ckpt = str(run / 'checkpoint01.tar')
    a, aset = _ms_set(tree, run, ['--init_checkpoint', ckpt])
    _select_all(aset)
    aset.dump_datalist()
    datalist = os.path.join(a.model_save_dir, 'datalist_01.pkl')
    assert os.path.exists(datalist)
    gen = _generator(a, ckpt)
    set2 = dataloader.get_active_dataset(a, train_transform=a.train_transform)
    set2.selection_iter = 1
    set2.load_datalist(datalist)
    monkeypatch.delenv("MAS_MS_ENSEMBLE", raising=False)
    table = gen.eval(set2, selection_iter=0)
    assert len(table.split(',')) == 1 + 22
    assert "[AL 0-round]" in capsys.readouterr().out
    png_dir = run / 'plbl_gen_ms' / 'round_01'
    assert sorted(os.listdir(png_dir)) == sorted(n + '.png' for n in tree['names'])
    # the maps of the fused ensemble equal those of the ATen chain on the same ten quarter-resolution forwards (the forward itself is
    # not bit-reproducible from run to run at every one of these input sizes, so both ensembles start from one set of forwards)
    from mulactseg_amd import ops
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from ms_ensemble_probe import aten_chain
    ds = set2.trg_label_dataset
    gen.net.eval()
    for idx in range(len(ds.im_idx)):
        batch = collate_fn([ds[idx]])
        name = batch['fnames'][0][1].split('/')[-1].split('.')[0]
        got = np.array(Image.open(str(png_dir / (name + '.png'))))
        k = tree['names'].index(name)
        H, W = tree['classes'][k].shape
        assert got.dtype == np.uint8 and got.shape == (H, W) and set(np.unique(got).tolist()) <= set(range(22)) | {255}
        imgs = batch['image_list'][0]
        sizes, flips = [tuple(im.shape[-2:]) for im in imgs], [i >= 5 for i in range(10)]
        with torch.no_grad():
            q = [gen.net.feat_forward_quarter(im[None]) for im in imgs]
            fq, lq = [f.contiguous() for f, _ in q], [z.contiguous() for _, z in q]
            f1, z1 = ops.ms_ensemble(fq, lq, sizes, flips, (H, W))
            f0, z0 = aten_chain(fq, lq, sizes, flips, (H, W))
            dev = gen.device
            args = (batch['labels'].to(dev), batch['target'].to(dev), batch['spmask'].to(dev), batch['spx'].to(dev))
            fused = gen.pseudo_label_generation(args[0], f1, z1.contiguous(), *args[1:])[0].cpu().numpy()
            aten = gen.pseudo_label_generation(args[0], f0, z0.contiguous(), *args[1:])[0].cpu().numpy()
        differ = np.argwhere(fused != aten)
        if len(differ):
            # The two ensembles differ by rounding (<= 1e-5, test above), and K9 turns some of that into label changes: a pixel whose
            # nearest prototype is a tie at that scale swaps prototypes, which moves that prototype's median threshold, which changes
            # what the propagation accepts elsewhere.  Shown here: the prototypes are the same pixels on both paths, every pixel whose
            # nearest prototype differs is such a tie, and the labels that change stay below 1 % of the picture.
            a1, a0 = _assignment(f1, z1, batch), _assignment(f0, z0, batch)
            assert np.array_equal(a1[4], a0[4]) and a1[3].shape == a0[3].shape
            swapped = np.flatnonzero((a1[0] != a0[0]) & (a1[0] >= 0) & (a0[0] >= 0))
            fh = f1[0].reshape(f1.shape[1], -1)
            for p in swapped:
                f = fh[:, p].double().cpu().numpy()
                gap = abs(float(a1[3][a1[0][p]] @ f) - float(a1[3][a0[0][p]] @ f))
                assert gap <= 1e-5, "pixel %d changes its nearest prototype without a near-tie (gap %.3g)" % (p, gap)
            near = sum(_near_tie(f1, a1, y, x) or _near_tie(f0, a0, y, x) for y, x in differ)
            print("%s: %d of %d pixels differ from the ATen chain (%d near-ties at the pixel itself, %d nearest-prototype swaps, "
                  "all ties)" % (name, len(differ), fused.size, near, len(swapped)))
            assert len(differ) <= 1e-2 * fused.size, "%d pixels differ from the ATen chain" % len(differ)
        assert (fused != 255).any()
    # train_stage2_AL.py: region_voc_plbl with --plbl_type ms finds them
    a3 = _voc_args(tree, run, ['--stage2', '--init_iteration', '1', '--datalist_path', datalist, '--resume_checkpoint', ckpt,
                               '--init_checkpoint', ckpt, '--method', 'active_voc', '--loader', 'region_voc_plbl', '--plbl_type', 'ms',
                               '--train_transform', 'rescale_513_notrg', '--loss_type', 'cross_entropy'])
    a3.or_labeling, a3.dominant_labeling, a3.fair_counting = False, False, False
    set3 = dataloader.get_active_dataset(a3, train_transform=a3.train_transform)
    set3.selection_iter = 1
    set3.load_datalist(datalist)
    train_set = set3.get_trainset()
    assert train_set.plbl_root == str(png_dir) and len(train_set) == 3
    train_set.transform.rng = random.Random(5)
    s = train_set[0]
    assert tuple(s['images'].shape) == (3, 513, 513) and tuple(s['labels'].shape) == (513, 513) and s['labels'].dtype == torch.int64
    from oracle import augment
    name = s['fnames'][0].split('/')[-1].split('.')[0]
    pic = np.array(Image.open(os.path.join(tree['root'], 'VOC2012/JPEGImages', name + '.jpg')).convert('RGB'))
    png = np.array(Image.open(str(png_dir / (name + '.png'))))
    p = augment.draw_params(random.Random(5), pic.shape[0], pic.shape[1], (513, 513))
    img, (lab,) = augment.train_augment(pic, [png], [255], p, (513, 513), MEAN, STD)
    assert np.array_equal(s['images'].cpu().numpy(), img) and np.array_equal(s['labels'].cpu().numpy(), lab)
