"""The two stage-2 ablations of paper Fig. 7 on the GPU: ``k_naive_plbl`` (csrc/naive_plbl.hip) against the materialised upsampling
and the restatement, ``k_spx_max_onehot`` (csrc/labels.hip) against its restatement and, through K9, against the oracle fed the
reference's rows; the three-map ``eval_dom_gt_spx`` samples of ``region_cityscapes_dom_w_gt`` against Pillow; and both generators
end to end (eval_AL.py flags of ``script/paper_experiment_final/figure7``), read back by ``region_cityscapes_plbl``."""
import logging
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
import naive_plbl_restated as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
H, W, NSEG = 128, 256, 64


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _logits(seed, N, C, h, w):
    rs = np.random.RandomState(seed)
    z = (2.0 * rs.randn(N, C, h, w)).astype(np.float32)
    z[:, 3, :4, :] = z[:, 1, :4, :]                         # exact ties at quarter resolution -> ties after the upsampling
    z[0, 7, h // 2, w // 2] = np.nan                        # a NaN logit: its footprint takes label 7 (the first NaN)
    return z


GEOMS = [(256, 512, 1024, 2048), (32, 64, 128, 256), (33, 41, 129, 161), (32, 64, 32, 64)]


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("C", [20, 21])
def test_kernel_is_the_argmax_of_the_materialised_upsampling(geom, C):
    ops = _gpu()
    h, w, Ho, Wo = geom
    N = 1 if Ho >= 1024 else 2
    zq = _logits(h * 7 + C, N, C, h, w)
    mask = np.random.RandomState(1).uniform(size=(N, Ho, Wo)) < 0.7
    zt, mt = torch.from_numpy(zq).cuda(), torch.from_numpy(mask).cuda()
    got = ops.naive_pseudo_labels(zt, (Ho, Wo), mt, 0.0).cpu().numpy()
    up = zt if (h, w) == (Ho, Wo) else ops.upsample_bilinear(zt, (Ho, Wo))
    up = up.cpu().numpy()
    want = np.where(mask, np.argmax(up, axis=1), 255)         # numpy: the first maximum, the first NaN
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(up, R.upsample(zq, Ho, Wo), equal_nan=True)     # the restatement's arithmetic is the kernel's
    assert np.array_equal(got, R.naive_labels(zq, Ho, Wo, mask, 0.0))
    assert np.isnan(up).any() and (got == 7).any()


@pytest.mark.parametrize("th", [0.2, 0.6])
def test_threshold_mode_agrees_with_float64_away_from_the_threshold(th):
    ops = _gpu()
    h, w, Ho, Wo = 32, 64, 128, 256
    zq = (3.0 * np.random.RandomState(4).randn(2, 20, h, w)).astype(np.float32)
    zt = torch.from_numpy(zq).cuda()
    got = ops.naive_pseudo_labels(zt, (Ho, Wo), None, th).cpu().numpy()
    up = ops.upsample_bilinear(zt, (Ho, Wo)).double().cpu().numpy()
    p = 1.0 / np.exp(up - up.max(axis=1, keepdims=True)).sum(axis=1)
    far = np.abs(p - th) > 1e-6
    assert np.array_equal(got[far] != 255, p[far] > th)
    assert np.array_equal(got[got != 255], np.argmax(up, axis=1)[got != 255])
    assert 0.01 < (got != 255).mean() < 0.99 and far.mean() > 0.999


def test_bad_geometry_is_refused():
    ops = _gpu()
    from mulactseg_amd import _lib
    z = torch.zeros((1, 20, 64, 64), device='cuda')
    m = torch.ones((1, 32, 32), dtype=torch.bool, device='cuda')
    with pytest.raises(ValueError, match="cannot be upsampled"):
        ops.naive_pseudo_labels(z, (32, 32), m, 0.0)                       # a downsampling
    with pytest.raises(ValueError, match="cannot be upsampled"):
        ops.naive_pseudo_labels(z, (64, 7 * 64), None, 0.5)                # wider than x6
    with pytest.raises(ValueError, match="spmask"):
        ops.naive_pseudo_labels(z, (128, 128), None, 0.0)
    out = torch.empty((1, 32, 32), dtype=torch.uint8, device='cuda')
    assert _lib.load().mas_naive_plbl(z.data_ptr(), 1, 20, 64, 64, 32, 32, m.data_ptr(), 0.0, out.data_ptr(), None) != 0


def _dominant_picture(seed, Hp, Wp, nseg):
    rs = np.random.RandomState(seed)
    spx = rs.randint(0, nseg - 3, size=(Hp, Wp))               # the last three ids carry no pixel
    spx[spx == 5] = 6
    dom = rs.randint(0, 20, size=nseg)
    t = dom[spx]
    t[rs.uniform(size=t.shape) < 0.03] = 255
    t[np.isin(spx, rs.choice(nseg, nseg // 3, replace=False))] = 255
    return t, spx


@pytest.mark.parametrize("S", [64, 2048])
@pytest.mark.parametrize("tdtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("sdtype", [torch.int64, torch.int32, torch.int16])
def test_spx_max_onehot_is_bit_exact_to_the_restatement(S, tdtype, sdtype):
    ops = _gpu()
    Hp, Wp = (128, 256) if S == 64 else (1024, 2048)
    t, spx = _dominant_picture(S, Hp, Wp, S)
    rows, mask = ops.spx_max_onehot(torch.from_numpy(t).to('cuda', tdtype), torch.from_numpy(spx).to('cuda', sdtype), S, 20)
    want_rows, want_mask = R.spx_max_onehot(t, spx, S, 20)
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (S, 20) and mask.dtype == torch.bool
    assert np.array_equal(rows.cpu().numpy(), want_rows) and np.array_equal(mask.cpu().numpy(), want_mask)
    assert rows[5].tolist() == [1] + [0] * 19
    bad = t.copy()
    bad[0, 0] = 21
    with pytest.raises(ValueError, match="outside"):
        ops.spx_max_onehot(torch.from_numpy(bad).cuda(), torch.from_numpy(spx).cuda(), S, 20)


def test_k9_on_these_rows_equals_the_oracle_on_the_reference_rows():
    """Rows sized nseg (this kernel) and max(id)+1 (the reference's scatter_max): the extra rows belong to no masked pixel."""
    ops = _gpu()
    from oracle import exact
    from test_oracle_golden import stage2_inputs
    N, C, Ch, Hp, Wp, S = 1, 20, 32, 64, 96, 48
    feats_full, z, _, spx, _, _ = stage2_inputs(29, N, C, Ch, Hp, Wp, S)
    q = torch.nn.functional.normalize(torch.nn.functional.avg_pool2d(torch.from_numpy(feats_full), 4)).numpy()
    spx = np.minimum(spx, S - 5)                                              # ids S-4 .. S-1 unused: max(id)+1 < nseg
    t, _ = _dominant_picture(3, Hp, Wp, S)
    dom = np.random.RandomState(3).randint(0, 20, size=S)
    t = np.where(t == 255, 255, dom[spx[0]])
    rows, mask = ops.spx_max_onehot(torch.from_numpy(t).cuda(), torch.from_numpy(np.ascontiguousarray(spx[0])).cuda(), S, C)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = ops.stage2_pseudo_labels(c(q), c(z), rows[None], mask[None], c(spx), True).cpu().numpy()
    ref_rows = R.spx_max_onehot_loop(t, spx[0], C)
    assert ref_rows.shape[0] == S - 4
    want = exact.stage2_pseudo_labels(q, z, ref_rows[None], (t != 255)[None], spx, True)
    assert np.array_equal(got, want) and (got != 255).any()


# -- the loader and the generators ---------------------------------------------------------------------------------------------
def _tree_with_dominant_maps(tmp_path):
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=3, H=H, W=W, nseg=NSEG)
    root = tree['root']
    lists = os.path.join(root, 'lists')
    plain = os.path.join(lists, 'train_seed%d.txt' % NSEG)
    dom = os.path.join(lists, 'train_seed%d_dominant.txt' % NSEG)
    with open(plain, 'w') as f:
        f.write('\n'.join('\t'.join([l.split('\t')[0], 'gtFine/train/%s/%s_gtFine_labelIds.png' % (s.split('_')[0], s), l.split('\t')[2]])
                          for l, s in zip(tree['lines'], tree['stems'])) + '\n')
    with open(dom, 'w') as f:
        f.write('\n'.join(l.replace('gtFine_or', 'gtFine_dominant').replace('.npy', '.png') for l in tree['lines']) + '\n')
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', 'mulactseg_amd.label_assignment', 'dominant', '--nseg', str(NSEG), '--spx_method', 'seeds',
                        '--trg_data_dir', root, '--trg_datalist', plain, '--region_dict', tree['region_dict'], '--generate_ignore',
                        '--num_worker', '2', '--nvis_color', '0'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    tree['dom_datalist'] = dom
    return tree


def _args(tree, run, extra, or_labeling):
    a = helpers.cityscapes_tree_args(tree, run, ['--stage2', '--val_batch_size', '1'] + list(extra))
    a.or_labeling = or_labeling
    a.dominant_labeling = not or_labeling
    a.val_batch_size = 1
    return a


def _selected_set(a):
    """The labelled set of one round: every second region of every picture, dumped as datalist_01.pkl."""
    from mulactseg_amd import dataloader
    dataloader.register_dataset_factory(None)
    os.makedirs(a.model_save_dir, exist_ok=True)
    aset = dataloader.get_active_dataset(a, train_transform=a.train_transform)
    pool = aset.trg_pool_dataset
    aset.selection_iter = 1
    if a.or_labeling:
        regions = []
        for key in pool.im_idx:
            for s in pool.suppix[key[2]][::2]:
                regions.append((1.0 - 1e-4 * len(regions), ','.join(key), s))
        aset.expand_training_set(regions, 10 ** 9, 'x')
    else:                                                     # (the dominant-label loaders keep no multi-hot index: set the lists)
        label = aset.trg_label_dataset
        label.im_idx = [list(k) for k in pool.im_idx]
        label.suppix = {k[2]: list(pool.suppix[k[2]][::2]) for k in pool.im_idx}
        pool.suppix = {k[2]: list(pool.suppix[k[2]][1::2]) for k in pool.im_idx}
    aset.dump_datalist()
    return os.path.join(a.model_save_dir, 'datalist_01.pkl')


def _dom_args(tree, run):
    ckpt = str(run / 'checkpoint01.tar')
    return _args(tree, run, ['--trg_datalist', tree['dom_datalist'], '--init_checkpoint', ckpt, '--resume_checkpoint', ckpt,
                             '--method', 'eval_save_cosplbl_prop_onehotignore', '--loader', 'region_cityscapes_dom_w_gt',
                             '--train_transform', 'eval_dom_gt_spx'], or_labeling=False)


@pytest.mark.parametrize("pred_ignore", [False, True])
def test_dom_w_gt_samples_equal_the_pillow_resize_of_the_decoded_files(tmp_path, pred_ignore):
    _gpu()
    from PIL import Image
    from mulactseg_amd import dataloader
    from mulactseg_amd.dataloader.formats import open_spx
    tree = _tree_with_dominant_maps(tmp_path)
    run = tmp_path / ('run_predignore' if pred_ignore else 'run')
    a = _dom_args(tree, run)
    datalist = _selected_set(a)
    aset = dataloader.get_active_dataset(a, train_transform=a.train_transform)
    aset.load_datalist(datalist)
    ds = aset.trg_label_dataset
    assert ds.pred_ignore == pred_ignore and ds.transform.n_maps == 3
    item = ds[1]
    img_f, lbl_f, spx_f = item['fnames']
    Hr, Wr = 1024, 2048                                        # ExtResize((1024, 2048)) of 128 x 256 pictures: a real resample
    pic = Image.open(img_f).convert('RGB').resize((Wr, Hr), Image.BILINEAR)
    ref_img = np.asarray(pic).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    ref_img = (ref_img - np.asarray(MEAN, np.float32)[:, None, None]) / np.asarray(STD, np.float32)[:, None, None]
    near = lambda arr: np.asarray(Image.fromarray(arr.astype(np.int32)).resize((Wr, Hr), Image.NEAREST)).astype(np.int64)
    dom = np.array(Image.open(lbl_f)).astype(np.int64)
    stem = lbl_f.split('/')[-1].split('.')[0]
    raw = np.array(Image.open(os.path.join(tree['root'], 'gtFine/train/%s/%s_gtFine_labelIds.png' % (stem.split('_')[0], stem))))
    lab = ds.encode_target(raw).astype(np.int64)
    if pred_ignore:
        dom[dom == 255] = 19
        lab[lab == 255] = 19
    spx = near(open_spx(spx_f))
    sel = np.isin(spx, ds.suppix[spx_f])
    assert np.array_equal(item['images'].cpu().numpy(), ref_img.astype(np.float32))
    assert np.array_equal(item['spx'].cpu().numpy(), spx)
    assert np.array_equal(item['labels'].cpu().numpy(), near(lab))
    assert np.array_equal(item['target'].cpu().numpy(), np.where(sel, near(dom), 255))
    assert np.array_equal(item['spmask'].cpu().numpy(), sel) and sel.any() and not sel.all()
    assert (item['labels'] == 255).any() != pred_ignore


def _generator(module, a, ckpt):
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    gen = module.ActiveTrainer(a, logging.getLogger("test"), 0)
    torch.save({'model_state_dict': gen.net.state_dict()}, ckpt)
    gen.load_checkpoint(ckpt)
    return gen


def _generate(gen, a, datalist, monkeypatch, workers):
    from mulactseg_amd import dataloader
    monkeypatch.setenv("MAS_STAGE2_WORKERS", str(workers))
    aset = dataloader.get_active_dataset(a, train_transform=a.train_transform)
    aset.trg_label_dataset.transform.target = (H, W)          # the pictures at their native size (the forward stays small)
    aset.selection_iter = 1
    aset.load_datalist(datalist)
    gen.save_dir = None
    return gen.eval(aset, selection_iter=0), aset


def _pngs(d):
    from PIL import Image
    return {f: np.array(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d))}


def _read_back(tree, run, datalist, ckpt, png_dir, extra):
    """train_stage2_AL.py ... --loader region_cityscapes_plbl: the training set finds the PNGs and a sample is the Pillow pipeline."""
    from PIL import Image
    from mulactseg_amd import dataloader
    from oracle import augment
    a3 = _args(tree, run, ['--init_iteration', '1', '--datalist_path', datalist, '--resume_checkpoint', str(run / 'checkpoint01.pkl'),
                           '--init_checkpoint', ckpt, '--method', 'active_predignore', '--loader', 'region_cityscapes_plbl',
                           '--train_transform', 'rescale_769_nospx', '--loss_type', 'cross_entropy'] + extra, or_labeling=False)
    set3 = dataloader.get_active_dataset(a3, train_transform=a3.train_transform)
    set3.selection_iter = 1
    set3.load_datalist(datalist)
    train_set = set3.get_trainset()
    assert train_set.plbl_root == str(png_dir) and len(train_set) == 3
    train_set.transform.size = (128, 128)
    train_set.transform.rng = random.Random(5)
    s = train_set[0]
    k = tree['stems'].index(s['fnames'][0].split('/')[-1].split('_leftImg8bit')[0])
    png = np.array(Image.open(str(png_dir / (tree['stems'][k] + '.png'))))
    p = augment.draw_params(random.Random(5), H, W, (128, 128))
    img, (lab,) = augment.train_augment(tree['pictures'][k], [png], [255], p, (128, 128), MEAN, STD)
    assert np.array_equal(s['images'].cpu().numpy(), img) and np.array_equal(s['labels'].cpu().numpy(), lab)


def test_naive_generator_end_to_end(tmp_path, monkeypatch, capsys):
    """figure7/(a)wo_prototype_.sh: eval_AL.py --method eval_save_naiveplbl --plbl_type naive --or_labeling --train_transform eval_spx
    --loader eval_region_cityscapes_all, then the training half's region_cityscapes_plbl --plbl_type naive."""
    ops = _gpu()
    from PIL import Image
    from mulactseg_amd.dataloader.utils import collate_fn
    from mulactseg_amd.trainer import eval_save_naiveplbl as G
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=3, H=H, W=W, nseg=NSEG)
    run = tmp_path / 'run'
    ckpt = str(run / 'checkpoint01.tar')
    a = _args(tree, run, ['--init_checkpoint', ckpt, '--resume_checkpoint', ckpt, '--method', 'eval_save_naiveplbl', '--plbl_type', 'naive',
                          '--loader', 'eval_region_cityscapes_all', '--train_transform', 'eval_spx', '--trim_multihot_boundary',
                          '--trim_kernel_size', '5'], or_labeling=True)
    datalist = _selected_set(a)
    gen = _generator(G, a, ckpt)
    png_dir = run / 'plbl_gen_naive' / 'round_01'
    (table, aset) = _generate(gen, a, datalist, monkeypatch, 1)
    one = _pngs(png_dir)
    out = capsys.readouterr().out
    assert out.count("[AL 0-round]: evaluation") == 1 and len(table.split(',')) == 1 + 20
    assert sorted(one) == sorted(s + '.png' for s in tree['stems'])
    _generate(gen, a, datalist, monkeypatch, 4)
    four = _pngs(png_dir)
    assert sorted(four) == sorted(one) and all(np.array_equal(one[f], four[f]) for f in one)
    # a PNG = the reference's lines on the logits of the same sample (with the upsampling of ops.upsample_bilinear)
    ds = aset.trg_label_dataset
    batch = collate_fn([ds[0]])
    with torch.no_grad():
        zq = gen.net(batch['images'].cuda(), lowres=True)
        z = ops.upsample_bilinear(zq.contiguous(), (H, W)).cpu().numpy()
    mask = batch['spmask'].cpu().numpy()
    want = np.where(mask, np.argmax(z, axis=1), 255)[0].astype(np.uint8)
    name = batch['fnames'][0][1].split('/')[-1].split('.')[0]
    assert np.array_equal(one[name + '.png'], want) and one[name + '.png'].dtype == np.uint8 and (want != 255).any()
    _read_back(tree, run, datalist, ckpt, png_dir, ['--plbl_type', 'naive'])


def test_onehotignore_generator_end_to_end(tmp_path, monkeypatch, capsys):
    """figure7/(b)Cityscapes_Stage2_Dom+PixBal.sh: eval_AL.py --method eval_save_cosplbl_prop_onehotignore --dominant_labeling
    --train_transform eval_dom_gt_spx --loader region_cityscapes_dom_w_gt (a 'predignore' run directory), then region_cityscapes_plbl."""
    ops = _gpu()
    from oracle import exact
    from mulactseg_amd.dataloader.utils import collate_fn
    from mulactseg_amd.trainer import eval_save_cosplbl_prop_onehotignore as G
    tree = _tree_with_dominant_maps(tmp_path)
    run = tmp_path / 'deepstem50_method-active_joint_multi_predignore_lossdecomp-_'
    a = _dom_args(tree, run)
    ckpt = a.init_checkpoint
    datalist = _selected_set(a)
    gen = _generator(G, a, ckpt)
    png_dir = run / 'plbl_gen' / 'round_01'
    table, aset = _generate(gen, a, datalist, monkeypatch, 1)
    one = _pngs(png_dir)
    out = capsys.readouterr().out
    for name in ('IoU', 'Precision', 'Recall'):
        assert out.count("[AL 0-round] %s: evaluation" % name) == 1
    assert len(table.split(',')) == 1 + 20 and sorted(one) == sorted(s + '.png' for s in tree['stems'])
    _generate(gen, a, datalist, monkeypatch, 4)
    four = _pngs(png_dir)
    assert sorted(four) == sorted(one) and all(np.array_equal(one[f], four[f]) for f in one)
    # a PNG = the oracle fed the reference's rows (scatter_max over max(id)+1 segments) and mask on the same sample
    ds = aset.trg_label_dataset
    assert ds.pred_ignore
    batch = collate_fn([ds[0]])
    t, spx = batch['target'][0].cpu().numpy(), batch['spx'][0].cpu().numpy()
    with torch.no_grad():
        feats, logits = gen.net.feat_forward_lowres(batch['images'].cuda())
    want = exact.stage2_pseudo_labels(feats.cpu().numpy(), logits.cpu().numpy(), R.spx_max_onehot_loop(t, spx, 20)[None],
                                      (t != 255)[None], spx[None], True)[0]
    name = batch['fnames'][0][1].split('/')[-1].split('.')[0]
    assert np.array_equal(one[name + '.png'], want.astype(np.uint8)) and (want != 255).any()
    _read_back(tree, run, datalist, ckpt, png_dir, [])
