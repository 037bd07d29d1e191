"""``k_candidate_plbl`` (csrc/candidate_plbl.hip) and ``k_stage2_assign_labels`` (csrc/stage2.hip) on the GPU: against the materialised
upsampling and the numpy restatement bit for bit, against float64 away from the threshold, against the executed reference
(tests/golden/g12_stage2_variants.npz), the counters, the refusals, and the four generators end to end (``eval_AL.py`` flags
``--loader eval_region_cityscapes_all --train_transform eval_spx --or_labeling --val_batch_size 1``), read back by
``region_cityscapes_plbl``."""
import os
import types

import numpy as np
import pytest
import torch

import candidate_plbl_restated as CR
import helpers
import naive_plbl_restated as R
from test_naive_plbl_gpu import MEAN, NSEG, STD, _args, _generator, _logits, _pngs, _selected_set
from test_oracle_golden import digest, stage2_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN, SET_ASIDE = 1e-6, 1e-3          # tests/test_naive_plbl_gpu.py:70; at most 0.1 % of the pixels within it


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _picture(seed, N, C, S, h, w, Ho, Wo):
    """Logits with exact ties, a NaN and a +inf in an excluded channel of a selected pixel; per-pixel random ids, half the superpixels
    selected; sparse rows (so many candidate sets are all negative), one selected row all ones, one with a single class; one selected
    pixel whose id is S."""
    rs = np.random.RandomState(seed)
    zq = _logits(seed, N, C, h, w)
    spx = rs.randint(0, S, size=(N, Ho, Wo)).astype(np.int64)
    rows = (rs.uniform(size=(N, S, C)) < 0.15).astype(np.uint8)
    chosen = rs.choice(S, S // 2, replace=False)
    rows[:, chosen[0], :] = 1
    rows[:, chosen[1], :] = 0
    rows[:, chosen[1], C - 2] = 1
    mask = np.isin(spx, chosen)
    y, x = [int(v[0]) for v in np.nonzero(mask[1] & ~np.isin(spx[1], chosen[:2]))]
    rows[1, spx[1, y, x], 4] = 0
    zq[1, 4, y * h // Ho, x * w // Wo] = np.inf              # (an excluded channel of that pixel: inf * 0)
    yb, xb = [int(v[3]) for v in np.nonzero(mask[0])]
    spx[0, yb, xb] = S                                       # selected, and no row
    return zq, spx, rows, mask, (yb, xb)


GEOMS = [(32, 64, 128, 256), (33, 41, 129, 161), (32, 64, 32, 64)]


@pytest.mark.parametrize("S", [64, 2048])
@pytest.mark.parametrize("C", [20, 21])
@pytest.mark.parametrize("geom", GEOMS)
def test_kernel_equals_the_materialised_upsampling_and_the_restatement(geom, C, S):
    ops = _gpu()
    h, w, Ho, Wo = geom
    zq, spx, rows, mask, (yb, xb) = _picture(h * 5 + C + S, 2, C, S, h, w, Ho, Wo)
    zt = c(zq)
    up = (zt if (h, w) == (Ho, Wo) else ops.upsample_bilinear(zt, (Ho, Wo))).cpu().numpy()
    assert np.array_equal(up, R.upsample(zq, Ho, Wo), equal_nan=True)            # the restatement's arithmetic is the kernel's
    assert np.isnan(up).any() and np.isinf(up).any()
    # candidate mode
    got = ops.candidate_pseudo_labels(zt, (Ho, Wo), c(mask), targets_rows=c(rows), superpixels=c(spx)).cpu().numpy()
    want = np.where(mask, CR.candidate_argmax(up, rows, spx), 255)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(got, CR.labels(zq, Ho, Wo, mask, rows=rows, spx=spx))
    assert got[0, yb, xb] == 255 and mask[0, yb, xb] and (got[mask] != 255).sum() == mask.sum() - 1
    picked = np.take_along_axis(rows[np.arange(2)[:, None, None], np.minimum(spx, S - 1)], np.minimum(got, C - 1)[..., None], axis=3)[..., 0]
    assert 0.05 < (picked[mask] == 0).mean() < 0.95                             # the all-negative quirk is exercised, and not alone
    # map mode
    inner = np.random.RandomState(2).randint(0, 256, size=mask.shape).astype(np.int64)
    got = ops.candidate_pseudo_labels(zt, (Ho, Wo), c(mask), inner=c(inner)).cpu().numpy()
    assert np.array_equal(got, np.where(mask, inner, 255)) and np.array_equal(got, CR.labels(zq, Ho, Wo, mask, inner=inner))


@pytest.fixture(scope="module")
def fallback_case():
    h, w, Ho, Wo, C, S = 32, 64, 128, 256, 20, 64
    rs = np.random.RandomState(4)
    zq = (3.0 * rs.randn(2, C, h, w)).astype(np.float32)
    spx = rs.randint(0, S, size=(2, Ho, Wo)).astype(np.int64)
    rows = (rs.uniform(size=(2, S, C)) < 0.15).astype(np.uint8)
    mask = np.isin(spx, rs.choice(S, S // 4, replace=False))
    return types.SimpleNamespace(zq=zq, spx=spx, rows=rows, mask=mask, size=(Ho, Wo), kept={}, up64=None)


@pytest.mark.parametrize("ce_temp", [1.0, 0.1])
@pytest.mark.parametrize("th", [0.0, 0.1, 0.6])
def test_fallback_equals_the_restatement_and_float64_away_from_the_threshold(fallback_case, th, ce_temp):
    ops = _gpu()
    f = fallback_case
    Ho, Wo = f.size
    zt = c(f.zq)
    got = ops.candidate_pseudo_labels(zt, f.size, c(f.mask), targets_rows=c(f.rows), superpixels=c(f.spx), fallback=True, th=th,
                                      ce_temp=ce_temp).cpu().numpy()
    inv_T = CR.inv_temperature(ce_temp)
    assert float(inv_T) == ops.inv_temperature(ce_temp)
    assert np.array_equal(got, CR.labels(f.zq, Ho, Wo, f.mask, rows=f.rows, spx=f.spx, fallback=True, th=th, inv_T=inv_T))
    if f.up64 is None:
        f.up64 = ops.upsample_bilinear(zt, f.size).double().cpu().numpy()
    p = CR.pmax64(f.up64, float(inv_T))
    unq = ~f.mask
    far = unq & (np.abs(p - th) > MARGIN)
    assert (unq & ~far).mean() <= SET_ASIDE
    assert np.array_equal(got[far] != 255, p[far] > th)
    kept = unq & (got != 255)
    assert np.array_equal(got[kept], np.argmax(f.up64, axis=1)[kept])
    assert np.array_equal(got[f.mask], CR.candidate_argmax(f.up64.astype(np.float32), f.rows, f.spx)[f.mask])
    if th == 0.0:
        assert kept.sum() == unq.sum()                   # "fallback on" is a property of the generator, not of th > 0
    f.kept[(th, ce_temp)] = kept.sum() / unq.sum()
    if len(f.kept) == 6:                                 # (not vacuous: some setting keeps a part of the unqueried pixels)
        assert any(0.01 < v < 0.99 for v in f.kept.values()), f.kept


@pytest.fixture(scope="module")
def g12():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_stage2_variants.npz"))
    feats, z, tgt, spx, msk, labels = stage2_inputs(int(g['seed']), int(g['N']), int(g['C']), int(g['Ch']), int(g['H']), int(g['W']), int(g['S']))
    assert digest(feats, z, tgt, spx, msk) == g['input_digest']
    return types.SimpleNamespace(g=g, feats=feats, z=z, tgt=tgt, spx=spx, msk=msk, labels=labels, settings=[tuple(s) for s in g['settings']])


def _assert_g12(got, want, g12, th=None, T=None):
    far = np.ones(want.shape, dtype=bool)
    if th is not None:
        far = g12.msk | (np.abs(CR.pmax64(g12.z, float(CR.inv_temperature(T))) - th) > MARGIN)
    assert (~far).mean() <= SET_ASIDE and np.array_equal(got[far], want.astype(np.int64)[far])


def test_kernels_on_the_g12_inputs_equal_the_executed_reference(g12):
    """All four generators' compositions at identity geometry, with the counters as the table strings the reference returned."""
    ops = _gpu()
    g, K = g12.g, 20
    zt, mt, labels = c(g12.z), c(g12.msk), c(g12.labels)
    inner = ops.stage2_pseudo_labels(c(g12.feats), zt, c(g12.tgt), mt, c(g12.spx), include_onehot=True, expand=False)
    assert inner.dtype == torch.int64 and np.array_equal(inner.cpu().numpy(), g['plbl_cosplbl'].astype(np.int64))
    size = g12.z.shape[2:]

    def run(key, th=None, T=None, **kw):
        counts = torch.zeros(3 * K + 3, dtype=torch.int64, device='cuda')
        got = ops.candidate_pseudo_labels(zt, size, mt, fallback=th is not None, th=th or 0.0, ce_temp=T or 1.0, targets=labels, counts=counts,
                                          num_classes=K, **kw).cpu().numpy()
        _assert_g12(got, g['plbl_' + key], g12, th, T)
        assert np.array_equal(counts.cpu().numpy(), CR.meaniou_counts(got, g12.labels, K))
        if np.array_equal(got, g['plbl_' + key].astype(np.int64)):          # (always, unless a pixel lies within the margin)
            assert CR.iou_table(counts.cpu().numpy(), K) == str(g['table_' + key])
    run('candidate', targets_rows=c(g12.tgt), superpixels=c(g12.spx))
    for k, (th, T) in enumerate(g12.settings):
        run('candprop_%d' % k, th, T, targets_rows=c(g12.tgt), superpixels=c(g12.spx))
        run('naiveprop_%d' % k, th, T, inner=inner)


def test_assignment_without_expansion_equals_the_oracle_under_the_mask():
    """stage2_pseudo_labels(expand=False, include_onehot=True) == where(mask, stage2(expand=True, include_onehot=True), 255) on
    quarter-resolution features.  (With include_onehot=False the identity does not hold: the expanding generator also labels selected
    one-hot pixels by propagation -- 60 of 347 on the G6 inputs of the executed reference -- so that variant has no oracle here.)"""
    ops = _gpu()
    from oracle import exact
    N, C, Ch, Hp, Wp, S = 1, 20, 32, 64, 96, 48
    feats_full, z, tgt, spx, msk, _ = stage2_inputs(29, N, C, Ch, Hp, Wp, S)
    msk = np.isin(spx, np.random.RandomState(29).choice(S, S // 5, replace=False))      # (N = 1: stage2_inputs selects nothing in the last picture)
    q = torch.nn.functional.normalize(torch.nn.functional.avg_pool2d(torch.from_numpy(feats_full), 4)).numpy()
    got = ops.stage2_pseudo_labels(c(q), c(z), c(tgt), c(msk), c(spx), include_onehot=True, expand=False).cpu().numpy()
    want = np.where(msk, exact.stage2_pseudo_labels(q, z, tgt, msk, spx, True), 255)
    assert np.array_equal(got, want) and (got[msk] != 255).all() and msk.any() and not msk.all()
    full = ops.stage2_pseudo_labels(c(q), c(z), c(tgt), c(msk), c(spx), include_onehot=True).cpu().numpy()       # the default still expands
    assert np.array_equal(np.where(msk, full, 255), got) and (full[~msk] != 255).any()
    empty = np.zeros_like(msk)
    assert (ops.stage2_pseudo_labels(c(q), c(z), c(tgt), c(empty), c(spx), expand=False) == 255).all()


@pytest.mark.parametrize("geom", [(33, 41, 129, 161), (32, 64, 32, 64)])
def test_counters_equal_the_counting_of_the_returned_labels(geom):
    ops = _gpu()
    h, w, Ho, Wo = geom
    K = 20
    zq, spx, rows, mask, _ = _picture(11, 2, 20, 64, h, w, Ho, Wo)
    rs = np.random.RandomState(6)
    t = rs.randint(0, 19, size=mask.shape).astype(np.int64)
    t[rs.uniform(size=t.shape) < 0.1] = 255
    t[0, :2, :5] = 25                                           # outside [0, K): seen nowhere, the prediction still counts
    tt = c(t)
    init = torch.arange(3 * K + 3, dtype=torch.int64, device='cuda') * 1000 + 7
    runs = []
    for _ in range(2):
        counts = init.clone()
        got = ops.candidate_pseudo_labels(c(zq), (Ho, Wo), c(mask), targets_rows=c(rows), superpixels=c(spx), fallback=True, th=0.2,
                                          targets=tt, counts=counts, num_classes=K, ignore_label=255)
        runs.append((got, counts))
    (got, counts), (got2, counts2) = runs
    assert torch.equal(got, got2) and torch.equal(counts, counts2)
    want = ops._meaniou_counts_aten(got, tt, K, 255, init.clone())
    assert torch.equal(counts, want)
    delta = (counts - init).cpu().numpy()
    assert np.array_equal(delta, CR.meaniou_counts(got.cpu().numpy(), t, K)) and delta[:K].sum() == ((t != 255) & (t < K)).sum()
    assert (delta[3 * K:] == 0).all() and delta[2 * K:3 * K].sum() > 0
    plain = ops.candidate_pseudo_labels(c(zq), (Ho, Wo), c(mask), targets_rows=c(rows), superpixels=c(spx), fallback=True, th=0.2)
    assert torch.equal(plain, got)                              # counting changes no label


def test_refusals():
    ops = _gpu()
    from mulactseg_amd import _lib
    z = torch.zeros((1, 20, 64, 64), device='cuda')
    f = ops.candidate_pseudo_labels

    def maps(Hh, Ww):
        return torch.ones((1, Hh, Ww), dtype=torch.bool, device='cuda'), torch.zeros((1, Hh, Ww), dtype=torch.int64, device='cuda')
    rows = torch.ones((1, 4, 20), dtype=torch.uint8, device='cuda')
    m, spx = maps(32, 32)
    with pytest.raises(ValueError, match="cannot be upsampled"):
        f(z, (32, 32), m, inner=spx)                                                 # a downsampling
    m7, spx7 = maps(64, 7 * 64)
    with pytest.raises(ValueError, match="cannot be upsampled"):
        f(z, (64, 7 * 64), m7, inner=spx7)                                           # wider than x6
    m2, spx2 = maps(128, 128)
    with pytest.raises(ValueError, match="at most 32"):
        f(torch.zeros((1, 33, 64, 64), device='cuda'), (128, 128), m2, targets_rows=torch.ones((1, 4, 33), dtype=torch.uint8, device='cuda'),
          superpixels=spx2)
    with pytest.raises(ValueError, match="exactly one"):
        f(z, (128, 128), m2, targets_rows=rows, superpixels=spx2, inner=spx2)
    with pytest.raises(ValueError, match="exactly one"):
        f(z, (128, 128), m2)
    # the raw entry point: a non-zero status, and nothing is launched (the output keeps its bytes)
    lib = _lib.load()
    bits = ops.target_bits(rows)
    z33 = torch.zeros((1, 33, 64, 64), device='cuda')

    def raw(zz, C, Ho, Wo, mk, sp, bt, inn, out):
        return lib.mas_candidate_plbl(zz.data_ptr(), 1, C, 64, 64, Ho, Wo, mk.view(torch.uint8).data_ptr(), sp.data_ptr() if sp is not None else None,
                                      bt.data_ptr() if bt is not None else None, 4, inn.data_ptr() if inn is not None else None, 0, 0.0, 1.0,
                                      None, 0, 255, None, out.data_ptr(), None)
    for zz, C, (Ho, Wo), (mk, sp), mode in ((z, 20, (32, 32), (m, spx), 'map'), (z, 20, (64, 448), (m7, spx7), 'map'),
                                            (z33, 33, (128, 128), (m2, spx2), 'cand'), (z, 20, (128, 128), (m2, spx2), 'both'),
                                            (z, 20, (128, 128), (m2, spx2), 'neither')):
        out = torch.full((1, Ho, Wo), 7, dtype=torch.uint8, device='cuda')
        status = raw(zz, C, Ho, Wo, mk, sp if mode in ('cand', 'both') else None, bits if mode in ('cand', 'both') else None,
                     sp if mode in ('map', 'both') else None, out)
        torch.cuda.synchronize()
        assert status != 0 and bool((out == 7).all()), mode
    out = torch.full((1, 128, 128), 7, dtype=torch.uint8, device='cuda')
    assert raw(z, 20, 128, 128, m2, None, None, spx2, out) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# -- the generators end to end ---------------------------------------------------------------------------------------------------
# Pictures of 256 x 512, not the 128 x 256 of test_naive_generator_end_to_end: at 128 x 256 this network's forward is not reproducible
# bit for bit from one call to the next (its stride-16 planes of 8 x 16 take other kernels; differences of 3e-7 in the features), which a
# nearest-prototype assignment between near-equal similarities turns into a pixel or two per picture.  At 256 x 512 it is.
H, W = 256, 512


def _generate(gen, a, datalist, monkeypatch, workers):
    from mulactseg_amd import dataloader
    monkeypatch.setenv("MAS_STAGE2_WORKERS", str(workers))
    aset = dataloader.get_active_dataset(a, train_transform=a.train_transform)
    aset.trg_label_dataset.transform.target = (H, W)          # the pictures at their native size
    aset.selection_iter = 1
    aset.load_datalist(datalist)
    gen.save_dir = None
    return gen.eval(aset, selection_iter=0), aset


def _read_back(tree, run, datalist, ckpt, png_dir, extra):
    """train_stage2_AL.py ... --loader region_cityscapes_plbl: the training set finds the PNGs and a sample is the Pillow pipeline."""
    import random
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


def _composition(name, gen, ops, batch, th, ce_temp):
    """The label map of one sample from the same network: quarter-resolution outputs through ops.upsample_bilinear, then the oracle of
    the assignment and / or the restatement of the label kernel at identity geometry."""
    from oracle import exact
    images = batch['images'].cuda()
    mask, spx, rows = batch['spmask'].cpu().numpy(), batch['spx'].cpu().numpy(), batch['target'].cpu().numpy()
    with torch.no_grad():
        if 'cosplbl' in name:
            feats, zq = gen.net.feat_forward_quarter(images)
        else:
            zq = gen.net(images, lowres=True)
        up = ops.upsample_bilinear(zq.contiguous(), (H, W)).cpu().numpy()
    if 'cosplbl' in name:
        inner = np.where(mask, exact.stage2_pseudo_labels(feats.cpu().numpy(), up, rows, mask, spx, True), 255)
        if name == 'eval_save_cosplbl':
            return inner, up
        return CR.labels(up, H, W, mask, inner=inner, fallback=True, th=th, inv_T=CR.inv_temperature(ce_temp)), up
    return CR.labels(up, H, W, mask, rows=rows, spx=spx, fallback=name.endswith('_prop'), th=th, inv_T=CR.inv_temperature(ce_temp)), up


@pytest.mark.parametrize("name, ptype", [('eval_save_cosplbl', 'wo_expand'), ('eval_save_cosplbl_naiveprop', 'naiveprop'),
                                         ('eval_save_candidateplbl', 'cand'), ('eval_save_candidateplbl_prop', None)])
def test_generator_end_to_end(tmp_path, monkeypatch, capsys, name, ptype):
    ops = _gpu()
    import importlib
    from mulactseg_amd.dataloader.utils import collate_fn
    G = importlib.import_module('mulactseg_amd.trainer.' + name)
    th, ce_temp = 0.1, 0.1
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=3, H=H, W=W, nseg=NSEG)
    run = tmp_path / 'run'
    ckpt = str(run / 'checkpoint01.tar')
    extra = ['--init_checkpoint', ckpt, '--resume_checkpoint', ckpt, '--method', name, '--loader', 'eval_region_cityscapes_all',
             '--train_transform', 'eval_spx', '--trim_multihot_boundary', '--trim_kernel_size', '5', '--plbl_th', str(th), '--ce_temp', str(ce_temp)]
    a = _args(tree, run, extra + (['--plbl_type', ptype] if ptype else []), or_labeling=True)
    datalist = _selected_set(a)
    gen = _generator(G, a, ckpt)
    sub = 'plbl_gen_' + (ptype or 'wcand')
    png_dir = run / sub / 'round_01'
    table, aset = _generate(gen, a, datalist, monkeypatch, 1)
    one = _pngs(png_dir)
    out = capsys.readouterr().out
    assert out.count("[AL 0-round]: evaluation") == 1 and len(table.split(',')) == 1 + 20
    assert sorted(one) == sorted(s + '.png' for s in tree['stems'])
    table4, _ = _generate(gen, a, datalist, monkeypatch, 4)
    four = _pngs(png_dir)
    assert sorted(four) == sorted(one) and all(np.array_equal(one[f], four[f]) for f in one) and table4 == table
    batch = collate_fn([aset.trg_label_dataset[0]])
    want, up = _composition(name, gen, ops, batch, th, ce_temp)
    mask = batch['spmask'].cpu().numpy()
    far = np.ones(mask.shape, dtype=bool)
    if 'prop' in name:
        far = mask | (np.abs(CR.pmax64(up, float(CR.inv_temperature(ce_temp))) - th) > MARGIN)
    png = one[batch['fnames'][0][1].split('/')[-1].split('.')[0] + '.png']
    assert png.dtype == np.uint8 and (~far).mean() <= SET_ASIDE and np.array_equal(png[far[0]], want[0].astype(np.uint8)[far[0]])
    assert (png[mask[0]] != 255).any() and ((png[~mask[0]] != 255).any() == ('prop' in name))
    _read_back(tree, run, datalist, ckpt, png_dir, ['--plbl_type', ptype or 'wcand'])
