"""``--save_vis`` / ``eval_naive_vis`` on the GPU: both kernels of csrc/render.hip byte for byte against the numpy restatement
(tests/render_restated.py); the stage-2 generators with and without ``--save_vis``; ``eval_naive_vis`` on both ``MAS_EVAL_NAIVE``
paths."""
import logging
import os
import tempfile
import types

import numpy as np
import pytest
import torch

import helpers
import render_restated as R
from mulactseg_amd.dataloader.constant import train_id_to_color, voc_id_to_color_map

pytestmark = pytest.mark.gpu
CITY = train_id_to_color.astype(np.uint8)
VOC = voc_id_to_color_map.astype(np.uint8)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _maps(seed, N, H, W, P, fill, nseg):
    """Labels in [0, P) with 255 and the fill index planted; superpixel ids with id 0 and small blobs (plus one INT64_MAX id)."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, P, size=(N, H, W)).astype(np.int64)
    lab[rs.uniform(size=lab.shape) < 0.15] = 255
    lab[rs.uniform(size=lab.shape) < 0.05] = fill
    bh, bw = max(1, H // 7), max(1, W // 9)
    spx = rs.randint(0, nseg, size=(N, (H + bh - 1) // bh, (W + bw - 1) // bw)).astype(np.int64)
    spx = np.repeat(np.repeat(spx, bh, axis=1), bw, axis=2)[:, :H, :W].copy()
    spx[rs.uniform(size=spx.shape) < 0.02] = rs.randint(0, nseg)            # single-pixel specks
    spx[0, : H // 3, : W // 4] = 0                                          # a block of the background id
    spx[-1, H // 2:, W // 2:] = np.iinfo(np.int64).max
    return lab, spx


SHAPES = [(1, 5, 6), (2, 33, 47), (3, 64, 128), (1, 1, 9), (2, 7, 1), (1, 129, 257)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("palette,fill", [(CITY, 20), (VOC, 21)])
@pytest.mark.parametrize("marks", [False, True])
def test_render_labels_equals_the_restatement(shape, dtype, palette, fill, marks):
    ops = _gpu()
    N, H, W = shape
    lab, spx = _maps(N * 1000 + H * 7 + W + fill + int(marks), N, H, W, len(palette), fill, 6)
    pal = torch.from_numpy(palette).cuda()
    lt = torch.from_numpy(lab).to(dtype).cuda()
    got = ops.render_labels(lt, pal, fill, torch.from_numpy(spx).cuda() if marks else None)
    want = R.render_labels(lab, palette, fill, spx if marks else None)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, H, W, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    if marks and H * W > 100:
        assert (want == (255, 255, 0)).all(-1).any()


def test_render_labels_at_full_size_and_on_a_slice():
    ops = _gpu()
    lab, spx = _maps(5, 2, 1024, 2048, 21, 20, 2048)
    pal = torch.from_numpy(CITY).cuda()
    lt, st = torch.from_numpy(lab).cuda(), torch.from_numpy(spx).cuda()
    got = ops.render_labels(lt, pal, 20, st)
    assert np.array_equal(got.cpu().numpy(), R.render_labels(lab, CITY, 20, spx))
    one = ops.render_labels(lt[1:], pal, 20, st[1:])                        # (a picture of a batch: an offset view)
    assert torch.equal(one, got[1:])


def test_a_label_outside_the_palette_raises():
    ops = _gpu()
    from mulactseg_amd import _lib
    pal = torch.from_numpy(CITY).cuda()
    lab = torch.zeros((1, 8, 8), dtype=torch.int64, device='cuda')
    lab[0, 3, 4] = 21
    lab[0, 5, 5] = -1
    with pytest.raises(_lib.MulActSegHipError, match="2 label"):
        ops.render_labels(lab, pal, 20)
    with pytest.raises(ValueError, match="fill"):
        ops.render_labels(lab, pal, 21)
    with pytest.raises(TypeError):
        ops.render_labels(lab.int(), pal, 20)


GEOMS = [(256, 512, 1024, 2048), (33, 65, 129, 257), (48, 80, 48, 80), (16, 24, 61, 97)]


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("CH,palette", [(20, CITY), (21, VOC)])
@pytest.mark.parametrize("N", [1, 3])
def test_render_lowres_pred_equals_the_materialised_argmax(geom, CH, palette, N):
    ops = _gpu()
    h, w, H, W = geom
    rs = np.random.RandomState(h + w + CH + N)
    zq = (2.0 * rs.randn(N, CH, h, w)).astype(np.float32)
    zq[:, 3, : h // 3] += 6.0
    zq[:, 5, : h // 3] = zq[:, 3, : h // 3]                                 # exact ties: the first channel wins
    zq[:, CH - 1] += 20.0                                                   # the last channel is never a candidate
    zq[0, 0, h - 2, w // 3] = np.nan
    zq[-1, 7, h // 2, w - 1] = np.nan
    zt = torch.from_numpy(zq).cuda()
    pal = torch.from_numpy(palette).cuda()
    got = ops.render_lowres_pred(zt, (H, W), pal)
    up = zt if (h, w) == (H, W) else ops.upsample_bilinear(zt, (H, W))
    want = pal[up[:, :-1].max(dim=1)[1]]
    assert tuple(got.shape) == (N, H, W, 3) and torch.equal(got, want)
    assert torch.isnan(up).any()
    if N * H * W <= 200_000:
        assert np.array_equal(got.cpu().numpy(), R.render_pred(up.cpu().numpy(), palette))


def test_render_lowres_pred_refuses_what_naive_plbl_refuses():
    ops = _gpu()
    pal = torch.from_numpy(CITY).cuda()
    with pytest.raises(ValueError):
        ops.render_lowres_pred(torch.zeros((1, 20, 64, 64), device='cuda'), (32, 32), pal)
    with pytest.raises(ValueError):
        ops.render_lowres_pred(torch.zeros((1, 30, 8, 8), device='cuda'), (32, 32), pal)   # 29 classes, 21 colours


# -- the stage-2 generators -------------------------------------------------------------------------------------------------------
def _samples(C, H, W, S, n, dev):
    from mulactseg_amd import synth
    g = torch.Generator(device=dev).manual_seed(4)
    rs = np.random.RandomState(5)
    out = []
    for i in range(n):
        spx = torch.from_numpy(synth.superpixel_map(70 + i, H, W, S)[None]).to(dev)
        trg = (rs.rand(1, S, C + 1) < 0.15).astype(np.uint8)
        trg[..., C] = 0
        trg[0, rs.rand(S) >= 0.4] = 0
        trg = torch.from_numpy(trg).to(dev)
        msk = (trg.sum(-1) > 0)[0][spx[0].long()][None]
        out.append({'images': torch.randn((1, 3, H, W), generator=g, device=dev), 'spx': spx, 'spmask': msk, 'target': trg,
                    'labels': torch.from_numpy(rs.randint(0, C, size=(1, H, W))).to(dev),
                    'fnames': [["i/p%03d.png" % i, "l/p%03d.png" % i, "s/p%03d.pkl" % i]]})
    return out


class _Loader:
    def __init__(self, samples):
        self.samples, self.k = samples, 0

    def __len__(self):
        return len(self.samples)

    def __next__(self):
        self.k += 1
        return self.samples[self.k - 1]


def _files(d):
    from PIL import Image
    return {f: np.array(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d))}


def _run_generator(mod, net, samples, C, workers, save_vis, capsys):
    tmp = tempfile.mkdtemp(prefix="mas_vis_")
    tr = object.__new__(mod.ActiveTrainer)
    tr.args = types.SimpleNamespace(ignore_idx=255, init_checkpoint=os.path.join(tmp, "checkpoint01.tar"), plbl_type=None,
                                    val_batch_size=1, save_vis=save_vis, nseg=64)
    tr.net, tr.device, tr.num_classes, tr.selection_iter, tr.save_dir = net, torch.device('cuda:0'), C, 1, None
    if hasattr(mod.ActiveTrainer, 'crop_size'):
        tr.crop_size = 128
    os.environ["MAS_STAGE2_WORKERS"] = str(workers)
    try:
        capsys.readouterr()
        _, table = tr.inference(_Loader(samples))
        out = capsys.readouterr().out
    finally:
        os.environ.pop("MAS_STAGE2_WORKERS", None)
    d = tr._save_dir()
    return out, table, _files(d), d + '_vis'


@pytest.mark.parametrize("name", ["eval_save_cosplbl_prop", "eval_save_cosplbl_prop_includeonehot", "eval_save_cosplbl_prop_onehotignore",
                                  "eval_save_cosplbl_prop_includeonehot_slide", "eval_save_cosplbl_prop_includeonehot_voc"])
def test_generators_write_the_vis_pictures_of_their_labels(name, capsys):
    _gpu()
    import importlib
    from mulactseg_amd.models import get_model
    mod = importlib.import_module("mulactseg_amd.trainer." + name)
    voc = name.endswith('_voc')
    C = 21 if voc else 19
    dev = torch.device('cuda:0')
    H, W, S = 256, 512, 48
    torch.manual_seed(2)
    net = get_model('deeplabv3pluswn_resnet50deepstem', C + (0 if voc else 1), 16, True, pretrained_backbone=False).to(dev).eval()
    samples = _samples(C, H, W, S, 5, dev)
    if voc:
        for s in samples:
            s['target'] = s['target'][..., :C].contiguous()
    if name.endswith('_onehotignore'):                  # (dominant-label queries: a per-pixel target map, 255 outside the mask)
        for s in samples:
            s['target'] = torch.where(s['spmask'], s['labels'], torch.full_like(s['labels'], 255))
    slide = name.endswith('_slide')
    same = lambda x, y: x[:2] == y[:2] and sorted(x[2]) == sorted(y[2]) and all(np.array_equal(x[2][f], y[2][f]) for f in x[2])
    if not slide:
        # The network's forward is not always bit-reproducible from one run to the next on these small pictures.  Every run
        # reuses the features of the first one, so the runs can be compared.
        cache, forward = {}, net.feat_forward_lowres

        def cached(images):
            key = images.data_ptr()
            if key not in cache:
                cache[key] = tuple(t.clone() for t in forward(images))
            return cache[key]
        net.feat_forward_lowres = cached
    try:
        _run_generator(mod, net, samples, C, 1, False, capsys)         # (fills the cache, one picture at a time)
        ref = _run_generator(mod, net, samples, C, 1, False, capsys)
        assert not os.path.exists(ref[3])
        for workers in ((1,) if slide else (1, 4)):
            out, table, pngs, vis_dir = _run_generator(mod, net, samples, C, workers, True, capsys)
            assert sorted(pngs) == sorted(ref[2]) and len(table.split(',')) == len(ref[1].split(','))
            if not slide:                  # (the sliding-window forward is not cached: its runs are not compared)
                assert same((out, table, pngs), ref)
            vis = _files(vis_dir)
            assert sorted(vis) == sorted(pngs) and len(vis) == len(samples)
            pal, fill = (VOC, 21) if voc else (CITY, 20)
            for s in samples:
                f = s['fnames'][0][1].split('/')[-1]
                want = R.render_labels(pngs[f][None], pal, fill, s['spx'].cpu().numpy().astype(np.int64))[0]
                assert vis[f].shape == (H, W, 3) and np.array_equal(vis[f], want)
            assert any((v == (255, 255, 0)).all(-1).any() for v in vis.values())
    finally:
        if not slide:
            del net.feat_forward_lowres


def test_the_ms_generator_writes_the_vis_pictures(tmp_path, monkeypatch, capsys):
    """eval_save_cosplbl_prop_includeonehot_voc_ms with --save_vis on a VOC tree: the vis picture of every label PNG, at the picture's
    own size; no vis directory without the flag.  (The ten-scale forward is not bit-reproducible from one run to the next, so the
    label PNGs of the two runs are not compared here: the single-forward generators above show that the flag leaves them alone.)"""
    _gpu()
    import test_ms_ensemble_gpu as MS
    from mulactseg_amd import dataloader
    from mulactseg_amd.dataloader.utils import collate_fn
    tree = helpers.write_voc_tree(str(tmp_path / 'voc'), n=2, sizes=((261, 341), (303, 265)))
    run = tmp_path / 'run'
    ckpt = str(run / 'checkpoint01.tar')
    a, aset = MS._ms_set(tree, run, ['--init_checkpoint', ckpt])
    MS._select_all(aset)
    aset.dump_datalist()
    datalist = os.path.join(a.model_save_dir, 'datalist_01.pkl')
    gen = MS._generator(a, ckpt)
    monkeypatch.delenv("MAS_MS_ENSEMBLE", raising=False)
    png_dir = run / 'plbl_gen_ms' / 'round_01'
    for save_vis in (False, True):
        gen.args.save_vis = save_vis
        gen.save_dir = None
        set2 = dataloader.get_active_dataset(a, train_transform=a.train_transform)
        set2.selection_iter = 1
        set2.load_datalist(datalist)
        table = gen.eval(set2, selection_iter=0)
        assert len(table.split(',')) == 1 + 22
        assert os.path.exists(str(png_dir) + '_vis') == save_vis
    pngs = _files(str(png_dir))
    vis = _files(str(png_dir) + '_vis')
    assert sorted(vis) == sorted(pngs) and len(vis) == 2
    ds = set2.trg_label_dataset
    for idx in range(len(ds.im_idx)):
        batch = collate_fn([ds[idx]])
        f = batch['fnames'][0][1].split('/')[-1].split('.')[0] + '.png'
        assert vis[f].shape == pngs[f].shape + (3,)
        want = R.render_labels(pngs[f][None], VOC, 21, batch['spx'].cpu().numpy().astype(np.int64))[0]
        assert np.array_equal(vis[f], want)


# -- eval_naive_vis -----------------------------------------------------------------------------------------------------------------
def test_eval_naive_vis_writes_the_pictures_and_the_table_of_eval_naive(tmp_path, monkeypatch, capsys):
    _gpu()
    import test_eval_naive_gpu as EN
    from PIL import Image
    from mulactseg_amd import dataloader, ops
    from mulactseg_amd.trainer import eval_naive, eval_naive_vis
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=2, H=128, W=256, nseg=64)
    run = tmp_path / 'run'
    ckpt = str(run / 'stage2_checkpoint03.tar')
    a = EN._eval_args(tree, run, ckpt)
    EN._seeded_checkpoint(a, ckpt)
    monkeypatch.chdir(tmp_path)

    def go(mod, path, save_vis):
        monkeypatch.setenv("MAS_EVAL_NAIVE", path)
        a.save_vis = save_vis
        dataloader.register_dataset_factory(None)
        active_set = dataloader.get_active_dataset(a, train_transform=a.train_transform)
        tr = mod.ActiveTrainer(a, logging.getLogger("test"), 0)
        tr.load_checkpoint(ckpt)
        capsys.readouterr()
        table = tr.eval(active_set, selection_iter=0)
        return tr, table, capsys.readouterr().out

    _, want_table, want_out = go(eval_naive, "lowres", False)
    vis = tmp_path / 'vis' / 'neurips23_supp_qual'
    assert not vis.exists()
    tr, table, out = go(eval_naive_vis, "lowres", False)
    assert table == want_table and out == want_out
    pred = _files(str(vis / 'round_03'))
    assert len(pred) == 2 and os.listdir(str(vis / 'gt')) == []
    # the pictures: palette[first arg-max of the upsampled class channels] of the first picture of each batch
    ds = dataloader.get_dataset(a, name=a.val_dataset, data_root=a.val_data_dir, datalist=a.val_datalist, imageset='eval')
    loader = tr.get_valloader(ds)
    want_pred, want_gt = {}, {}
    with torch.no_grad():
        for _ in range(len(loader)):
            batch = next(loader)
            f = batch['fnames'][0][1].split('/')[-1].split('.')[0] + '.png'
            z = ops.upsample_bilinear(tr.net(batch['images'].cuda().float(), lowres=True).contiguous(), batch['labels'].shape[-2:])
            want_pred[f] = CITY[z[:1, :-1].max(dim=1)[1][0].cpu().numpy()]
            lab = batch['labels'][0].cpu().numpy()
            want_gt[f] = CITY[np.where(lab == 255, 19, lab)]
    assert sorted(pred) == sorted(want_pred) and all(np.array_equal(pred[f], want_pred[f]) for f in pred)
    # --save_vis adds the ground truth; the full-resolution path writes the same pictures and table
    for path in ("lowres", "full"):
        for d in (vis / 'round_03', vis / 'gt'):
            for f in os.listdir(str(d)):
                os.remove(str(d / f))
        _, table, out = go(eval_naive_vis, path, True)
        assert table == want_table and out == want_out
        pred, gt = _files(str(vis / 'round_03')), _files(str(vis / 'gt'))
        assert sorted(gt) == sorted(want_gt) and all(np.array_equal(gt[f], want_gt[f]) for f in gt)
        assert sorted(pred) == sorted(want_pred)
        if path == "lowres":
            assert all(np.array_equal(pred[f], want_pred[f]) for f in pred)
        else:                        # (net(images) upsamples with F.interpolate: a pixel at an exact tie may differ)
            assert all((pred[f] != want_pred[f]).any(-1).mean() < 1e-3 for f in pred)
