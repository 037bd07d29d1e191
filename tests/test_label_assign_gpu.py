"""The region-label kernels (csrc/labels.hip) and the data-generation command line, bit for bit against the numpy restatement."""
import gzip
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_assign_restated as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# (H, W, nseg, C): Cityscapes, VOC-like squares and both orientations
SHAPES = [(1024, 2048, 2048, 19), (513, 513, 150, 21), (500, 375, 150, 21), (375, 500, 150, 21)]
_CACHE = {}


def _case(shape_i):
    if shape_i not in _CACHE:
        H, W, nseg, C = SHAPES[shape_i]
        spx = R.voronoi(100 + shape_i, H, W, nseg)
        spx[0, :5] = nseg + 3                                   # ids outside [0, nseg): no region, but they make boundaries
        spx[-1, -3:] = -1
        lab = R.labels_for(200 + shape_i, spx, C)
        rs = np.random.RandomState(300 + shape_i)
        present = np.unique(spx[(spx >= 0) & (spx < nseg)])
        ids = [int(i) for i in rs.permutation(present)[: len(present) - 3]]      # three present ids unlisted
        absent = sorted(set(range(nseg)) - set(present.tolist()))
        ids += absent[:1] + ids[:2]                            # a listed id with no pixel, two repeated ids
        _CACHE[shape_i] = (lab, spx, ids, nseg, C)
    return _CACHE[shape_i]


def _ids_as(spx, dtype):
    return spx.astype({'i64': np.int64, 'i32': np.int32, 'u16': np.uint16}[dtype])


@pytest.mark.parametrize("dtype", ['i64', 'i32', 'u16'])
@pytest.mark.parametrize("k", [0, 3, 5])
@pytest.mark.parametrize("shape_i", range(len(SHAPES)))
def test_multi_hot_matches_the_restatement(shape_i, k, dtype):
    from mulactseg_amd import label_assignment as la
    lab, spx, ids, nseg, C = _case(shape_i)
    sp = spx if dtype != 'u16' else np.where(spx < 0, 65535, spx)              # -1 as u16 is 65535: still no region
    want = R.multi_hot(lab, sp, ids, nseg, C, k)
    got = la.assign(lab, _ids_as(sp, dtype), ids, nseg, C, trim_kernel_size=k)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]), "multi-hot bits differ"
    assert np.array_equal(got[1], want[1]), "sizes differ"
    again = la.assign(lab, _ids_as(sp, dtype), ids, nseg, C, trim_kernel_size=k)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("generate_ignore", [False, True])
@pytest.mark.parametrize("shape_i", range(len(SHAPES)))
def test_dominant_matches_the_restatement(shape_i, generate_ignore, sample):
    from mulactseg_amd import label_assignment as la
    lab, spx, ids, nseg, C = _case(shape_i)
    dtype = ['i64', 'i32', 'i64', 'i32'][shape_i]
    want = R.dominant(lab, spx, ids, nseg, C, generate_ignore, R.sample_generator(5) if sample else None)
    got = la.assign(lab, _ids_as(spx, dtype), ids, nseg, C, dominant=True, generate_ignore=generate_ignore,
                    generator=la.sample_generator(5) if sample else None)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    again = la.assign(lab, _ids_as(spx, dtype), ids, nseg, C, dominant=True, generate_ignore=generate_ignore,
                      generator=la.sample_generator(5) if sample else None)
    assert got.tobytes() == again.tobytes()


def test_dominant_u16_ids_and_the_literal_loop():
    from mulactseg_amd import label_assignment as la
    lab, spx, ids, nseg, C = _case(2)
    sp = np.where(spx < 0, 65535, spx)
    for gi in (False, True):
        got = la.assign(lab, sp.astype(np.uint16), ids, nseg, C, dominant=True, generate_ignore=gi)
        assert np.array_equal(got, R.dominant_loop(lab, sp, ids, gi))


def test_int16_ids_as_decode_map_yields_them():
    from mulactseg_amd import label_assignment as la
    lab, spx, ids, nseg, C = _case(1)
    sp = np.clip(spx, 0, nseg + 3)
    got = la.assign(lab, sp.astype(np.int16), ids, nseg, C, trim_kernel_size=5)
    want = R.multi_hot(lab, sp, ids, nseg, C, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_out_of_range_labels_raise():
    from mulactseg_amd import label_assignment as la
    lab, spx, ids, nseg, C = _case(3)
    bad = lab.copy()
    bad[10, 10] = C                                           # the reference folds C into the ignore column; here it is an error
    with pytest.raises(ValueError):
        la.assign(bad, spx, ids, nseg, C, trim_kernel_size=3)
    with pytest.raises(ValueError):
        la.assign(bad, spx, ids, nseg, C, dominant=True)


# ---- end to end: the command line on a synthetic dataset ----------------------------------------------------------------------
def _golden_lines(n):
    with gzip.open(os.path.join(ROOT, 'tests', 'golden', 'cityscapes_train_seed2048_or.txt.gz'), 'rt') as f:
        return [next(f).rstrip('\n') for _ in range(n)]


def _build_dataset(root, n=5, H=96, W=160, nseg=64):
    """labelIds PNGs, {'labels': ...} pickles, a labelIds datalist, its _or twin and a region dict (paths of the golden list)."""
    from PIL import Image
    from mulactseg_amd.dataloader import constant
    raw_of_train = np.zeros(256, dtype=np.uint8)               # train id -> a raw label id; 255 -> 0 (unlabeled)
    for raw in range(constant.N_RAW_IDS):
        t = int(constant.id_to_train_id[raw])
        if t != 255:
            raw_of_train[t] = raw
    lines, or_lines, region, pics = [], [], {}, []
    for i, line in enumerate(_golden_lines(n)):
        img, or_lbl, spx_rel = line.split('\t')
        stem = os.path.basename(spx_rel).split('.')[0]
        city = stem.split('_')[0]
        lbl_rel = 'gtFine/train/%s/%s_gtFine_labelIds.png' % (city, stem)
        spx = R.voronoi(40 + i, H, W, nseg)
        lab = R.labels_for(60 + i, spx, 19)
        os.makedirs(os.path.dirname(os.path.join(root, lbl_rel)), exist_ok=True)
        os.makedirs(os.path.dirname(os.path.join(root, spx_rel)), exist_ok=True)
        Image.fromarray(raw_of_train[lab]).save(os.path.join(root, lbl_rel))
        with open(os.path.join(root, spx_rel), 'wb') as f:
            pickle.dump({'labels': spx.astype(np.int32)}, f)
        present = np.unique(spx).tolist()
        missing = [j for j in range(nseg) if j not in present][:2] + [3 + i]
        region[spx_rel] = [nseg, sorted(set(missing))]
        ids = [j for j in range(nseg) if j not in set(missing)]
        lines.append('\t'.join([img, lbl_rel, spx_rel]))
        or_lines.append(line)
        pics.append((img, lab, spx, ids))
    lists = os.path.join(root, 'lists')
    os.makedirs(lists)
    paths = {k: os.path.join(lists, v) for k, v in (('list', 'train.txt'), ('or', 'train_or.txt'), ('dict', 'train.dict'),
                                                   ('dom', 'train_dominant.txt'))}
    with open(paths['list'], 'w') as f:
        f.write('\n'.join(lines) + '\n')
    with open(paths['or'], 'w') as f:
        f.write('\n'.join(or_lines) + '\n')
    with open(paths['dom'], 'w') as f:
        f.write('\n'.join(l.replace('gtFine_or', 'gtFine_dominant').replace('.npy', '.png') for l in or_lines) + '\n')
    with open(paths['dict'], 'w') as f:
        json.dump(region, f)
    return pics, paths


def _cli(args, timeout=300):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', 'mulactseg_amd.label_assignment'] + args, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_end_to_end(tmp_path):
    import argparse
    import torch
    from PIL import Image
    from mulactseg_amd.dataloader import formats
    from mulactseg_amd.dataloader.picture_store import decode_map
    from mulactseg_amd.dataloader.region_cityscapes_or_tensor import RegionCityscapesOr
    nseg, C, root = 64, 19, str(tmp_path / 'data')
    pics, paths = _build_dataset(root, nseg=nseg)
    common = ['--nseg', str(nseg), '--spx_method', 'seeds', '--trg_data_dir', root, '--trg_datalist', paths['list'],
              '--region_dict', paths['dict'], '--num_worker', '3']
    out = _cli(['multi_hot'] + common + ['--trim_multihot_boundary', '--trim_kernel_size', '5'])
    assert 'pictures' in out
    save = os.path.join(root, 'superpixel_seed/cityscapes/seeds_%d/train/gtFine_multi_tensor_trim_5x5' % nseg)
    cls, size = np.load(os.path.join(save, 'multi_hot_cls.npy')), np.load(os.path.join(save, 'sp_size.npy'))
    assert cls.dtype == np.uint8 and cls.shape == (len(pics), nseg, C + 1)
    assert size.dtype == np.int64 and size.shape == (len(pics), nseg)
    for i, (_, lab, spx, ids) in enumerate(pics):
        w = R.multi_hot(lab, spx, ids, nseg, C, 5)
        assert cls[i].tobytes() == w[0].tobytes() and size[i].tobytes() == w[1].tobytes()
    # the stage-1 loader reads them back: the row of each sample is the restated one
    args = argparse.Namespace(nseg=nseg, spx_method='seeds', trim_multihot_boundary=True, trim_kernel_size=5, trg_datalist=paths['or'],
                              ignore_size=0, mark_topk=-1, prob_dominant=False)
    ds = RegionCityscapesOr(args, root, paths['or'], split='active-ulabel', transform=lambda *a: a, region_dict=paths['dict'])
    for i, (_, lab, spx, ids) in enumerate(pics):
        row = ds.multi_hot_row(ds.im_idx[i][1], torch.device('cuda'))
        assert np.array_equal(row.cpu().numpy(), R.multi_hot(lab, spx, ids, nseg, C, 5)[0])

    # dominant maps, the _sample draw under a fixed seed, with ignore generated (the published configuration)
    _cli(['dominant'] + common + ['--generate_ignore', '--loader', 'region_cityscapes_dominant_all_sample', '--seed', '3',
                                  '--nvis_color', '2'])
    ddir = os.path.join(root, 'superpixel_seed/cityscapes/seeds_%d/train/gtFine_dominant_ignore_sample' % nseg)
    g = R.sample_generator(3)
    for i, (img, lab, spx, ids) in enumerate(pics):
        want = R.dominant(lab, spx, ids, nseg, C, True, g)
        stem = '_'.join(os.path.basename(img).split('_')[:3])
        with Image.open(os.path.join(ddir, stem + '.png')) as im:
            assert im.mode == 'I;16'
            assert np.array_equal(np.array(im), want.astype(np.uint16))
        assert os.path.exists(os.path.join(ddir.replace('gtFine', 'gtColor'), stem + '.png')) == (i < 2)
    # argmax maps without ignore, read back through the dominant datalist (known_ignore: the gtFine_dominant paths)
    _cli(['dominant'] + common)
    im_idx, _ = formats.read_datalist(paths['dom'], root, paths['dict'], known_ignore=True)
    for i, (img, lab, spx, ids) in enumerate(pics):
        got = decode_map(im_idx[i][1].replace('seeds_2048', 'seeds_%d' % nseg))         # the golden paths name seeds_2048
        assert np.array_equal(got, R.dominant(lab, spx, ids, nseg, C, False))
