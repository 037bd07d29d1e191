"""The data-generation step without a GPU: the numpy restatement against the reference's per-id loop and scipy, hand-checked cases,
the command line's arguments and output paths, and argument errors of the C entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_assign_restated as R  # noqa: E402


def _small(seed, H=23, W=31, nseg=12, C=5):
    rs = np.random.RandomState(seed)
    spx = rs.randint(-1, nseg + 2, (H // 4 + 1, W // 4 + 1)).repeat(4, 0).repeat(4, 1)[:H, :W]
    spx = np.where(rs.uniform(size=(H, W)) < 0.05, rs.randint(0, nseg, (H, W)), spx)
    lab = rs.randint(0, C, (H, W))
    lab = np.where(rs.uniform(size=(H, W)) < 0.15, 255, lab).astype(np.uint8)
    ids = list(rs.permutation(nseg)[:nseg - 2]) + [int(rs.randint(0, nseg))]        # a missing id or two, a repeated one
    return lab, spx, ids, nseg, C


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("k", [0, 1, 3, 5])
def test_vectorised_multi_hot_equals_the_per_id_loop(seed, k):
    lab, spx, ids, nseg, C = _small(seed)
    a, b = R.multi_hot(lab, spx, ids, nseg, C, k), R.multi_hot_loop(lab, spx, ids, nseg, C, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("generate_ignore", [False, True])
def test_vectorised_dominant_equals_the_per_id_loop(seed, generate_ignore):
    lab, spx, ids, nseg, C = _small(seed)
    assert np.array_equal(R.dominant(lab, spx, ids, nseg, C, generate_ignore), R.dominant_loop(lab, spx, ids, generate_ignore))


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("generate_ignore", [False, True])
def test_sample_replay_equals_the_per_id_loop(seed, generate_ignore):
    lab, spx, ids, nseg, C = _small(seed)
    a = R.dominant(lab, spx, ids, nseg, C, generate_ignore, R.sample_generator(7))
    b = R.dominant_loop(lab, spx, ids, generate_ignore, R.sample_generator(7))
    assert np.array_equal(a, b)


def test_library_draw_equals_the_restated_draw():
    """label_assignment.multinomial_draw (what the CLI hands the kernels) consumes the generator as the reference loop does."""
    from mulactseg_amd import label_assignment as la
    lab, spx, ids, nseg, C = _small(3)
    full = R.histograms(lab, spx, nseg, C)
    for gi in (False, True):
        drawn = la.multinomial_draw(full, ids, C, gi, la.sample_generator(11))
        val = np.where(drawn == C, 255, drawn)
        sp = spx.astype(np.int64)
        ok = (sp >= 0) & (sp < nseg)
        v = np.where(ok, val[np.clip(sp, 0, nseg - 1)], -1)
        painted = np.where((v >= 0) & (gi | (lab != 255)), v, lab).astype(np.uint8)
        assert np.array_equal(painted, R.dominant_loop(lab, spx, ids, gi, R.sample_generator(11)))


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_boundary_and_dilation_equal_scipy(seed, k):
    ndimage = pytest.importorskip("scipy.ndimage")
    _, spx, _, _, _ = _small(seed, H=29, W=37)
    cross = ndimage.generate_binary_structure(2, 1)
    want = ndimage.grey_dilation(spx, footprint=cross, mode='reflect') != ndimage.grey_erosion(spx, footprint=cross, mode='reflect')
    b = R.thick_boundary(spx)
    assert np.array_equal(b, want)
    assert np.array_equal(R.dilate(b, k), ndimage.binary_dilation(b, structure=np.ones((k, k), np.uint8), border_value=0))


def test_hand_checked_multi_hot_cases():
    C, nseg = 4, 8
    spx = np.zeros((8, 12), dtype=np.int64)
    spx[:, 6:] = 1
    spx[3, 2] = 2                          # id 2: one pixel inside id 0 -- entirely inside the trimmed band (fallback)
    spx[0:2, 10:12] = 3                    # id 3: all-ignore region
    spx[7, 0] = 9                          # id 9 >= nseg: no region
    lab = np.full((8, 12), 1, dtype=np.uint8)
    lab[:, 6:] = 2
    lab[3, 2] = 3
    lab[0:2, 10:12] = 255
    lab[7, 0] = 0
    ids = [0, 1, 2, 3, 5]                  # 5: listed, absent; 4, 6, 7: unlisted
    for k in (0, 3):
        cls, size = R.multi_hot(lab, spx, ids, nseg, C, k)
        assert np.array_equal(cls, R.multi_hot_loop(lab, spx, ids, nseg, C, k)[0])
        assert cls[2].tolist() == [0, 0, 0, 1, 0] and size[2] == 1              # fallback to the untrimmed region
        assert cls[3].tolist() == [0, 0, 0, 0, 1] and size[3] == 4              # only the ignore column
        assert cls[5].tolist() == [0] * 5 and size[5] == 0
        assert cls[4].tolist() == [0] * 5 and size[4] == -1 and size[6] == -1
        assert cls[0].tolist() == [0, 1, 0, 0, 0]                               # the id-2 and id-9 pixels are not id 0's
    _, size0 = R.multi_hot(lab, spx, ids, nseg, C, 0)
    assert size0[0] == 8 * 6 - 2           # id 2's pixel and the id-9 pixel are not id 0


def test_hand_checked_dominant_ties():
    C, nseg = 4, 2
    spx = np.zeros((2, 4), dtype=np.int64)
    spx[:, 2:] = 1
    lab = np.array([[3, 1, 255, 255], [1, 3, 2, 0]], dtype=np.uint8)
    out = R.dominant(lab, spx, [0, 1], nseg, C, False)
    assert out[:, :2].tolist() == [[1, 1], [1, 1]]                              # tie 1 / 3: the smaller value
    assert out[:, 2:].tolist() == [[255, 255], [0, 0]]                          # ignore kept; tie 2 / 0 -> 0
    out = R.dominant(lab, spx, [0, 1], nseg, C, True)
    assert out[:, 2:].tolist() == [[255, 255], [255, 255]]                      # 255 competes: 2 x 255 vs 1 x 2, 1 x 0
    lab2 = lab.copy()
    lab2[1, 3] = 255
    lab2[0, 3] = 2
    out = R.dominant(lab2, spx, [0, 1], nseg, C, True)                          # 255 x2 vs 2 x2: 255 loses the tie
    assert out[:, 2:].tolist() == [[2, 2], [2, 2]]
    assert np.array_equal(out, R.dominant_loop(lab2, spx, [0, 1], True))


def test_out_of_range_labels_are_an_error():
    lab = np.array([[0, 19]], dtype=np.uint8)
    with pytest.raises(ValueError):
        R.multi_hot(lab, np.zeros((1, 2), np.int64), [0], 1, 19)


# ---- the command line -------------------------------------------------------------------------------------------------------
def _args(argv):
    from mulactseg_amd import label_assignment as la
    return la.resolve(la.get_parser().parse_args(argv))


def test_cli_cityscapes_multi_hot_defaults():
    a = _args(['multi_hot', '--trim_multihot_boundary', '--trim_kernel_size', '5', '--ignore_size', '3', '--prob_dominant'])
    assert (a.nseg, a.num_classes, a.num_worker, a.trg_data_dir, a.trim) == (2048, 19, 8, './data/Cityscapes', 5)
    assert a.trg_datalist == 'dataloader/init_data/cityscapes/train_seed2048.txt'
    assert a.region_dict == 'dataloader/init_data/cityscapes/train_seed2048.dict'
    assert a.save_data_dir == './data/Cityscapes/superpixel_seed/cityscapes/seed_2048/train/gtFine_multi_tensor_trim_5x5'
    a = _args(['multi_hot', '--save_data_dir', '/x/y', '--trim_kernel_size', '4'])         # trimming off: k is not looked at
    assert a.save_data_dir == '/x/y' and a.trim == 0


def test_cli_rejects_an_even_trim_kernel():
    with pytest.raises(ValueError):
        _args(['multi_hot', '--trim_multihot_boundary', '--trim_kernel_size', '4'])


def test_cli_cityscapes_dominant_paths():
    from mulactseg_amd import label_assignment as la
    a = _args(['dominant', '--generate_ignore', '--loader', 'region_cityscapes_dominant_all_sample', '--trg_data_dir', '/d'])
    assert a.sample and not a.known_ignore and a.nvis_color == 3000
    assert a.do_data_dir == '/d/superpixel_seed/cityscapes/seed_2048/train/gtFine_dominant_ignore_sample'
    f = la.dominant_file(a, '/d/leftImg8bit/train/aachen/aachen_000000_000019_leftImg8bit.png')
    assert f == a.do_data_dir + '/aachen_000000_000019.png'
    assert la.color_file(f) == '/d/superpixel_seed/cityscapes/seed_2048/train/gtColor_dominant_ignore_sample/aachen_000000_000019.png'
    a = _args(['dominant', '--nseg', '1024', '--spx_method', 'seeds'])
    assert not a.sample and a.known_ignore
    assert a.do_data_dir == './data/Cityscapes/superpixel_seed/cityscapes/seeds_1024/train/gtFine_dominant'
    assert a.trg_datalist == 'dataloader/init_data/cityscapes/train_seeds1024.txt'


def test_cli_voc_paths():
    from mulactseg_amd import label_assignment as la
    a = _args(['dominant', '--dataset', 'voc', '--generate_ignore'])
    assert (a.nseg, a.num_classes, a.trg_data_dir) == (150, 21, './data/VOCdevkit')
    assert a.trg_datalist == 'dataloader/init_data/voc/train_seed150.txt'
    assert a.do_data_dir == './data/VOCdevkit/superpixels/pascal_voc_seg/seeds_150/train/gtFine_dominant_ignore'
    assert la.dominant_file(a, './data/VOCdevkit/VOC2012/JPEGImages/2007_000032.jpg') == a.do_data_dir + '/2007_000032.png'
    a = _args(['multi_hot', '--dataset', 'voc', '--trim_multihot_boundary', '--trim_kernel_size', '5'])
    assert a.save_data_dir == './data/VOCdevkit/superpixels/pascal_voc_seg/seeds_32/train/gtFine_multi_tensor_trim_5x5'


def test_cli_reads_a_datalist(tmp_path):
    from mulactseg_amd import label_assignment as la
    import json
    (tmp_path / 'l.txt').write_text('img/a_1_2_x.png\tlbl/a.png\tspx/a.pkl\nimg/b_3_4_x.png\tlbl/b.png\tspx/b.pkl\n')
    (tmp_path / 'r.dict').write_text(json.dumps({'spx/a.pkl': [4, [1]], 'spx/b.pkl': [3, []]}))
    a = _args(['multi_hot', '--trg_data_dir', str(tmp_path), '--trg_datalist', str(tmp_path / 'l.txt'),
               '--region_dict', str(tmp_path / 'r.dict'), '--nseg', '4'])
    pics, lists = la.read_pictures(a)
    assert [p[1] for p in pics] == [os.path.join(str(tmp_path), 'lbl/a.png'), os.path.join(str(tmp_path), 'lbl/b.png')]
    assert lists == [[0, 2, 3], [0, 1, 2]]


# ---- the C entry points reject bad arguments before any launch ------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from mulactseg_amd import _lib
    lib = _lib.load()
    fake = 4096                                               # never dereferenced: every call below fails its argument checks
    # even trim kernel, too large, negative
    for k in (2, 4, 17, -1):
        assert lib.mas_region_label_counts(fake, _lib.ID_I64, fake, 8, 8, 4, 19, k, fake, fake, fake, None) == -6
    # C + 1 > MAS_MAX_CLASSES
    assert lib.mas_region_label_counts(fake, _lib.ID_I64, fake, 8, 8, 4, _lib.MAX_CLASSES, 0, fake, None, fake, None) == -3
    assert lib.mas_region_multi_hot(fake, None, fake, 4, _lib.MAX_CLASSES, fake, fake, None) == -3
    assert lib.mas_region_dominant(fake, fake, None, 4, 0, 0, fake, None) == -3
    # null pointers
    assert lib.mas_region_label_counts(None, _lib.ID_I64, fake, 8, 8, 4, 19, 0, fake, None, fake, None) == -1
    assert lib.mas_region_label_counts(fake, _lib.ID_I64, fake, 8, 8, 4, 19, 5, fake, None, fake, None) == -1     # trimmed missing
    assert lib.mas_region_multi_hot(fake, None, None, 4, 19, fake, fake, None) == -1
    assert lib.mas_region_dominant(fake, fake, None, 4, 19, 0, None, None) == -1
    assert lib.mas_region_paint(fake, _lib.ID_I32, fake, 8, 8, 4, None, 0, fake, None) == -1
    # dtype and shape
    assert lib.mas_region_paint(fake, 3, fake, 8, 8, 4, fake, 0, fake, None) == -4
    assert lib.mas_region_label_counts(fake, _lib.ID_U16, fake, 0, 8, 4, 19, 0, fake, None, fake, None) == -2
    assert lib.mas_region_multi_hot(fake, None, fake, 0, 19, fake, fake, None) == -2


def test_ops_reject_an_even_trim_kernel_before_any_launch():
    from mulactseg_amd import ops
    with pytest.raises(ValueError):
        ops.trim_kernel(2)
    assert ops.trim_kernel(None) == 0 and ops.trim_kernel(5) == 5
    with pytest.raises(ValueError):
        ops.listed_ids([0, 4], 4, 'cpu')
