"""Photometric augmentation (csrc/photometric.h, csrc/photometric.hip) without a GPU: the library's host entry
``mas_photometric_reference`` -- the CPU-side statement of the arithmetic the kernels are compared with bit for bit in
tests/test_photometric_gpu.py -- against Pillow itself (ImageEnhance, ImageStat, convert('HSV'), convert('L')), against the G13
goldens the reference's own transform classes produced (tools/gen_golden_photometric.py), and the new transform names."""
import itertools
import os
import random
import re
import types

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageStat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G13 = os.path.join(os.path.dirname(__file__), "golden", "g13_photometric.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
ENHANCERS = {BRIGHTNESS: ImageEnhance.Brightness, CONTRAST: ImageEnhance.Contrast, SATURATION: ImageEnhance.Color}


def dt():
    from mulactseg_amd.dataloader import device_transforms
    return device_transforms


def chain(order=(0, 1, 2, 3), factors=(None, None, None, None), grey=False):
    return dict(order=list(order), factors=list(factors), grey=grey)


def one_op(op, a):
    f = [None] * 4
    f[op] = a
    return chain(factors=f)


def pillow_hue(pil, hue):
    """torchvision 0.12 ``adjust_hue``: the H band plus ``uint8(hue * 255)``, wrapping."""
    h, s, v = pil.convert('HSV').split()
    nh = (np.array(h, dtype=np.uint8).astype(np.int32) + (int(hue * 255) & 0xFF)).astype(np.uint8)
    return Image.merge('HSV', (Image.fromarray(nh, 'L'), s, v)).convert('RGB')


def pillow_chain(pil, order, factors, grey):
    for op in order:
        if factors[op] is None:
            continue
        pil = pillow_hue(pil, factors[op]) if op == HUE else ENHANCERS[op](pil).enhance(factors[op])
    if grey:
        lum = np.array(pil.convert('L'))
        pil = Image.fromarray(np.dstack([lum, lum, lum]), 'RGB')
    return np.array(pil)


def pictures():
    """Random and extreme pictures; the last two have a mean L whose fraction is >= .5 and < .5."""
    rs = np.random.RandomState(7)
    out = [rs.randint(0, 256, size=(37, 53, 3)).astype(np.uint8), rs.randint(0, 40, size=(16, 20, 3)).astype(np.uint8),
           rs.randint(215, 256, size=(16, 20, 3)).astype(np.uint8), np.zeros((5, 7, 3), np.uint8), np.full((5, 7, 3), 255, np.uint8)]
    ext = rs.randint(0, 256, size=(24, 24, 3)).astype(np.uint8)
    ext[:8], ext[8:16, :, 0], ext[16:, :, 2] = 255, 0, 255
    out.append(ext)
    hi = np.zeros((1, 4, 3), np.uint8)
    hi[0, :3] = 100            # grey pixels (L = value): 100, 100, 100 and
    hi[0, 3] = 102             # 102 -> mean L = 100.5
    lo = hi.copy()
    lo[0, 3] = 101             # mean L = 100.25
    return out + [hi, lo]


def factors_under_test():
    rs = np.random.RandomState(3)
    return [0.0, 0.6, 1.0, 1.4] + [float(v) for v in rs.uniform(0.0, 2.5, size=50).astype(np.float32)]


def test_grey_blends_and_contrast_mean_equal_pillow():
    pics = pictures()
    fr = [ImageStat.Stat(Image.fromarray(p).convert('L')).mean[0] % 1.0 for p in pics]
    assert fr[-2] >= 0.5 and 0 < fr[-1] < 0.5
    for p in pics:
        pil = Image.fromarray(p)
        lum = np.array(pil.convert('L'))
        u8, _, lsum = dt().photometric_reference(p, chain(grey=True))
        assert np.array_equal(u8, np.dstack([lum, lum, lum])) and lsum == 0
        # the contrast sum and mean: ImageStat on convert('L'), as ImageEnhance.Contrast computes its degenerate image
        _, _, lsum = dt().photometric_reference(p, one_op(CONTRAST, 0.0))
        assert lsum == int(lum.astype(np.int64).sum())
        u8, _, _ = dt().photometric_reference(p, one_op(CONTRAST, 0.0))
        assert (u8 == int(ImageStat.Stat(pil.convert('L')).mean[0] + 0.5)).all()
        for a in factors_under_test():
            for op, enh in ENHANCERS.items():
                u8, _, _ = dt().photometric_reference(p, one_op(op, a))
                assert np.array_equal(u8, np.array(enh(pil).enhance(a))), (op, a)


@pytest.fixture(scope="module")
def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("shift", [0, 1, 25, 244])
def test_hue_equals_pillow_on_all_colours(all_colours, shift):
    """Both HSV directions over all 2^24 colours; the hue value is chosen so that ``int(hue * 255) & 0xFF`` is the shift."""
    hue = {0: 0.0, 1: 0.004, 25: 0.1, 244: -0.05}[shift]
    assert int(float(np.float32(hue)) * 255) & 0xFF == shift
    ref = np.array(pillow_hue(Image.fromarray(all_colours), float(np.float32(hue))))
    u8, _, _ = dt().photometric_reference(all_colours, one_op(HUE, hue))
    assert np.array_equal(u8, ref)


def test_all_orders_equal_the_chained_pillow_calls():
    rs = np.random.RandomState(11)
    pic = pictures()[0]
    pil = Image.fromarray(pic)
    for k, order in enumerate(itertools.permutations(range(4))):
        f = [float(v) for v in rs.uniform(0.6, 1.4, size=3).astype(np.float32)] + [float(np.float32(rs.uniform(-0.1, 0.1)))]
        grey = k % 3 == 0
        u8, f32, _ = dt().photometric_reference(pic, chain(order, f, grey))
        ref = pillow_chain(pil, order, f, grey)
        assert np.array_equal(u8, ref), order
        # to-tensor + normalise exactly as k_train_augment writes it
        want = (ref.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - np.asarray(MEAN, np.float32)[:, None, None]) \
            / np.asarray(STD, np.float32)[:, None, None]
        assert np.array_equal(f32, want)
    # an absent op is skipped wherever it stands; no jitter at all is the identity
    u8, _, _ = dt().photometric_reference(pic, chain((3, 1, 0, 2), (None, 1.3, None, -0.07)))
    assert np.array_equal(u8, pillow_chain(pil, (3, 1, 0, 2), (None, 1.3, None, -0.07), False))
    u8, _, _ = dt().photometric_reference(pic, dict(order=None, factors=[None] * 4, grey=False))
    assert np.array_equal(u8, pic)


def test_bad_chains_are_refused():
    from mulactseg_amd import _lib
    pic = pictures()[0]
    for bad in (chain((0, 1, 2, 2), (1.0, 1.0, 1.0, 0.0)), chain((0, 1, 2, 4), (1.0, 1.0, 1.0, 0.0)), one_op(BRIGHTNESS, -0.1),
                one_op(HUE, 0.6), one_op(CONTRAST, float('nan'))):
        with pytest.raises(_lib.MulActSegHipError):
            dt().photometric_reference(pic, bad)


def g13_samples():
    g = np.load(G13)
    col = {str(n): i for i, n in enumerate(g['columns'])}
    for k, row in enumerate(g['samples']):
        yield g, k, {n: row[i] for n, i in col.items()}


def g13_draw(row, crop, H, W):
    """``draw_params`` then ``draw_photometric`` under the stored seeds -> the sample's parameters."""
    gen = torch.Generator().manual_seed(int(row['torch_seed']))
    p = dt().draw_params(random.Random(int(row['py_seed'])), H, W, crop, scale_range=(row['scale_lo'], row['scale_hi']))
    p['photometric'] = dt().draw_photometric(gen, row['brightness'], row['contrast'], row['saturation'], row['hue'], row['p_jitter'],
                                             row['p_gray'])
    return p


def test_g13_draw_order_and_arithmetic_equal_the_executed_reference_classes():
    """The geometry (oracle/augment.py, pinned by G9) under the stored ``random`` seed gives the u8 crop; the photometric draws under
    the stored torch seed and the host entry give the picture -- bit-equal to what the reference's ExtColorJitter / ExtRandomGrayscale
    / ExtToTensor / ExtNormalize produced."""
    from oracle import augment
    seen = set()
    for g, k, row in g13_samples():
        H, W, crop = int(g['H']), int(g['W']), tuple(int(v) for v in g['crop'])
        pic = int(row['picture'])
        p = g13_draw(row, crop, H, W)
        ph = p['photometric']
        assert (ph['order'] is not None) == bool(row['jittered']) and ph['grey'] == bool(row['grey'])
        if ph['order'] is not None:
            assert ph['order'] == [int(v) for v in g['orders'][k]]
            want = [None if np.isnan(v) else float(v) for v in g['factors'][k]]
            assert ph['factors'] == want
            seen.add(tuple(ph['order']))
        plain, (lbl, spx) = augment.train_augment(g['pictures'][pic], [g['labels'][pic], g['spx'][pic]], [0, int(g['nseg'])], p, crop, MEAN, STD)
        assert np.array_equal(lbl, g['out_labels'][k]) and np.array_equal(spx, g['out_spx'][k])
        if ph['order'] is None and not ph['grey']:
            assert np.array_equal(plain, g['images'][k])
            continue
        # the u8 crop behind the plain picture: x -> (x / 255 - mean) / std is strictly increasing on 0..255
        lut = [(np.arange(256, dtype=np.float32) / np.float32(255) - np.float32(MEAN[c])) / np.float32(STD[c]) for c in range(3)]
        crop_u8 = np.stack([np.searchsorted(lut[c], plain[c]) for c in range(3)], axis=2).astype(np.uint8)
        assert all(np.array_equal(lut[c][crop_u8[..., c]], plain[c]) for c in range(3))
        _, f32, _ = dt().photometric_reference(crop_u8, ph, MEAN, STD)
        assert np.array_equal(f32, g['images'][k]), (k, ph)
    assert len(seen) == 24


def test_g13_holds_what_it_should():
    g = np.load(G13)
    col = {str(n): i for i, n in enumerate(g['columns'])}
    rows, kinds = g['samples'], [str(k) for k in g['kinds']]
    ref = rows[[k == 'ref' for k in kinds]]
    jit, grey = ref[:, col['jittered']] == 1, ref[:, col['grey']] == 1
    assert len(ref) == 12 and jit.sum() >= 4 and grey.sum() >= 2 and (jit & grey).any() and (~jit & ~grey).any()
    assert (ref[:, col['p_jitter']] == 0.2).all() and (ref[:, col['p_gray']] == 0.2).all()
    assert len({tuple(o) for o, k in zip(g['orders'], kinds) if k == 'order'}) == 24
    assert 2 * rows[:, col['padded']].sum() >= len(rows)
    assert kinds.count('single') >= 4 and os.path.getsize(G13) < 256 * 1024
    for pic in g['pictures']:
        flat = (pic.max(axis=2) == pic.min(axis=2)).mean()
        assert flat > 0.05 and (pic == 255).any() and (pic == 0).any()


def test_draw_photometric_follows_torchvision_0_12():
    """rand (jitter unless p < u), randperm(4), one uniform_ per component with a range, rand (grey) -- on the given generator."""
    d = dt()
    for seed in range(40):
        gen, twin = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        got = d.draw_photometric(gen, 0.4, 0.0, 0.4, 0.1, 0.5, 0.3)
        u = torch.rand(1, generator=twin)
        if 0.5 < u:
            assert got['order'] is None and got['factors'] == [None] * 4
        else:
            assert got['order'] == [int(v) for v in torch.randperm(4, generator=twin)]
            b = float(torch.empty(1).uniform_(0.6, 1.4, generator=twin))
            s = float(torch.empty(1).uniform_(0.6, 1.4, generator=twin))
            h = float(torch.empty(1).uniform_(-0.1, 0.1, generator=twin))
            assert got['factors'] == [b, None, s, h]             # contrast 0: no range, no draw
        assert got['grey'] == bool(torch.rand(1, generator=twin) < 0.3)
        assert torch.equal(gen.get_state(), twin.get_state())
    # None: the global generator, as in the reference
    torch.manual_seed(5)
    a = d.draw_photometric(None, p_jitter=1.0)
    torch.manual_seed(5)
    assert a == d.draw_photometric(None, p_jitter=1.0) and a['order'] is not None
    assert d._jitter_range(0.4) == (0.6, 1.4) and d._jitter_range(1.5) == (0.0, 2.5) and d._jitter_range(0) is None
    with pytest.raises(ValueError):
        d.draw_photometric(None, hue=0.6)


CITY = {'rescale_769_nospx_strongv1': ('rescale_769_nospx', 1), 'rescale_769_strongv1': ('rescale_769', 2),
        'rescale_769_multi_strongv1': ('rescale_769_multi', 2), 'rescale_769_multi_notrg_strongv1': ('rescale_769_multi_notrg', 1),
        'rescale_769_multi_notrg_ignore_strongv1': ('rescale_769_multi_notrg_ignore', 2)}
VOC = {'rescale_513_notrg_strongv1': ('rescale_513_notrg', 1), 'rescale_513_strongv1': ('rescale_513', 2),
       'rescale_513_multi_notrg_strongv1': ('rescale_513_multi_notrg', 1)}


def test_strong_names():
    from mulactseg_amd.dataloader import device_transforms as d
    from mulactseg_amd.dataloader import get_train_transform, get_train_transform_voc
    args = types.SimpleNamespace(ignore_idx=255, nseg=2048, load_smaller_spx=False)
    small = types.SimpleNamespace(ignore_idx=255, nseg=2048, load_smaller_spx=True)
    for get, names, size in ((get_train_transform, CITY, (768, 768)), (get_train_transform_voc, VOC, (513, 513))):
        for name, (base, n_maps) in names.items():
            t, b = get(args, name), get(args, base)
            assert type(t) is d.DeviceTrainAugmentStrong and type(b) is d.DeviceTrainAugment          # old names: the same class as before
            assert t.n_maps == b.n_maps == n_maps and t.pad_values == b.pad_values and t.size == b.size == size
            assert t.scale_range == b.scale_range == (0.5, 2.0) and np.array_equal(t.fill, b.fill)
            assert t.jitter == dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p_jitter=0.2, p_gray=0.2)
            assert t.torch_generator is None
            if 'multi' in name:
                with pytest.raises(NotImplementedError):
                    get(small, name)
    assert get_train_transform(args, 'rescale_769_multi_notrg_ignore_strongv1').pad_values == [0, 2048]
    assert type(get_train_transform(args, 'eval_spx')) is d.DeviceResize
    assert type(get_train_transform_voc(args, 'rescale_769_nospx')) is d.DeviceResizeFlip
    with pytest.raises(NotImplementedError):
        get_train_transform(args, 'rescale_769_strongv2')


def test_header_exports_and_ctypes_table_agree():
    import ctypes
    from mulactseg_amd import _lib
    header = open(os.path.join(ROOT, "include", "mulactseg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mas_[a-z0-9_]+)\s*\(", text)))
    assert sorted(_lib.SIGNATURES) == declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mas_train_augment_u8", "mas_photometric", "mas_photometric_reference"):
        assert name in declared and hasattr(lib, name)
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(',') if a.strip()])
        assert n_args == len(_lib.SIGNATURES[name][1])
    assert int(re.search(r"#define MAS_ABI_VERSION (\d+)", header).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().mas_abi_version()


def test_argument_errors():
    from mulactseg_amd import _lib
    lib = _lib.load()
    pic = pictures()[0]
    o, f = np.arange(4, dtype=np.int32), np.ones(4, dtype=np.float32)
    m = np.asarray(MEAN, np.float32)
    assert lib.mas_photometric_reference(None, 4, 4, o.ctypes.data, f.ctypes.data, 0, 0, m.ctypes.data, m.ctypes.data, None, None, None) == -1
    assert lib.mas_photometric_reference(pic.ctypes.data, 0, 4, o.ctypes.data, f.ctypes.data, 0, 0, m.ctypes.data, m.ctypes.data, None, None, None) == -2
    assert lib.mas_photometric_reference(pic.ctypes.data, 4, 4, None, None, 1, 0, m.ctypes.data, m.ctypes.data, None, None, None) == -1
    assert lib.mas_photometric_reference(pic.ctypes.data, 4, 4, o.ctypes.data, f.ctypes.data, 16, 0, m.ctypes.data, m.ctypes.data, None, None, None) == -6
    # refused before any launch: no GPU is needed to be told so
    assert lib.mas_photometric(None, 4, 4, o.ctypes.data, f.ctypes.data, 0, 0, m.ctypes.data, m.ctypes.data, None, None, None, None) == -1
    assert lib.mas_photometric(pic.ctypes.data, 4, 4, o.ctypes.data, f.ctypes.data, 0, 0, m.ctypes.data, m.ctypes.data, None, None, None, None) == -1
