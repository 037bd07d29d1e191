"""Photometric augmentation on the device (csrc/photometric.hip): mas_train_augment_u8 and mas_photometric against the f32 kernel,
against the host entry mas_photometric_reference (csrc/photometric.h run as a host loop, itself pinned to Pillow in
tests/test_photometric_cpu.py) and against the G13 goldens the reference's own transform classes produced -- bit for bit."""
import itertools
import os
import random

import numpy as np
import pytest
import torch

import helpers
from test_photometric_cpu import CONTRAST, MEAN, STD, chain, g13_samples, one_op

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd.dataloader import device_transforms
    return device_transforms


def normalise(u8):
    """to-tensor + normalise of a u8 [h,w,3] crop exactly as k_train_augment writes it."""
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    return (x - np.asarray(MEAN, np.float32)[:, None, None]) / np.asarray(STD, np.float32)[:, None, None]


def crop_picture(seed, h, w):
    """Noise with a flat grey block (s == 0), black, white and saturated channels."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    img[2:9, 3:14] = rs.randint(1, 255)
    img[10:15, 1:9], img[16:22, 5:20] = 0, 255
    img[20:30, 24:40] = (255, 0, 77)
    img[3:12, 30:44, 1] = 255
    return img


def identity_params(h, w, ph):
    return dict(scale=1.0, th=h, tw=w, gap_y=0, gap_x=0, i=0, j=0, flip=False, photometric=ph)


def chains_under_test():
    rs = np.random.RandomState(21)
    out = [one_op(op, a) for op in range(3) for a in (0.0, 0.7, 1.0, 1.3, 2.2)]              # every single op, both sides of 1
    out += [one_op(3, h) for h in (-0.5, -0.05, 0.0, 0.004, 0.1, 0.5)]
    out += [chain((1, 0, 2, 3), (0.8, 1.3, 1.2, 0.03)), chain((0, 2, 3, 1), (1.3, 0.7, 0.8, -0.08))]   # contrast first / last
    for k, order in enumerate(itertools.permutations(range(4))):                              # all 24 orders, every third grey
        f = [float(v) for v in rs.uniform(0.6, 1.4, size=3).astype(np.float32)] + [float(np.float32(rs.uniform(-0.1, 0.1)))]
        out.append(chain(order, f, grey=k % 3 == 0))
    out += [dict(order=None, factors=[None] * 4, grey=True),                                  # grey alone
            chain((2, 3, 0, 1), (None, 1.25, None, 0.07), grey=True)]                         # absent ops between present ones
    return out


@pytest.mark.parametrize("h,w", [(32, 48), (33, 47)])          # 1536 = 4 * 384 pixels: the 16-byte stores; 1551: the scalar tail
def test_kernel_equals_host_entry(h, w):
    dt = _gpu()
    img = crop_picture(h, h, w)
    dev = torch.from_numpy(img).cuda()
    aug = dt.DeviceTrainAugmentStrong(size=(h, w), scale_range=(1.0, 1.0), pad_values=[])
    for ph in chains_under_test():
        ref_u8, ref_f32, ref_sum = dt.photometric_reference(img, ph, MEAN, STD)
        crop, _, lsum = aug.augment_u8(dev, (), identity_params(h, w, ph))
        assert np.array_equal(crop.cpu().numpy(), img)                    # pass 1 stores the crop un-jittered
        has_contrast = ph['order'] is not None and ph['factors'][CONTRAST] is not None
        assert (lsum is not None) == has_contrast
        if has_contrast:
            assert int(lsum.item()) == ref_sum and ref_sum > 0            # the accumulator: the host sum, exactly
        f32, u8 = dt.photometric(crop, ph, lsum, MEAN, STD, return_u8=True)
        assert np.array_equal(u8.cpu().numpy(), ref_u8), ph
        assert np.array_equal(f32.cpu().numpy(), ref_f32), ph
        assert np.array_equal(ref_f32, normalise(ref_u8))


def test_augment_u8_equals_the_f32_kernel_and_g13():
    """Pass 1 against mas_train_augment with the same geometry (its u8 values mapped through the normalisation are the f32 picture,
    its maps are the same) and against the Pillow-made goldens of G13 (maps of every sample; the picture where nothing was drawn)."""
    dt = _gpu()
    n_plain = 0
    for g, k, row in g13_samples():
        H, W, crop, nseg = int(g['H']), int(g['W']), tuple(int(v) for v in g['crop']), int(g['nseg'])
        pic = int(row['picture'])
        p = dt.draw_params(random.Random(int(row['py_seed'])), H, W, crop, scale_range=(row['scale_lo'], row['scale_hi']))
        img, lbl, spx = (torch.from_numpy(g[n][pic]).cuda() for n in ('pictures', 'labels', 'spx'))
        plain = dt.DeviceTrainAugment(size=crop, pad_values=[0, nseg])
        t, (l1, s1) = plain(img, [lbl, spx], params=p)
        strong = dt.DeviceTrainAugmentStrong(size=crop, pad_values=[0, nseg])
        ph = chain((2, 1, 0, 3), (1.2, 0.9, 1.1, 0.05)) if k % 2 else dict(order=None, factors=[None] * 4, grey=True)
        c, (l2, s2), lsum = strong.augment_u8(img, [lbl, spx], dict(p, photometric=ph))
        assert np.array_equal(normalise(c.cpu().numpy()), t.cpu().numpy())
        assert torch.equal(l1, l2) and torch.equal(s1, s2) and (lsum is not None) == bool(k % 2)
        assert np.array_equal(l2.cpu().numpy(), g['out_labels'][k]) and np.array_equal(s2.cpu().numpy(), g['out_spx'][k])
        if not row['jittered'] and not row['grey']:
            n_plain += 1
            assert np.array_equal(normalise(c.cpu().numpy()), g['images'][k])
    assert n_plain >= 1


def _strong_for(dt, g, row, **kw):
    return dt.DeviceTrainAugmentStrong(brightness=row['brightness'], contrast=row['contrast'], saturation=row['saturation'], hue=row['hue'],
                                       p_jitter=row['p_jitter'], p_gray=row['p_gray'], size=tuple(int(v) for v in g['crop']),
                                       scale_range=(row['scale_lo'], row['scale_hi']), pad_values=[0, int(g['nseg'])], **kw)


def test_g13_through_the_strong_transform():
    """The stored seeds on Python's ``random`` (geometry) and on a torch generator (photometric draws): picture and maps of every
    sample equal what the reference's classes produced; ``torch_generator=None`` draws from torch's global generator."""
    dt = _gpu()
    for g, k, row in g13_samples():
        pic = int(row['picture'])
        img, lbl, spx = (torch.from_numpy(g[n][pic]).cuda() for n in ('pictures', 'labels', 'spx'))
        if k % 5 == 0:
            aug = _strong_for(dt, g, row, rng=random.Random(int(row['py_seed'])))
            torch.manual_seed(int(row['torch_seed']))
        else:
            aug = _strong_for(dt, g, row, rng=random.Random(int(row['py_seed'])),
                              torch_generator=torch.Generator().manual_seed(int(row['torch_seed'])))
        t, (l2, s2) = aug(img, [lbl, spx])
        assert t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), g['images'][k]), (k, str(g['kinds'][k]))
        assert l2.dtype == torch.uint8 and np.array_equal(l2.cpu().numpy(), g['out_labels'][k])
        assert s2.dtype == torch.int64 and np.array_equal(s2.cpu().numpy(), g['out_spx'][k])


def test_a_sample_that_draws_neither_op_is_the_plain_augmentation():
    dt = _gpu()
    rs = np.random.RandomState(4)
    img = torch.from_numpy(rs.randint(0, 256, size=(130, 75, 3)).astype(np.uint8)).cuda()
    spx = torch.from_numpy(rs.randint(0, 40, size=(130, 75)).astype(np.int32)).cuda()
    for seed in range(4):
        plain = dt.DeviceTrainAugment(size=(96, 128), pad_values=[40], rng=random.Random(seed))
        strong = dt.DeviceTrainAugmentStrong(p_jitter=0.0, p_gray=0.0, size=(96, 128), pad_values=[40], rng=random.Random(seed),
                                             torch_generator=torch.Generator().manual_seed(seed + 1))      # (u = 0 is never drawn here)
        a, (sa,) = plain(img, [spx])
        b, (sb,) = strong(img, [spx])
        assert torch.equal(a, b) and torch.equal(sa, sb)
    # and with the parameters handed in
    p = dt.draw_params(random.Random(9), 130, 75, (96, 128))
    a, _ = plain(img, [spx], params=p)
    b, _ = strong(img, [spx], params=dict(p, photometric=dict(order=None, factors=[None] * 4, grey=False)))
    assert torch.equal(a, b)


def test_production_shape_full_chain_twice():
    """1024 x 2048 -> 768 x 768 with the whole chain and grayscale: the kernels against the host entry on the same u8 crop, the
    accumulator against the host sum, and two runs against each other."""
    dt = _gpu()
    rs = np.random.RandomState(14)
    img = torch.from_numpy(rs.randint(0, 256, size=(1024, 2048, 3)).astype(np.uint8)).cuda()
    spx = torch.from_numpy(rs.randint(0, 2048, size=(1024, 2048)).astype(np.int16)).cuda()
    aug = dt.DeviceTrainAugmentStrong(size=(768, 768), pad_values=[2048])
    for seed, ph in ((14, chain((3, 0, 1, 2), (1.31, 0.72, 1.18, -0.06), grey=False)), (15, chain((2, 1, 3, 0), (0.66, 1.37, 0.81, 0.09), grey=True))):
        p = dict(dt.draw_params(random.Random(seed), 1024, 2048, (768, 768)), photometric=ph)
        t1, (s1,) = aug(img, [spx], params=p)
        t2, (s2,) = aug(img, [spx], params=p)
        assert torch.equal(t1, t2) and torch.equal(s1, s2)
        crop, _, lsum = aug.augment_u8(img, [spx], p)
        _, ref, ref_sum = dt.photometric_reference(crop.cpu().numpy(), ph, MEAN, STD)
        assert int(lsum.item()) == ref_sum
        assert tuple(t1.shape) == (3, 768, 768) and np.array_equal(t1.cpu().numpy(), ref)


def test_file_backed_sample_with_a_strong_name(tmp_path):
    """``--loader region_cityscapes_or_tensor --train_transform rescale_769_multi_notrg_strongv1`` on a written tree: a labelled
    sample with both ops forced and one at the reference's probabilities."""
    dt = _gpu()
    from mulactseg_amd import dataloader
    H, W, NSEG, CROP = 128, 256, 64, 128
    dataloader.register_dataset_factory(None)
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=3, H=H, W=W, nseg=NSEG)
    args = helpers.cityscapes_tree_args(tree, tmp_path / 'run', ['--train_transform', 'rescale_769_multi_notrg_strongv1'])
    os.makedirs(args.model_save_dir, exist_ok=True)
    aset = dataloader.get_active_dataset(args, train_transform=args.train_transform)
    pool, label = aset.trg_pool_dataset, aset.trg_label_dataset
    assert type(label.transform) is dt.DeviceTrainAugmentStrong and label.transform.n_maps == 1
    label.transform.size = (CROP, CROP)
    aset.selection_iter = 1
    aset.expand_training_set([(1.0 - 0.01 * i, ','.join(pool.im_idx[1]), s) for i, s in enumerate([3, 7, 11, 40])], 10 ** 6, 'x')
    label.transform.rng = random.Random(11)
    torch.manual_seed(3)
    plain = label[0]
    label.transform.jitter.update(p_jitter=1.0, p_gray=1.0)
    grey = label[0]
    for s in (plain, grey):
        assert s['images'].is_cuda and s['images'].dtype == torch.float32 and tuple(s['images'].shape) == (3, CROP, CROP)
        assert bool(torch.isfinite(s['images']).all())
        assert s['spx'].dtype == torch.int64 and tuple(s['spx'].shape) == (CROP, CROP) and s['spmask'].dtype == torch.bool
    # grayscale: the three planes hold one u8 value per pixel
    x = grey['images'].cpu().numpy()
    back = [np.rint((x[c] * np.float32(STD[c]) + np.float32(MEAN[c])) * 255).astype(np.int64) for c in range(3)]
    assert np.array_equal(back[0], back[1]) and np.array_equal(back[1], back[2])
