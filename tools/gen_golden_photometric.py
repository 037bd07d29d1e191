"""Generate ``tests/golden/g13_photometric.npz`` by RUNNING THE REFERENCE'S OWN transform classes (build container only; needs the
reference tree, see ``oracle/refshim/install.py``) as ``dataloader/transform.py:139-153`` composes them for
``rescale_769_multi_notrg_ignore_strongv1``::

    ExtCompose([ExtRandomScale, ExtRandomCrop(pad_if_needed), ExtRandomHorizontalFlip, ExtColorJitter(b, c, s, h, p),
                ExtRandomGrayscale(p), ExtToTensor, ExtNormalize])

with a 32x48 crop of 40x56 pictures, under seeded ``random`` (geometry) and seeded ``torch`` (photometric draws).

Run:  ``python tools/gen_golden_photometric.py``.  Nothing of the reference is copied: ``dataloader/ext_transforms.py`` is imported
from where it lies, with ``torchvision`` replaced by ``oracle/refshim/torchvision_shim`` (torchvision is not installed here).  That
stand-in has no ``ColorJitter`` / ``RandomGrayscale``; the two classes below restate torchvision 0.12.0's (``transforms/transforms.py``,
``transforms/functional_pil.py``) on the Pillow calls it makes -- ``ImageEnhance.{Brightness,Contrast,Color}``, ``convert('HSV')``,
``convert('L')`` -- so the order of the draws comes from the reference's classes and the arithmetic from Pillow itself.  Like the
shim they are a stand-in at a third-party boundary; they record what they drew so that the fixture can say which samples were
jittered.

Samples (``kind``): 12 at the reference's probabilities (0.4, 0.4, 0.4, 0.1, p = 0.2; grey p = 0.2), torch seeds scanned in order
until 5 jittered-only, 2 grey-only, 1 both and 4 neither are found; all 24 op orders at p = 1 (the first torch seed that yields each
permutation; every fourth also grey); one sample per single op, one with hue 0.5, one grey only.  The pictures hold noise, flat
grey / black / white blocks (the ``s == 0`` branch of HSV -> RGB) and saturated channels; odd samples draw their scale from
(0.5, 0.78), so that the crop holds pad fill.  The archive is written with fixed member dates: a rerun reproduces it byte for byte.
"""
import importlib.util
import io
import itertools
import os
import random
import sys
import zipfile

import numpy as np
import torch
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.refshim import install as refshim  # noqa: E402
from oracle.refshim import torchvision_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g13_photometric.npz")
H, W, CROP, NSEG = 40, 56, (32, 48), 24
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
STRONG = (0.4, 0.4, 0.4, 0.1)
N_PICTURES = 4


class ColorJitter:
    """torchvision 0.12.0 ``transforms.ColorJitter`` on PIL images."""
    last = None

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = self._check_input(brightness)
        self.contrast = self._check_input(contrast)
        self.saturation = self._check_input(saturation)
        self.hue = self._check_input(hue, center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    @staticmethod
    def _check_input(value, center=1, bound=(0, float("inf")), clip_first_on_zero=True):
        if value < 0:
            raise ValueError("a jitter strength must be non negative")
        value = [center - float(value), center + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError("jitter values should be between {}".format(bound))
        return None if value[0] == value[1] == center else value

    @staticmethod
    def get_params(brightness, contrast, saturation, hue):
        fn_idx = torch.randperm(4)
        b = None if brightness is None else float(torch.empty(1).uniform_(brightness[0], brightness[1]))
        c = None if contrast is None else float(torch.empty(1).uniform_(contrast[0], contrast[1]))
        s = None if saturation is None else float(torch.empty(1).uniform_(saturation[0], saturation[1]))
        h = None if hue is None else float(torch.empty(1).uniform_(hue[0], hue[1]))
        return fn_idx, b, c, s, h

    def __call__(self, img):
        fn_idx, b, c, s, h = self.get_params(self.brightness, self.contrast, self.saturation, self.hue)
        ColorJitter.last = ([int(v) for v in fn_idx], [b, c, s, h])
        for fn_id in fn_idx:
            if fn_id == 0 and b is not None:
                img = ImageEnhance.Brightness(img).enhance(b)
            elif fn_id == 1 and c is not None:
                img = ImageEnhance.Contrast(img).enhance(c)
            elif fn_id == 2 and s is not None:
                img = ImageEnhance.Color(img).enhance(s)
            elif fn_id == 3 and h is not None:
                img = adjust_hue(img, h)
        return img


def adjust_hue(img, hue_factor):
    """``functional_pil.adjust_hue``: the H band plus ``np.uint8(hue_factor * 255)``, wrapping (the cast truncates toward zero and
    wraps a negative value, written out here because numpy 2 no longer casts a negative float silently)."""
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError("hue_factor ({}) is not in [-0.5, 0.5].".format(hue_factor))
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(int(hue_factor * 255) & 0xFF)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


class RandomGrayscale:
    """torchvision 0.12.0 ``transforms.RandomGrayscale`` on an RGB PIL image: ``convert('L')`` stacked three times."""
    last = False

    def __init__(self, p=0.1):
        self.p = p

    def __call__(self, img):
        RandomGrayscale.last = False
        if torch.rand(1) < self.p:
            RandomGrayscale.last = True
            lum = np.array(img.convert("L"), dtype=np.uint8)
            return Image.fromarray(np.dstack([lum, lum, lum]), "RGB")
        return img


def reference_ext_transforms():
    """The reference's ``dataloader/ext_transforms.py`` by path (the package name ``dataloader`` is taken by the stand-in)."""
    import collections
    import collections.abc
    refshim.install()
    tv = torchvision_shim.install_torchvision()
    tv.transforms.ColorJitter = ColorJitter
    tv.transforms.RandomGrayscale = RandomGrayscale
    if not hasattr(collections, "Iterable"):
        collections.Iterable = collections.abc.Iterable
    spec = importlib.util.spec_from_file_location("ref_ext_transforms", os.path.join(refshim.REFERENCE_ROOT, "dataloader", "ext_transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def picture(k):
    """Picture k with its label and superpixel maps: noise, a smooth ramp, flat grey / black / white blocks, saturated channels."""
    rs = np.random.RandomState(1300 + k)
    img = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    img[:, 28:] = np.stack([(xx * 4 + yy) % 256, (yy * 6) % 256, (255 - xx * 3) % 256], axis=2).astype(np.uint8)[:, 28:]
    img[4:14, 4:16] = rs.randint(0, 256)                 # flat grey: max == min, s == 0
    img[16:24, 2:12] = 0
    img[26:36, 6:18] = 255
    img[6:18, 34:46] = (255, 0, rs.randint(0, 256))      # saturated channels
    img[22:34, 36:50] = (rs.randint(0, 256), 255, 255)
    img[30:38, 20:30, 0] = 255                           # a saturated channel over noise
    blocks = (yy // 10) * 6 + xx // 10
    lbl = ((blocks * 7 + k) % 19).astype(np.uint8)
    spx = (blocks % NSEG).astype(np.int32)
    return img, lbl, spx


def run(et, pic, py_seed, torch_seed, jitter, p_jitter, p_gray, scale_range):
    img, lbl, spx = pic
    tf = et.ExtCompose([et.ExtRandomScale(scale_range),
                        et.ExtRandomCrop(size=CROP, pad_values=[0, NSEG], padding=(124, 116, 104), pad_if_needed=True),
                        et.ExtRandomHorizontalFlip(),
                        et.ExtColorJitter(*jitter, p=p_jitter),
                        et.ExtRandomGrayscale(p=p_gray),
                        et.ExtToTensor(dtype_list=['uint8', 'int']),
                        et.ExtNormalize(mean=MEAN, std=STD)])
    random.seed(py_seed)
    torch.manual_seed(torch_seed)
    ColorJitter.last = None
    t, (tl, ts) = tf(Image.fromarray(img), [Image.fromarray(lbl), Image.fromarray(spx).convert('I')])
    return t.numpy(), tl.numpy().astype(np.uint8), ts.numpy().astype(np.int32), ColorJitter.last, RandomGrayscale.last


def save_fixed(path, arrays):
    """``np.savez_compressed`` with fixed member dates (numpy stamps the members with the clock)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(1)
    et = reference_ext_transforms()
    pics = [picture(k) for k in range(N_PICTURES)]
    samples = []          # (kind, py_seed, torch_seed, jitter, p_jitter, p_gray)

    def scale_of(k):
        return (0.5, 0.78) if k % 2 else (0.5, 2.0)

    def sample(kind, torch_seed, jitter, p_jitter, p_gray):
        k = len(samples)
        return (kind, 500 + k, torch_seed, jitter, p_jitter, p_gray, scale_of(k), k % N_PICTURES)

    def execute(s):
        _, py_seed, torch_seed, jitter, p_jitter, p_gray, scale_range, pic = s
        return run(et, pics[pic], py_seed, torch_seed, jitter, p_jitter, p_gray, scale_range)

    # 1. the reference's probabilities: scan torch seeds in order until the quota of every category is filled
    quota = {(True, False): 5, (False, True): 2, (True, True): 1, (False, False): 4}
    seed = 0
    while sum(quota.values()):
        s = sample('ref', seed, STRONG, 0.2, 0.2)
        _, _, _, jit, grey = execute(s)
        cat = (jit is not None, bool(grey))
        if quota[cat]:
            quota[cat] -= 1
            samples.append(s)
        seed += 1
    # 2. all 24 orders at p = 1: the first torch seed that yields each permutation
    for perm in itertools.permutations(range(4)):
        seed = 0
        while True:
            torch.manual_seed(seed)
            torch.rand(1)
            if tuple(int(v) for v in torch.randperm(4)) == perm:
                break
            seed += 1
        samples.append(sample('order', seed, STRONG, 1.0, 1.0 if len(samples) % 4 == 0 else 0.0))
    # 3. one sample per single op, the widest hue range, grey alone
    for j, jitter in enumerate(((0.4, 0, 0, 0), (0, 0.4, 0, 0), (0, 0, 0.4, 0), (0, 0, 0, 0.1), (0, 0, 0, 0.5))):
        samples.append(sample('single', 40 + j, jitter, 1.0, 0.0))
    samples.append(sample('grey', 50, STRONG, 0.0, 1.0))

    out = dict(H=H, W=W, crop=np.asarray(CROP), nseg=NSEG, mean=np.asarray(MEAN), std=np.asarray(STD),
               pictures=np.stack([p[0] for p in pics]), labels=np.stack([p[1] for p in pics]), spx=np.stack([p[2] for p in pics]))
    rows, orders, factors, kinds = [], [], [], []
    images, lbls, spxs = [], [], []
    n_pad = 0
    for k, s in enumerate(samples):
        kind, py_seed, torch_seed, jitter, p_jitter, p_gray, scale_range, pic = s
        t, tl, ts, jit, grey = execute(s)
        images.append(t), lbls.append(tl), spxs.append(ts)
        padded = bool((ts == NSEG).any())
        n_pad += padded
        kinds.append(kind)
        rows.append([py_seed, torch_seed, pic, *jitter, p_jitter, p_gray, *scale_range, int(jit is not None), int(grey), int(padded)])
        orders.append(jit[0] if jit else [-1] * 4)
        factors.append([np.nan if v is None else v for v in jit[1]] if jit else [np.nan] * 4)
        print("g13 %2d %-6s seeds (%d, %d) picture %d jitter %s order %s grey %d pad %d"
              % (k, kind, py_seed, torch_seed, pic, jit is not None, orders[-1], grey, padded))
    rows = np.asarray(rows, dtype=np.float64)
    ref = rows[[k == 'ref' for k in kinds]]
    jit_, grey_ = ref[:, 11] == 1, ref[:, 12] == 1
    assert len(ref) == 12 and jit_.sum() >= 4 and grey_.sum() >= 2 and (jit_ & grey_).any() and (~jit_ & ~grey_).any()
    assert len({tuple(o) for o, k in zip(orders, kinds) if k == 'order'}) == 24
    assert 2 * n_pad >= len(samples), "pad fill on at least half the samples"
    out.update(kinds=np.asarray(kinds), samples=rows, orders=np.asarray(orders, dtype=np.int32), factors=np.asarray(factors, dtype=np.float64),
               columns=np.asarray(['py_seed', 'torch_seed', 'picture', 'brightness', 'contrast', 'saturation', 'hue', 'p_jitter', 'p_gray',
                                   'scale_lo', 'scale_hi', 'jittered', 'grey', 'padded']),
               images=np.stack(images), out_labels=np.stack(lbls), out_spx=np.stack(spxs))
    import PIL
    out['pillow'] = np.str_(PIL.__version__)
    save_fixed(OUT, out)
    print("g13: %d samples, %d with pad fill; wrote %s (%d bytes)" % (len(samples), n_pad, OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
