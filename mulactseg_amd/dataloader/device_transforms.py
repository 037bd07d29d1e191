"""Training-time augmentation on the device.

Mirror of the reference's training transform ``dataloader/transform.py:105-113``::

    ExtCompose([ExtRandomScale((0.5, 2.0)),
                ExtRandomCrop(size=(768, 768), pad_values=[ignore_idx, nseg], padding=(124, 116, 104), pad_if_needed=True),
                ExtRandomHorizontalFlip(), ExtToTensor(dtype_list=[...]), ExtNormalize(mean, std)])

(``dataloader/ext_transforms.py:172-192, 443-520, 323-341, 384-437``) for pictures and maps that are already resident
in HBM (decoded once; a Cityscapes picture is 6 MB as u8, the whole 2 975-image training set 18.7 GB).  The reference
runs these steps on PIL images in 12 DataLoader workers; here one kernel per sample (``csrc/augment.hip``) writes the
normalised float crop and the cropped maps directly.  Results are bit-identical to Pillow's ``Image.resize``
(BILINEAR / NEAREST) followed by pad, crop, flip, ``to_tensor`` and ``normalize``: the host computes Pillow's
fixed-point coefficient tables in double precision exactly as ``src/libImaging/Resample.c`` does, the kernel applies
them in integer arithmetic.  The random draws are the reference's, in its order, on Python's ``random``:
``uniform`` (scale), ``randint`` x 2 (crop origin; skipped when nothing is left to choose), ``random`` (flip)."""
import math
import random as _random

import numpy as np
import torch

from .. import _lib

PRECISION_BITS = 32 - 8 - 2
_MAP_CODES = {torch.int64: _lib.ID_I64, torch.int32: _lib.ID_I32, torch.int16: _lib.ID_U16, torch.uint8: 3}
if hasattr(torch, "uint16"):
    _MAP_CODES[torch.uint16] = _lib.ID_U16


def bilinear_tables(in_size, out_size):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for BILINEAR over a whole axis, vectorised over the
    output index with the per-element operation order of the C loop.  -> (bounds int32 [out,2], kk int32 [out,ksize])."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int) truncates toward zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        live = x < xmax
        v = np.abs((x + xmin - center + 0.5) * ss)
        f = np.where(live & (v < 1.0), 1.0 - v, 0.0)
        w[:, x] = f
        ww = ww + f                                                          # sequential, as in the C loop
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz, None]
    kk = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)   # weights are >= 0: truncation = floor
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    return bounds, kk


def nearest_table(in_size, out_size):
    """Source index per output index of Pillow's NEAREST resize (``Geometry.c:ImagingScaleAffine``): the coordinate
    starts at a/2 and advances by repeated double additions of a = in/out (a cumulative sum, not a multiplication)."""
    a = in_size / out_size
    steps = np.full(out_size, a, dtype=np.float64)
    steps[0] = a * 0.5
    xo = np.cumsum(steps)
    return np.minimum(xo.astype(np.int64), in_size - 1).astype(np.int32)


class _PinnedRing:
    """Page-locked staging slots for the per-sample coefficient tables: a copy from pageable memory blocks the host until
    the stream's earlier work has drained, so a prefetching provider would serialise with its own augmentation kernels;
    from a pinned slot the copy is only enqueued.  A slot is reused after the event recorded behind its copy."""

    def __init__(self, slots=8):
        self.bufs, self.events, self.k = [None] * slots, [None] * slots, 0

    def upload(self, arr, device):
        k, self.k = self.k, (self.k + 1) % len(self.bufs)
        if self.events[k] is not None:
            self.events[k].synchronize()
        n = int(arr.size)
        if self.bufs[k] is None or self.bufs[k].numel() < n:
            self.bufs[k] = torch.empty(max(n, 1 << 15), dtype=torch.int32).pin_memory()
        host = self.bufs[k][:n]
        host.numpy()[:] = arr
        dev = torch.empty(n, dtype=torch.int32, device=device)
        dev.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self.events[k] = ev
        return dev


def draw_params(rng, H, W, crop, scale_range=(0.5, 2.0), p_flip=0.5):
    """The reference's random draws, in its order (``ext_transforms.py:186-187, 470-474, 339``)."""
    scale = rng.uniform(scale_range[0], scale_range[1])
    th, tw = int(H * scale), int(W * scale)
    gap_y = int(math.ceil((crop[0] - th) / 2)) if th < crop[0] else 0
    gap_x = int(math.ceil((crop[1] - tw) / 2)) if tw < crop[1] else 0
    ph, pw = th + 2 * gap_y, tw + 2 * gap_x
    if pw == crop[1] and ph == crop[0]:
        i = j = 0
    else:
        i = rng.randint(0, ph - crop[0])
        j = rng.randint(0, pw - crop[1])
    flip = rng.random() < p_flip
    return dict(scale=scale, th=th, tw=tw, gap_y=gap_y, gap_x=gap_x, i=i, j=j, flip=bool(flip))


class DeviceTrainAugment:
    """``transform(img_u8[H,W,3] cuda, [map, ...] cuda) -> (image f32 [3,ch,cw], [maps])`` -- up to two maps
    (label, superpixel ids), int64 out (uint8 in -> uint8 out when ``keep_u8``)."""

    def __init__(self, size=(768, 768), scale_range=(0.5, 2.0), pad_values=(255, 2048), fill=(124, 116, 104),
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), rng=None, keep_u8=True):
        self.size = (int(size), int(size)) if isinstance(size, int) else tuple(int(v) for v in size)
        self.scale_range = scale_range
        self.pad_values = list(pad_values)
        self.fill = (np.asarray(fill, dtype=np.uint8))
        self.mean = np.asarray(mean, dtype=np.float32)
        self.std = np.asarray(std, dtype=np.float32)
        self.rng = rng if rng is not None else _random
        self.keep_u8 = keep_u8
        self._ring = _PinnedRing()

    def _prepare(self, img, maps, params):
        """Checks, draws (unless ``params``), coefficient tables and map outputs of one sample -> (params, the geometry arguments
        up to ``out_w`` of the augmentation entries, the map arguments, the map outputs, the table tensor to keep alive)."""
        if not (img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.is_contiguous()):
            raise ValueError("picture must be a contiguous uint8 [H,W,3] tensor on the GPU")
        maps = list(maps)
        if len(maps) > 2 or len(maps) > len(self.pad_values):
            raise ValueError("at most two maps, each with a pad value")
        H, W = int(img.shape[0]), int(img.shape[1])
        for m in maps:
            if not (m.is_cuda and tuple(m.shape) == (H, W) and m.dtype in _MAP_CODES and m.is_contiguous()):
                raise ValueError("maps must be contiguous [H,W] integer tensors on the picture's device")
        p = params if params is not None else self._draw(H, W)
        th, tw = p['th'], p['tw']
        hb, hk = bilinear_tables(W, tw)
        vb, vk = bilinear_tables(H, th)
        xi, yi = nearest_table(W, tw), nearest_table(H, th)
        parts = [hb.ravel(), hk.ravel(), vb.ravel(), vk.ravel(), xi, yi]
        offs = np.cumsum([0] + [a.size for a in parts])
        tab = self._ring.upload(np.concatenate(parts).astype(np.int32, copy=False), img.device)   # one small pinned H2D copy
        ptr = [tab.data_ptr() + 4 * int(o) for o in offs[:-1]]
        ch, cw = self.size
        outs, margs = [], []
        for k in range(2):
            if k < len(maps):
                u8 = self.keep_u8 and maps[k].dtype == torch.uint8
                o = torch.empty((ch, cw), dtype=torch.uint8 if u8 else torch.int64, device=img.device)
                outs.append(o)
                margs += [maps[k].data_ptr(), _MAP_CODES[maps[k].dtype], int(self.pad_values[k]), o.data_ptr(), int(u8)]
            else:
                margs += [None, 0, 0, None, 0]
        geom = [img.data_ptr(), H, W, th, tw, ptr[0], ptr[1], hk.shape[1], ptr[2], ptr[3], vk.shape[1], ptr[4], ptr[5],
                p['gap_y'], p['gap_x'], p['i'], p['j'], int(p['flip']), ch, cw]
        return p, geom, margs, outs, tab

    def _draw(self, H, W):
        return draw_params(self.rng, H, W, self.size, self.scale_range)

    def __call__(self, img, maps=(), params=None):
        p, geom, margs, outs, tab = self._prepare(img, maps, params)
        ch, cw = self.size
        out = torch.empty((3, ch, cw), dtype=torch.float32, device=img.device)
        lib = _lib.load()
        with torch.cuda.device(img.device):
            st = torch.cuda.current_stream(img.device).cuda_stream
            _lib.check(lib.mas_train_augment(*geom, self.mean.ctypes.data, self.std.ctypes.data, self.fill.ctypes.data, *margs,
                                             out.data_ptr(), st), "mas_train_augment")
        tab.record_stream(torch.cuda.current_stream(img.device))
        return out, outs


class DeviceTrainAugmentThreeMaps(DeviceTrainAugment):
    """``DeviceTrainAugment`` with THREE maps (``rescale_769_multi_notrg_ignore`` with ``--load_smaller_spx``, ``transform.py:115-125``
    of the reference: precise label, superpixel ids, finer superpixel ids).  The main launch takes the picture and the first two maps;
    the third map goes through the map-only entry (``mas_train_augment_maps``) with the draws and the NEAREST tables of that launch, so
    the picture is resampled once.  The random draws are those of the two-map transform, in the same order.  With ``params`` given
    (``DeviceResize.geometry``) it is the deterministic resize of the same three maps."""

    def __init__(self, pad_values=(0, 2048, 8192), **kw):
        pads = list(pad_values)
        if len(pads) != 3:
            raise ValueError("three maps, three pad values")
        super().__init__(pad_values=pads[:2], **kw)
        self.third_pad = pads[2]

    @property
    def all_pad_values(self):
        return list(self.pad_values) + [self.third_pad]

    def __call__(self, img, maps=(), params=None):
        maps = list(maps)
        if len(maps) != 3:
            raise ValueError("the three-map augmentation takes exactly three maps, got %d" % len(maps))
        third = maps[2]
        H, W = int(img.shape[0]), int(img.shape[1])
        if not (third.is_cuda and tuple(third.shape) == (H, W) and third.dtype in _MAP_CODES and third.is_contiguous()):
            raise ValueError("maps must be contiguous [H,W] integer tensors on the picture's device")
        p, geom, margs, outs, tab = self._prepare(img, maps[:2], params)
        ch, cw = self.size
        out = torch.empty((3, ch, cw), dtype=torch.float32, device=img.device)
        u8 = self.keep_u8 and third.dtype == torch.uint8
        o3 = torch.empty((ch, cw), dtype=torch.uint8 if u8 else torch.int64, device=img.device)
        lib = _lib.load()
        with torch.cuda.device(img.device):
            st = torch.cuda.current_stream(img.device).cuda_stream
            _lib.check(lib.mas_train_augment(*geom, self.mean.ctypes.data, self.std.ctypes.data, self.fill.ctypes.data, *margs,
                                             out.data_ptr(), st), "mas_train_augment")
            # geom: img, H, W, th, tw, hb, hk, hks, vb, vk, vks, xidx, yidx, gap_y, gap_x, i, j, flip, out_h, out_w
            _lib.check(lib.mas_train_augment_maps(*geom[1:5], *geom[11:20], third.data_ptr(), _MAP_CODES[third.dtype], int(self.third_pad),
                                                  o3.data_ptr(), int(u8), None, 0, 0, None, 0, st), "mas_train_augment_maps")
        tab.record_stream(torch.cuda.current_stream(img.device))
        return out, outs + [o3]


def _jitter_range(value, center=1.0, clip_first_on_zero=True):
    """torchvision 0.12 ``ColorJitter._check_input`` for a number: ``[center - v, center + v]`` (the first clipped at 0);
    ``None`` when the range collapses to its centre (nothing is drawn then)."""
    if value < 0:
        raise ValueError("a jitter strength must be non-negative")
    lo, hi = center - float(value), center + float(value)
    if clip_first_on_zero:
        lo = max(lo, 0.0)
    return None if lo == hi == center else (lo, hi)


def draw_photometric(gen, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p_jitter=0.2, p_gray=0.2):
    """The photometric draws of ``ExtColorJitter(b, c, s, h, p)`` + ``ExtRandomGrayscale(p)`` (reference ``ext_transforms.py:48-88``)
    in the order torchvision 0.12.0 makes them, on torch's CPU generator ``gen`` (``None``: the global one): ``rand(1)`` -- jitter
    unless ``p < u``; then ``randperm(4)`` and one ``uniform_`` each for brightness, contrast, saturation, hue (a component whose
    range collapses draws nothing); then ``rand(1) < p_gray``, always drawn.
    -> ``dict(order=[4 ints] or None, factors=[b, c, s, h] with None for an absent op, grey=bool)``; ``order is None``: no jitter."""
    ranges = [_jitter_range(brightness), _jitter_range(contrast), _jitter_range(saturation),
              _jitter_range(hue, center=0.0, clip_first_on_zero=False)]
    if not 0 <= hue <= 0.5:
        raise ValueError("hue must lie in [0, 0.5]")
    order, factors = None, [None] * 4
    if not bool(p_jitter < torch.rand(1, generator=gen)):
        order = [int(v) for v in torch.randperm(4, generator=gen)]
        factors = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1], generator=gen)) for r in ranges]
    grey = bool(torch.rand(1, generator=gen) < p_gray)
    return dict(order=order, factors=factors, grey=grey)


def _chain_args(photometric):
    """-> (order int32[4], factor float32[4], present bits, grey) of the C entries."""
    order = photometric.get('order')
    factors = photometric.get('factors') or [None] * 4
    present = 0
    if order is not None:
        for k, f in enumerate(factors):
            present |= (f is not None) << k
    o = np.asarray(order if order is not None else range(4), dtype=np.int32)
    f = np.asarray([0.0 if v is None else v for v in factors], dtype=np.float32)
    return o, f, int(present), int(bool(photometric.get('grey')))


def photometric_reference(crop, photometric, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """``mas_photometric_reference``: the arithmetic of ``csrc/photometric.h`` as a host loop (no GPU) on a uint8 ``[h,w,3]`` numpy
    crop -> (uint8 [h,w,3], float32 [3,h,w], the contrast L sum -- 0 without contrast)."""
    crop = np.ascontiguousarray(crop, dtype=np.uint8)
    h, w = crop.shape[:2]
    o, f, present, grey = _chain_args(photometric)
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    u8 = np.empty((h, w, 3), dtype=np.uint8)
    f32 = np.empty((3, h, w), dtype=np.float32)
    lsum = np.zeros(1, dtype=np.uint32)
    _lib.check(_lib.load().mas_photometric_reference(crop.ctypes.data, h, w, o.ctypes.data, f.ctypes.data, present, grey, mean.ctypes.data,
                                                     std.ctypes.data, u8.ctypes.data, f32.ctypes.data, lsum.ctypes.data),
               "mas_photometric_reference")
    return u8, f32, int(lsum[0])


def photometric(crop, photometric, lsum=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), return_u8=False):
    """``mas_photometric`` (pass 2 of the jittered path) on a uint8 ``[h,w,3]`` crop on the GPU; ``lsum``: the one-element device
    accumulator pass 1 filled (needed when contrast is in the chain) -> float32 ``[3,h,w]`` (and the uint8 result when asked)."""
    if not (crop.is_cuda and crop.dtype == torch.uint8 and crop.dim() == 3 and crop.shape[2] == 3 and crop.is_contiguous()):
        raise ValueError("crop must be a contiguous uint8 [h,w,3] tensor on the GPU")
    h, w = int(crop.shape[0]), int(crop.shape[1])
    o, f, present, grey = _chain_args(photometric)
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    out = torch.empty((3, h, w), dtype=torch.float32, device=crop.device)
    u8 = torch.empty((h, w, 3), dtype=torch.uint8, device=crop.device) if return_u8 else None
    with torch.cuda.device(crop.device):
        st = torch.cuda.current_stream(crop.device).cuda_stream
        _lib.check(_lib.load().mas_photometric(crop.data_ptr(), h, w, o.ctypes.data, f.ctypes.data, present, grey, mean.ctypes.data,
                                               std.ctypes.data, None if lsum is None else lsum.data_ptr(), out.data_ptr(),
                                               None if u8 is None else u8.data_ptr(), st), "mas_photometric")
    return (out, u8) if return_u8 else out


class DeviceTrainAugmentStrong(DeviceTrainAugment):
    """``DeviceTrainAugment`` followed by ``ExtColorJitter(brightness, contrast, saturation, hue, p=p_jitter)`` and
    ``ExtRandomGrayscale(p=p_gray)`` (reference ``transform.py:139-153``, the ``_strongv1`` names), bit-identical to torchvision
    0.12 on the installed Pillow (``csrc/photometric.h``).  The geometry draws stay on ``rng`` (Python's ``random``); the photometric
    draws follow them on ``torch_generator`` (``None``: torch's global CPU generator, as in the reference).  A sample that draws
    neither op takes the parent's single launch; otherwise ``mas_train_augment_u8`` writes the u8 crop, the maps and (for contrast)
    the L sum, and ``mas_photometric`` turns the crop into the normalised picture -- nothing comes back to the host in between.
    ``params`` may carry the photometric draw under ``'photometric'`` (``draw_photometric``'s dictionary)."""

    def __init__(self, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p_jitter=0.2, p_gray=0.2, torch_generator=None, **kw):
        super().__init__(**kw)
        self.jitter = dict(brightness=brightness, contrast=contrast, saturation=saturation, hue=hue, p_jitter=p_jitter, p_gray=p_gray)
        draw_photometric(torch.Generator().manual_seed(0), **self.jitter)          # refuse bad strengths here, not at the first sample
        self.torch_generator = torch_generator

    def _draw(self, H, W):
        p = super()._draw(H, W)
        p['photometric'] = draw_photometric(self.torch_generator, **self.jitter)
        return p

    def _with_photometric(self, params):
        if params is not None and 'photometric' not in params:
            params = dict(params, photometric=draw_photometric(self.torch_generator, **self.jitter))
        return params

    def augment_u8(self, img, maps=(), params=None):
        """Pass 1 alone (``mas_train_augment_u8``) -> (crop uint8 [ch,cw,3], [maps], the one-element L accumulator -- ``None``
        without contrast in the chain)."""
        p, geom, margs, outs, tab = self._prepare(img, maps, self._with_photometric(params))
        o, f, present, _ = _chain_args(p['photometric'])
        ch, cw = self.size
        crop = torch.empty((ch, cw, 3), dtype=torch.uint8, device=img.device)
        lsum = torch.zeros(1, dtype=torch.int32, device=img.device) if (present >> _lib.PM_CONTRAST) & 1 else None
        with torch.cuda.device(img.device):
            st = torch.cuda.current_stream(img.device).cuda_stream
            _lib.check(_lib.load().mas_train_augment_u8(*geom, self.fill.ctypes.data, *margs, o.ctypes.data, f.ctypes.data, present,
                                                        crop.data_ptr(), None if lsum is None else lsum.data_ptr(), st),
                       "mas_train_augment_u8")
        tab.record_stream(torch.cuda.current_stream(img.device))
        return crop, outs, lsum

    def __call__(self, img, maps=(), params=None):
        params = self._with_photometric(params)
        if params is None:
            params = self._draw(int(img.shape[0]), int(img.shape[1])) if img.dim() == 3 else None
        ph = params['photometric'] if params is not None else None
        if ph is None or not (_chain_args(ph)[2] or ph.get('grey')):          # the plain sample: today's single launch
            return super().__call__(img, maps, params=params)
        crop, outs, lsum = self.augment_u8(img, maps, params)
        return photometric(crop, ph, lsum, self.mean, self.std), outs          # (crop and sum live on the stream both passes use)


class DeviceMultiScaleFlip(DeviceTrainAugment):
    """``TestTimeAugmentation`` (``ext_transforms.py:18-46``, name ``eval_spx_identity_ms``): for flip in (False, True), then for each
    factor, the picture resized (Pillow BILINEAR) to ``(int(factor * H), int(factor * W))``, flipped horizontally after the resize
    when ``flip``, to-tensor + normalise -> a list of f32 ``[3,h_k,w_k]`` tensors, the unflipped ones first.  One launch of the
    augmentation kernel per entry (no pad, no crop); factor 1.0 is the exact identity (every bilinear weight is 1).  The picture
    only: labels and ids stay at the original size."""

    def __init__(self, factors=(0.5, 0.75, 1.0, 1.25, 1.5), **kw):
        super().__init__(size=(1, 1), scale_range=(1.0, 1.0), pad_values=(), **kw)
        self.factors = tuple(factors)

    def geometry(self, H, W):
        """[(th, tw, flip)] in the reference's order."""
        return [(int(f * H), int(f * W), flip) for flip in (False, True) for f in self.factors]

    def __call__(self, img, maps=(), params=None):
        if len(maps):
            raise ValueError("the multi-scale transform takes the picture only")
        out = []
        for th, tw, flip in self.geometry(int(img.shape[0]), int(img.shape[1])):
            self.size = (th, tw)
            p = dict(scale=1.0, th=th, tw=tw, gap_y=0, gap_x=0, i=0, j=0, flip=flip)
            out.append(DeviceTrainAugment.__call__(self, img, (), params=p)[0])
        return out


class DeviceIdentity(DeviceTrainAugment):
    """``ExtToTensor`` + ``ExtNormalize`` at the picture's own size (name ``eval_spx_identity``, ``transform_voc.py:212-219``): the
    augmentation kernel at factor 1.0 (every bilinear weight is 1, every nearest index its own), no pad, no crop, no flip -- the
    picture as Pillow's to-tensor + normalise, the label and id maps unchanged."""

    def __init__(self, pad_values=(255, 2048), **kw):
        super().__init__(size=(1, 1), scale_range=(1.0, 1.0), pad_values=pad_values, **kw)

    def __call__(self, img, maps=(), params=None):
        H, W = int(img.shape[0]), int(img.shape[1])
        self.size = (H, W)
        return super().__call__(img, maps, params=dict(scale=1.0, th=H, tw=W, gap_y=0, gap_x=0, i=0, j=0, flip=False))


def get_device_transform(args):
    """The reference's ``'rescale_769_multi'`` training transform (``transform.py:67-89``) for resident data."""
    return DeviceTrainAugment(size=(768, 768), scale_range=(0.5, 2.0), pad_values=[args.ignore_idx, args.nseg])


class DeviceResize(DeviceTrainAugment):
    """The reference's deterministic transforms for pool / validation / evaluation pictures on the same kernel:
    ``ExtResize((h, w))`` (``dataloader/__init__.py:124-136``: Cityscapes to 1024x2048 -- the identity for native pictures, every
    bilinear weight is then exactly 1) or ``ExtResize(s)`` + ``ExtCenterCrop(s)`` (VOC, ``:156-170``: the shorter side to ``s``,
    torchvision's ``int(s * long / short)`` for the other, crop origin ``int(round((side - s) / 2.))``), then to-tensor + normalise.
    No random draw is consumed."""

    def __init__(self, size, center_crop=None, pad_values=(255, 2048), **kw):
        super().__init__(size=(1, 1), scale_range=(1.0, 1.0), pad_values=pad_values, **kw)
        self.target = size
        self.center_crop = center_crop

    def geometry(self, H, W):
        if isinstance(self.target, int):
            s = int(self.target)
            if W <= H:
                tw, th = s, int(s * H / W)
            else:
                th, tw = s, int(s * W / H)
        else:
            th, tw = int(self.target[0]), int(self.target[1])
        if self.center_crop is None:
            return dict(scale=1.0, th=th, tw=tw, gap_y=0, gap_x=0, i=0, j=0, flip=False), (th, tw)
        c = int(self.center_crop)
        if th < c or tw < c:
            raise ValueError("center crop %d larger than the resized picture %dx%d" % (c, th, tw))
        return dict(scale=1.0, th=th, tw=tw, gap_y=0, gap_x=0, i=int(round((th - c) / 2.)), j=int(round((tw - c) / 2.)), flip=False), (c, c)

    def __call__(self, img, maps=(), params=None):
        p, self.size = self.geometry(int(img.shape[0]), int(img.shape[1]))
        return super().__call__(img, maps, params=p)


class DeviceResizeThreeMaps(DeviceResize):
    """``ExtResize((h, w))`` + to-tensor + normalise with THREE maps (name ``eval_dom_gt_spx``, ``transform.py:161-167``: dominant
    target, precise label, superpixel ids), all resampled NEAREST with the same tables.  The augmentation entry takes at most two maps,
    so the third goes through a second launch with the same geometry; that launch also resamples the picture again into a scratch
    tensor (one more picture read and a 3 x h x w f32 write, 25 MB at 1024 x 2048) -- the price of leaving the kernel's entry as it
    is."""

    def __init__(self, size, pad_values=(255, 255, 2048), **kw):
        pads = list(pad_values)
        if len(pads) != 3:
            raise ValueError("three maps, three pad values")
        super().__init__(size, pad_values=pads[:2], **kw)
        self._third = DeviceResize(size, pad_values=pads[2:], **kw)

    def __call__(self, img, maps=(), params=None):
        maps = list(maps)
        if len(maps) != 3:
            raise ValueError("the three-map resize takes exactly three maps, got %d" % len(maps))
        self._third.target = self.target
        image, out = super().__call__(img, maps[:2])
        _, third = self._third(img, maps[2:])
        return image, out + third


class DeviceResizeFlip(DeviceResize):
    """``ExtResize(s)`` + ``ExtCenterCrop(s)`` + ``ExtRandomHorizontalFlip`` -- the VOC stage-2 training transform
    (``transform_voc.py:52-61``, name ``rescale_769_nospx``): one ``random()`` draw per sample."""

    def __call__(self, img, maps=(), params=None):
        p, self.size = self.geometry(int(img.shape[0]), int(img.shape[1]))
        p['flip'] = bool(self.rng.random() < 0.5)
        return DeviceTrainAugment.__call__(self, img, maps, params=p)
