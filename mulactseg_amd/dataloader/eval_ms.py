"""The evaluation list at the pictures' own sizes, as scaled and flipped copies -- the data of ``--method eval_naive_ms`` (multi-scale +
flip evaluation of a checkpoint).  The reference ships no such loader (its README leaves VOC evaluation as a TODO); the pieces are
its own: ``TestTimeAugmentation`` (``ext_transforms.py:18-46``) on the raw picture and the evaluation sets' label encoding
(``dataloader/dataset.py:12-76, 190-278``).

Entry ``i`` of the datalist yields ``image_list`` (``DeviceMultiScaleFlip(factors)`` on the picture: the scales, then the same scales
flipped; without flipping only the first half), ``labels`` (the class map at the picture's own size, no resize and no crop:
Cityscapes ids -> train ids, VOC as stored, 255 stays 255), ``fnames`` and ``imsizes`` (W, H).  Pictures differ in size, so a batch
holds one entry."""
from . import dataset as _ds
from .device_transforms import DeviceMultiScaleFlip

DEFAULT_FACTORS = (0.5, 0.75, 1.0, 1.25, 1.5)


class OwnSizeScales(DeviceMultiScaleFlip):
    """``DeviceMultiScaleFlip`` that can leave the flipped half out."""

    def __init__(self, factors=DEFAULT_FACTORS, flip=True, **kw):
        super().__init__(factors=factors, **kw)
        self.flip = bool(flip)

    def geometry(self, H, W):
        g = super().geometry(H, W)
        return g if self.flip else g[:len(g) // 2]


class _OwnSize:
    def __getitem__(self, index):
        img_fname, lbl_fname = self.im_idx[index][:2]
        picture = self.store.picture(img_fname)
        labels = self.encode_on_device(self.store.labelmap(lbl_fname))
        if tuple(labels.shape) != tuple(picture.shape[:2]):
            raise ValueError("%s is %dx%d, its labels %s are %dx%d" % ((img_fname,) + tuple(picture.shape[:2]) + (lbl_fname,) + tuple(labels.shape)))
        return {'image_list': self.transform(picture), 'labels': labels,
                'imsizes': (int(picture.shape[1]), int(picture.shape[0])), 'fnames': self.im_idx[index]}


class CityscapesOwnSizeMS(_OwnSize, _ds.CityscapesGTA5):
    pass


class VOCOwnSizeMS(_OwnSize, _ds.VOC):
    pass


def get_ms_eval_dataset(name, data_root, datalist, factors=DEFAULT_FACTORS, flip=True, store=None):
    """The evaluation set of ``name`` ('cityscapes' or 'voc') over ``datalist`` with ``len(factors) * (2 if flip else 1)`` copies per
    picture."""
    if name not in ("cityscapes", "voc"):
        raise NotImplementedError("multi-scale evaluation of %r (cityscapes or voc)" % (name,))
    factors = tuple(float(f) for f in factors)
    if not factors or min(factors) <= 0:
        raise ValueError("scale factors must be positive, got %r" % (factors,))
    cls = CityscapesOwnSizeMS if name == "cityscapes" else VOCOwnSizeMS
    return cls(data_root, datalist, 'eval', transform=OwnSizeScales(factors, flip), store=store)
