"""Training transforms by name -- the reference's ``dataloader/transform.py:5-170`` (Cityscapes) and
``dataloader/transform_voc.py:5-224`` (VOC) -- built on the device augmentation (``device_transforms.py``,
``csrc/augment.hip``): the names the launch scripts use (``script/**/*.sh``: ``rescale_769_multi_notrg``, ``rescale_769_nospx``,
``rescale_513_multi_notrg``, ``rescale_513_notrg``, ``eval_spx``, ``eval_dom_gt_spx``) plus the other names with the same structure.  A transform is
called as ``transform(picture u8 [H,W,3] cuda, [maps]) -> (image f32 [3,h,w], [maps])``; ``transform.n_maps`` says how many maps
it pads (``ExtRandomCrop.pad_values``; the reference asserts the same count, ``ext_transforms.py:489``).

The suffix ``_strongv1`` adds the reference's photometric stage after crop and flip -- ``ExtColorJitter(0.4, 0.4, 0.4, 0.1, p=0.2)``
then ``ExtRandomGrayscale(p=0.2)`` (``transform.py:139-153``) -- to the crops above: ``DeviceTrainAugmentStrong``,
``csrc/photometric.hip``, bit-identical to torchvision 0.12 on the installed Pillow (12.2.0 is what the tests pin; the reference
pins 9.2.0).  The geometry draws stay on Python's ``random``, the photometric draws come from torch's global CPU generator, as in
the reference.  ``rescale_769_multi_notrg_ignore_strongv1`` is the reference's own name; the other ``_strongv1`` names apply the
same stage to the other built crops.

``--load_smaller_spx`` (the finer superpixel map of the hierarchical group loss) is taken by ``rescale_769_multi_notrg`` alone, where
it is the second of two maps [superpixel, small], padded with [nseg, small_nseg]; the names that would need a THIRD map
(``rescale_769_multi``, ``..._ignore``) and every ``_strongv1`` name refuse it in ``get_train_transform``.  The one loader whose
samples carry three maps, ``region_cityscapes_or_tensor_ignore_async``, gets ``rescale_769_multi_notrg_ignore`` with [label, superpixel,
small] from ``get_async_train_transform`` (``get_active_dataset`` calls it for that loader).

Not offered (outside the production configurations): the unpadded 512x1024 crops (``orig_*``, ``rescale``).  ``eval_spx_identity`` (VOC) keeps the picture and its two maps at their own size;
``eval_spx_identity_ms`` (VOC) returns a LIST of ten pictures (five scales, then the same
flipped) and takes no map (``n_maps == 0``)."""
from .device_transforms import (DeviceIdentity, DeviceMultiScaleFlip, DeviceResize, DeviceResizeFlip, DeviceResizeThreeMaps, DeviceTrainAugment,
                                DeviceTrainAugmentStrong, DeviceTrainAugmentThreeMaps)

STRONG_V1 = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p_jitter=0.2, p_gray=0.2)


def _with_maps(t, n):
    t.n_maps = n
    return t


def _no_small(args, name):
    if getattr(args, 'load_smaller_spx', False):
        raise NotImplementedError("train_transform %r with --load_smaller_spx (a third map) is outside the hot path" % name)


def get_async_train_transform(args, transform):
    """The training transform of the loader ``region_cityscapes_or_tensor_ignore_async``: the reference's name
    ``rescale_769_multi_notrg_ignore`` with ``--load_smaller_spx`` (``transform.py:115-125``), THREE maps [label padded with 0,
    superpixel, small] through ``DeviceTrainAugmentThreeMaps``.  ``get_train_transform`` keeps refusing that combination for every
    other loader, whose samples carry no third map."""
    if transform != 'rescale_769_multi_notrg_ignore':
        raise NotImplementedError("--loader region_cityscapes_or_tensor_ignore_async takes --train_transform rescale_769_multi_notrg_ignore "
                                  "(three maps: label, superpixel, small), got %r" % (transform,))
    if not getattr(args, 'load_smaller_spx', False):
        raise NotImplementedError("--loader region_cityscapes_or_tensor_ignore_async needs --load_smaller_spx (and --small_nseg)")
    return _with_maps(DeviceTrainAugmentThreeMaps(pad_values=[0, args.nseg, args.small_nseg], size=(768, 768), scale_range=(0.5, 2.0)), 3)


def get_train_transform(args, transform):
    """Cityscapes: 768x768 crops of a U(0.5, 2) rescale, padded with (124, 116, 104) / the per-map pad values.  ``*_strongv1``: the
    same crop followed by colour jitter and grayscale.  ``rescale_769_multi_notrg_ignore_strongv1`` is the reference's name; there it
    ASSERTS ``--load_smaller_spx`` and pads a third map (the smaller superpixels), which is not built: here the name takes the two
    maps [label padded with 0, superpixel] and refuses ``--load_smaller_spx`` like every other name."""
    if transform is None:
        return None
    crop = dict(size=(768, 768), scale_range=(0.5, 2.0))
    if transform == 'rescale_769_nospx':                            # [label]
        return _with_maps(DeviceTrainAugment(pad_values=[args.ignore_idx], **crop), 1)
    if transform == 'rescale_769':                                  # [label, superpixel]
        return _with_maps(DeviceTrainAugment(pad_values=[args.ignore_idx, args.nseg], **crop), 2)
    if transform == 'rescale_769_multi':
        _no_small(args, transform)
        return _with_maps(DeviceTrainAugment(pad_values=[args.ignore_idx, args.nseg], **crop), 2)
    if transform == 'rescale_769_multi_notrg':                      # [superpixel]: the stage-1 production transform
        if getattr(args, 'load_smaller_spx', False):                # [superpixel, small] (transform.py:96-110 of the reference)
            return _with_maps(DeviceTrainAugment(pad_values=[args.nseg, args.small_nseg], **crop), 2)
        return _with_maps(DeviceTrainAugment(pad_values=[args.nseg], **crop), 1)
    if transform == 'rescale_769_multi_notrg_ignore':               # [label padded with 0, superpixel]
        _no_small(args, transform)
        return _with_maps(DeviceTrainAugment(pad_values=[0, args.nseg], **crop), 2)
    strong = dict(crop, **STRONG_V1)                                # + ExtColorJitter(0.4, 0.4, 0.4, 0.1, p=0.2), ExtRandomGrayscale(p=0.2)
    if transform == 'rescale_769_nospx_strongv1':
        return _with_maps(DeviceTrainAugmentStrong(pad_values=[args.ignore_idx], **strong), 1)
    if transform == 'rescale_769_strongv1':
        return _with_maps(DeviceTrainAugmentStrong(pad_values=[args.ignore_idx, args.nseg], **strong), 2)
    if transform == 'rescale_769_multi_strongv1':
        _no_small(args, transform)
        return _with_maps(DeviceTrainAugmentStrong(pad_values=[args.ignore_idx, args.nseg], **strong), 2)
    if transform == 'rescale_769_multi_notrg_strongv1':
        _no_small(args, transform)
        return _with_maps(DeviceTrainAugmentStrong(pad_values=[args.nseg], **strong), 1)
    if transform == 'rescale_769_multi_notrg_ignore_strongv1':
        # The reference's name (transform.py:139-153).  The reference ASSERTS --load_smaller_spx there and pads a third map
        # (the smaller superpixels); that map is not built, so the name is offered with the two maps [label padded with 0,
        # superpixel] of 'rescale_769_multi_notrg_ignore' and --load_smaller_spx is refused as for every other name.
        _no_small(args, transform)
        return _with_maps(DeviceTrainAugmentStrong(pad_values=[0, args.nseg], **strong), 2)
    if transform == 'eval_spx':                                     # ExtResize((1024, 2048)), two maps
        return _with_maps(DeviceResize((1024, 2048), pad_values=[args.ignore_idx, args.nseg]), 2)
    if transform == 'eval_dom_gt_spx':                              # ExtResize((1024, 2048)), three maps: dominant target, label, ids
        return _with_maps(DeviceResizeThreeMaps((1024, 2048), pad_values=[args.ignore_idx, args.ignore_idx, args.nseg]), 3)
    raise NotImplementedError("train_transform %r is outside the hot path (see dataloader/transform.py)" % transform)


def get_train_transform_voc(args, transform):
    """VOC: 513x513 crops."""
    if transform is None:
        return None
    crop = dict(size=(513, 513), scale_range=(0.5, 2.0))
    if transform == 'rescale_769_nospx':                            # resize 513 + centre crop 513 + flip, [label]
        return _with_maps(DeviceResizeFlip(513, center_crop=513, pad_values=[args.ignore_idx]), 1)
    if transform == 'rescale_513_notrg':                            # [label]
        return _with_maps(DeviceTrainAugment(pad_values=[args.ignore_idx], **crop), 1)
    if transform == 'rescale_513':                                  # [label, superpixel]
        return _with_maps(DeviceTrainAugment(pad_values=[args.ignore_idx, args.nseg], **crop), 2)
    if transform == 'rescale_513_multi_notrg':                      # [superpixel]
        _no_small(args, transform)
        return _with_maps(DeviceTrainAugment(pad_values=[args.nseg], **crop), 1)
    strong = dict(crop, **STRONG_V1)                                # the photometric stage of the Cityscapes '_strongv1' names
    if transform == 'rescale_513_notrg_strongv1':
        return _with_maps(DeviceTrainAugmentStrong(pad_values=[args.ignore_idx], **strong), 1)
    if transform == 'rescale_513_strongv1':
        return _with_maps(DeviceTrainAugmentStrong(pad_values=[args.ignore_idx, args.nseg], **strong), 2)
    if transform == 'rescale_513_multi_notrg_strongv1':
        _no_small(args, transform)
        return _with_maps(DeviceTrainAugmentStrong(pad_values=[args.nseg], **strong), 1)
    if transform == 'eval_spx':
        return _with_maps(DeviceResize(513, center_crop=513, pad_values=[args.ignore_idx, args.nseg]), 2)
    if transform == 'eval_spx_identity':                            # ToTensor + Normalize at the picture's own size, [label, superpixel]
        return _with_maps(DeviceIdentity(pad_values=[args.ignore_idx, args.nseg]), 2)
    if transform == 'eval_spx_identity_ms':                         # TestTimeAugmentation: 5 scales x {no flip, flip}, picture only
        return _with_maps(DeviceMultiScaleFlip(), 0)
    raise NotImplementedError("train_transform %r is outside the hot path (see dataloader/transform.py)" % transform)


def get_val_transform(name, n_maps=1, ignore_idx=255, nseg=2048):
    """The pool / validation / evaluation transform of ``dataloader/__init__.py:38-78,124-136,156-170``."""
    pads = [ignore_idx, nseg]            # (never applied: a resize / centre crop pads nothing)
    if name == 'cityscapes':
        return _with_maps(DeviceResize((1024, 2048), pad_values=pads), n_maps)
    if name == 'voc':
        return _with_maps(DeviceResize(513, center_crop=513, pad_values=pads), n_maps)
    raise NotImplementedError(name)
