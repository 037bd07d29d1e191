"""The labelled set of the cross-view hierarchical group loss -- the reference's
``dataloader/region_cityscapes_or_tensor_ignore_async.py:11-73`` (``--loader region_cityscapes_or_tensor_ignore_async
--train_transform rescale_769_multi_notrg_ignore --load_smaller_spx``; trainers ``active_joint_hier_multi_async`` / ``..._async_weight``).

A labelled sample is the ``region_cityscapes_or_tensor`` sample in TWO views of one picture:

* the strong view: the training augmentation of the picture and of three maps -- the precise ``gtFine_labelIds`` picture (padded with
  0), the superpixel ids (padded with ``nseg``) and the finer ids (padded with ``small_nseg``): ``images``, ``spx``, ``spx_small``;
* the weak view: ``ExtResize((1024, 2048))``, to-tensor, normalise of the same picture and maps, no random draw: ``image_weak``,
  ``spx_weak``, ``spx_small_weak``.

In both views the mask (``spmask``, ``spmask_weak``) is "superpixel selected" AND "ground-truth training id != 255"; the label
picture is encoded to training ids on the device.  ``labels`` is the multi-hot row table of the picture, as in the parent.  Without
``--load_smaller_spx`` the reference raises (``:50-51``), and so does the constructor here.  Pool samples (``active-ulabel``) are the
parent's.  Both views resample the picture once; the third map of each goes through the map-only augmentation entry."""
from . import region_cityscapes_or_tensor
from .device_transforms import DeviceTrainAugmentThreeMaps

WEAK_SIZE = (1024, 2048)


class RegionCityscapesOr(region_cityscapes_or_tensor.RegionCityscapesOr):
    def __init__(self, args, root, datalist, split='train', transform=None, return_spx=False,
                 region_dict=None, mask_region=True, dominant_labeling=False, loading='binary', load_smaller_spx=False, store=None,
                 weak_size=WEAK_SIZE):
        super().__init__(args, root, datalist, split, transform, return_spx, region_dict, mask_region, dominant_labeling, loading,
                         load_smaller_spx, store=store)
        if split != 'active-ulabel':
            if not self.load_smaller_spx:
                raise NotImplementedError("--loader region_cityscapes_or_tensor_ignore_async needs --load_smaller_spx (and --small_nseg)")
            if not isinstance(transform, DeviceTrainAugmentThreeMaps):
                raise ValueError("--loader region_cityscapes_or_tensor_ignore_async augments three maps: --train_transform "
                                 "rescale_769_multi_notrg_ignore")
        self.weak_transform = DeviceTrainAugmentThreeMaps(pad_values=[0, args.nseg, getattr(args, 'small_nseg', args.nseg)])
        self.weak_size = weak_size

    @property
    def weak_size(self):
        """(height, width) the weak view is resized to -- ``ExtResize((1024, 2048))`` in the reference."""
        return self.weak_transform.size

    @weak_size.setter
    def weak_size(self, size):
        self.weak_transform.size = (int(size[0]), int(size[1]))

    def sample_files(self, index):
        files = super().sample_files(index)
        if self.split != 'active-ulabel':
            files.append(('map', self.precise_label_file(self.im_idx[index][1])))
        return files

    def weak_view(self, picture, maps):
        """The deterministic resize to ``weak_size``: the augmentation's geometry with no padding, crop or flip; no draw is consumed."""
        th, tw = self.weak_size
        return self.weak_transform(picture, maps, params=dict(scale=1.0, th=th, tw=tw, gap_y=0, gap_x=0, i=0, j=0, flip=False))

    def view_mask(self, spx_fname, precise, superpixel):
        """selected superpixel AND a ground-truth training id other than 255 (:56-59, :63-66)"""
        return self.selection_mask(spx_fname, superpixel) & (self._encode_on_device(precise) != 255)

    def __getitem__(self, index):
        if self.split == 'active-ulabel':
            return super().__getitem__(index)
        assert self.mask_region
        img_fname, lbl_fname, spx_fname = self.im_idx[index]
        picture = self.store.picture(img_fname)
        maps = [self.store.labelmap(self.precise_label_file(lbl_fname)), self.store.idmap(spx_fname),
                self.store.idmap(self.small_spx_fname(spx_fname))]
        image_weak, (precise_weak, spx_weak, small_weak) = self.weak_view(picture, maps)
        image, (precise, superpixel, small) = self.transform(picture, maps)
        return {'images': image, 'image_weak': image_weak, 'labels': self.multi_hot_row(lbl_fname, image.device),
                'spx': superpixel, 'spx_weak': spx_weak, 'spmask': self.view_mask(spx_fname, precise, superpixel),
                'spmask_weak': self.view_mask(spx_fname, precise_weak, spx_weak), 'spx_small': small, 'spx_small_weak': small_weak,
                'fnames': self.im_idx[index]}
