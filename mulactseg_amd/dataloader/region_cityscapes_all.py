"""The loader of ``script/open_source/eval_city_mul_res50.sh`` -- the reference's ``dataloader/region_cityscapes_all.py``
(``--loader region_cityscapes_all --train_transform eval_spx``).

The module exports two names, as the reference's does:
* ``RegionCityscapes`` is ``region_cityscapes.RegionCityscapes`` itself (the reference imports it at module level), so
  ``get_active_dataset`` without ``--or_labeling`` builds plain ``RegionCityscapes`` pool and label sets for this loader -- what the
  evaluation script runs on;
* ``RegionCityscapesAll``: per picture, for every id the region dict lists, the classes of the region by pixel count
  (``superpixel_info``).  The per-id label histograms are one launch of ``ops.region_label_counts`` (``csrc/labels.hip``, no
  trimming) on the resized maps; ``[nseg, C + 1]`` is read back once per picture and the lists are built on the host.

Entries of ``superpixel_info[id]`` (the reference's loop, :39-54, one ``np.unique`` per id):
``cls`` / ``cpx`` the non-ignore classes and their pixel counts by descending count, ties in the order of numpy's
``c.argsort()[::-1]`` over the classes in ascending order; ``npx`` the pixel count; ``isignore`` whether a pixel is 255;
``allignore = all(u != 255)`` -- True when the region has NO ignore pixel, and then ``cls`` and ``cpx`` are ``[]`` (the reference's
inverted flag, kept as it is: INTEGRATION.md section 5).  An id without pixels gets ``npx = 0``, ``isignore = False``,
``allignore = True``."""
import numpy as np
import torch

from .. import ops
from .region_cityscapes import RegionCityscapes


class RegionCityscapesAll(RegionCityscapes):
    def __init__(self, args, root, datalist, split='train', transform=None, region_dict="dataloader/init_data/cityscapes/train.dict",
                 store=None):
        super().__init__(args, root, datalist, split, transform, False, region_dict, True, False, store=store)

    def __getitem__(self, index):
        img_fname, lbl_fname, spx_fname = self.im_idx[index]
        _, (target, superpixel) = self.transform(self.store.picture(img_fname), [self.store.labelmap(lbl_fname), self.store.idmap(spx_fname)])
        target = self._encode_on_device(target).to(torch.uint8)           # training ids 0 .. C-1 and 255
        C, nseg = self.args.num_classes, self.args.nseg
        ids = self.suppix.get(spx_fname, [])
        if len(ids) and (min(ids) < 0 or max(ids) >= nseg):
            raise ValueError("listed superpixel ids must be in [0, %d)" % nseg)
        full, _ = ops.region_label_counts(target.contiguous(), superpixel.contiguous(), nseg, C)
        counts = full.cpu().numpy().astype(np.int64)                       # [nseg, C + 1], last column: 255
        return {'superpixel_info': {p: region_info(counts[p], C) for p in ids}, 'fname': self.im_idx[index]}


def region_info(row, C):
    """The entry of one region from its label histogram ``row`` int64 [C + 1] (column C: label 255)."""
    isignore = bool(row[C] > 0)
    allignore = not isignore
    cls, cpx = [], []
    if not allignore:
        u_valid = np.flatnonzero(row[:C])
        c_valid = row[u_valid]
        order = c_valid.argsort()[::-1]
        cls, cpx = u_valid[order].tolist(), c_valid[order].tolist()
    return {'cls': cls, 'cpx': cpx, 'npx': int(row.sum()), 'isignore': isignore, 'allignore': allignore}
