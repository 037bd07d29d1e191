"""The labelled set of the dominant-label stage-2 ablation (paper Fig. 7 (b)) -- the reference's
``dataloader/region_cityscapes_dom_w_gt.py`` (``--loader region_cityscapes_dom_w_gt --train_transform eval_dom_gt_spx
--dominant_labeling``): per picture the dominant-label map of the datalist (``target``, 255 outside the selected superpixels), the
precise ground truth (``labels``, training ids, only for the IoU of the generated labels), the superpixel ids and the selection mask.
``pred_ignore`` (``'predignore'`` in ``--init_checkpoint``, a substring test on the path as in the reference) turns 255 into class
19 in both maps before the selection is applied; without it the precise labels keep 255 (unlike ``eval_region_cityscapes_all``).
The three maps are resampled together (``DeviceResizeThreeMaps``, one set of nearest tables)."""
import torch

from . import region_cityscapes


def pred_ignore_of(args):
    return 'predignore' in args.init_checkpoint


class RegionCityscapes(region_cityscapes.RegionCityscapes):
    def __init__(self, args, root, datalist, split='train', transform=None, return_spx=False,
                 region_dict=None, mask_region=True, dominant_labeling=False, store=None):
        super().__init__(args, root, datalist, split, transform, return_spx, region_dict, mask_region, dominant_labeling, store=store)
        assert self.dominant_labeling
        self.pred_ignore = pred_ignore_of(args)

    def sample_files(self, index):
        img, lbl, spx = self.im_idx[index]
        return [('rgb', img), ('map', lbl), ('map', self.precise_label_file(lbl)), ('ids', spx)]

    def __getitem__(self, index):
        img_fname, lbl_fname, spx_fname = self.im_idx[index]
        maps = [self.store.labelmap(lbl_fname), self.store.labelmap(self.precise_label_file(lbl_fname)), self.store.idmap(spx_fname)]
        image, (target, precise, superpixel) = self.transform(self.store.picture(img_fname), maps)
        target = target.long()
        label = self._encode_on_device(precise)
        if self.pred_ignore:                                        # the original "ignore" as the 19th class (:506-520)
            target = torch.where(target == 255, torch.full_like(target, 19), target)
            label = torch.where(label == 255, torch.full_like(label, 19), label)
        sp_mask = self.selection_mask(spx_fname, superpixel)
        target = torch.where(sp_mask, target, torch.full_like(target, 255))
        return {'images': image, 'target': target, 'labels': label, 'spx': superpixel, 'spmask': sp_mask, 'fnames': self.im_idx[index]}
