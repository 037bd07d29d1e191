"""The VOC labelled set as the multi-scale stage-2 generator reads it -- the reference's ``dataloader/eval_region_voc_all_ms.py:10-80``:
``eval_region_voc_all`` with the picture through ``TestTimeAugmentation`` (``train_transform eval_spx_identity_ms``: ten tensors,
five scales then the same flipped) and the class PNG (255 -> class 21), the id map and the mask at the picture's original size."""
import torch

from . import eval_region_voc_all


class RegionVOCOr(eval_region_voc_all.RegionVOCOr):
    def __getitem__(self, index):
        img_fname, lbl_fname, spx_fname = self.im_idx[index]
        picture = self.store.picture(img_fname)
        images = self.transform(picture)
        precise = self.store.labelmap(self.precise_label_file(lbl_fname)).long()
        precise = torch.where(precise == 255, torch.full_like(precise, 21), precise)
        superpixel = self.store.idmap(spx_fname).long()
        target = self.multi_hot_row(lbl_fname, precise.device)
        n_cls = target.sum(dim=1)
        keep = self.selection_lut(spx_fname, precise.device).clone()
        keep[:-1] &= n_cls != 0                                     # (:60-65)
        if self.remove_dominant:
            keep[:-1] &= n_cls != 1
        sp_mask = keep[superpixel.clamp(min=0, max=self.args.nseg)] & (superpixel >= 0)
        return {'image_list': images, 'labels': precise, 'target': target, 'spx': superpixel, 'spmask': sp_mask,
                'imsizes': (int(picture.shape[1]), int(picture.shape[0])), 'fnames': self.im_idx[index]}
