"""Multi-scale + flip naive arg-max pseudo labels for PASCAL VOC -- reference ``trainer/eval_save_cosplbl_naive_voc_ms.py:30-147``
(``--method eval_save_cosplbl_naive_voc_ms --train_transform eval_spx_identity_ms --loader eval_region_voc_all_ms``): every picture of
``batch['image_list'][0]`` (five scales, then the same five flipped) goes through ``feat_forward``; the logits are flipped back for
the second half, resized to the original size (bilinear, ``align_corners=False``), averaged over the ten, and the arg-max is taken as
in the single-scale generator.  The averaged features are never used, so they are not computed.  PNGs go to ``plbl_gen_<plbl_type>``
or ``plbl_gen_ms`` (:40-43).

On the GPU the ten forwards stop at quarter resolution and one kernel (``ops.ms_naive_labels``, csrc/ms_naive.hip) does the
upsampling, the flip, the resize, the mean, the arg-max and the IoU counters; ``MAS_MS_NAIVE=aten`` takes the ATen chain."""
import torch

from . import eval_save_cosplbl_naive_voc, eval_save_cosplbl_prop_includeonehot_voc_ms


class ActiveTrainer(eval_save_cosplbl_naive_voc.ActiveTrainer):
    _save_dir = eval_save_cosplbl_prop_includeonehot_voc_ms.ActiveTrainer._save_dir      # plbl_gen_ms without a type

    def sources(self, batch):
        """-> (quarter-resolution logits of the ten pictures, their sizes, flips: the second half)."""
        image_list = batch['image_list'][0]
        n = len(image_list)
        logits_q = [self.net(img.to(self.device, dtype=torch.float32)[None], lowres=True).contiguous() for img in image_list]
        return logits_q, [tuple(img.shape[-2:]) for img in image_list], [(n - 1) // 2 < idx for idx in range(n)]

    def pseudo_labels(self, images, labels, targets, spmasks, superpixels):
        raise NotImplementedError("the multi-scale generator consumes batch['image_list']: use inference()")
