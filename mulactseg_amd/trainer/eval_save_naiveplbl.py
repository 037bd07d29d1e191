"""Naive top-1 stage-2 pseudo labels, the ablation without prototypes (paper Fig. 7 (a)) -- reference
``trainer/eval_save_naiveplbl.py:13-97`` (``--method eval_save_naiveplbl --plbl_type naive --loader eval_region_cityscapes_all
--train_transform eval_spx``): per picture the arg-max of the network's logits over all C channels on the selected superpixels
(one-hot ones included), or, with ``--plbl_th > 0``, on every pixel whose softmax maximum exceeds it; 255 elsewhere.  Saved as uint8
PNGs under ``plbl_gen_<plbl_type>/round_RR`` (``plbl_gen`` without a type).

On the GPU the network stops at quarter resolution and one kernel (``ops.naive_pseudo_labels``, csrc/naive_plbl.hip) upsamples,
takes the arg-max and applies the mask or the threshold: the full-resolution logits never exist.  ``MAS_NAIVE_PLBL=aten`` takes the
reference's ATen lines instead.  The pictures go through the threaded loop of ``eval_save_cosplbl_prop.inference``."""
from .. import ops
from . import eval_save_cosplbl_prop


class ActiveTrainer(eval_save_cosplbl_prop.ActiveTrainer):
    threaded_generation = True          # (no state between pictures)

    def pseudo_labels(self, images, labels, targets, spmasks, superpixels):
        if getattr(self.net, 'lowres_logits', False):
            z = self.net(images, lowres=True)
        else:
            z = self.net(images)
        return ops.naive_pseudo_labels(z.contiguous(), images.shape[-2:], spmasks, getattr(self.args, 'plbl_th', 0.0))
