"""Stage-2 pseudo labels by prototype assignment WITHOUT expansion (the second row of the paper's Table 2, "disambiguation" only) --
reference ``trainer/eval_save_cosplbl.py:16-196`` (``--method eval_save_cosplbl --loader eval_region_cityscapes_all --train_transform
eval_spx --or_labeling``): every selected pixel, one-hot superpixels included, gets the class of the most similar prototype of its own
superpixel; everything else stays 255.  Saved as uint8 PNGs under ``plbl_gen_<plbl_type>/round_RR`` (``plbl_gen`` without a type).

The reference's launch script for that row runs ``eval_save_cosplbl_prop --plbl_type wo_expand``, where ``plbl_type`` only names the
directory: that command still expands.  This is the generator that stops after the assignment: ``ops.stage2_pseudo_labels(expand=False,
include_onehot=True)`` (``mas_stage2_assign`` + ``mas_stage2_assign_labels``, csrc/stage2.hip) on the quarter-resolution features.  With
every selected pixel valid its labels are those of ``eval_save_cosplbl_prop_includeonehot`` under the mask."""
from .. import ops
from . import eval_save_cosplbl_prop


class ActiveTrainer(eval_save_cosplbl_prop.ActiveTrainer):
    include_onehot = True               # (:139-164: every selected pixel is valid)
    threaded_generation = True          # (no state between pictures)

    def pseudo_label_generation(self, labels, feats, inputs, targets, spmasks, superpixels):
        """Same signature as the reference (:99); ``feats`` may be the quarter-resolution map."""
        return ops.stage2_pseudo_labels(feats.contiguous(), inputs.contiguous(), targets.contiguous(), spmasks.contiguous(),
                                        superpixels.contiguous(), include_onehot=True, expand=False)
