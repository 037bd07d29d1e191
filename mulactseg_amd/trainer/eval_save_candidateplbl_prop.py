"""Top-1 within the candidate set inside the selected superpixels, a confidence-thresholded top-1 everywhere else -- reference
``trainer/eval_save_candidateplbl_prop.py:13-88`` (``--method eval_save_candidateplbl_prop --plbl_th P --ce_temp T --loader
eval_region_cityscapes_all --train_transform eval_spx --or_labeling``): ``eval_save_candidateplbl``'s labels under the mask; outside it
the arg-max of the logits where ``softmax(logits / ce_temp).max > plbl_th`` (for every ``plbl_th``, 0 included), 255 elsewhere.  Saved
under ``plbl_gen_<plbl_type>/round_RR``; without ``--plbl_type`` the reference sets ``wcand`` (:26-27), and so does this.

One kernel per picture (``ops.candidate_pseudo_labels(fallback=True)``, csrc/candidate_plbl.hip), counters included."""
from . import eval_save_candidateplbl


class ActiveTrainer(eval_save_candidateplbl.ActiveTrainer):
    fallback = True

    def _save_dir(self):
        if getattr(self.args, 'plbl_type', None) is None:
            self.args.plbl_type = 'wcand'
        return super()._save_dir()
