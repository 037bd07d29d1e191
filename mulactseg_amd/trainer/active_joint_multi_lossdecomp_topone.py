"""Naive top-1 partial-label baseline -- reference ``trainer/active_joint_multi_lossdecomp_topone.py``:

    loss = coeff * ce(one-hot regions) + coeff_mc * mc(multi-hot regions)          (no group term)

with ``mc`` ``-log max_{c in Y} p_c`` over the multi-hot pixels.  Meters as the reference's: ``train-loss``, ``ce-loss``, ``pos-loss``.  Both losses come
from one forward and one backward scan of ``utils.loss.FusedPartialLabelLoss(group=False, multi_hot='topone')``; by default
(``args.lowres_loss``) the scans take the model's quarter-resolution logits, so no full-resolution logit tensor exists.
"""
from ..utils.loss import FusedPartialLabelLoss, OnehotCEMultihotTopone
from . import active_joint_multi_lossdecomp


class ActiveTrainer(active_joint_multi_lossdecomp.ActiveTrainer):
    multi_hot = 'topone'
    group_term = False          # (the step is active_joint_multi_predignore_lossdecomp's, without its group term)

    def get_criterion(self):
        a = self.args
        self.multi_pos_loss = OnehotCEMultihotTopone(num_class=self.num_classes, temperature=a.multi_ce_temp)       # (drop-in surface)
        self.fused_loss = FusedPartialLabelLoss(a.nseg, a.multi_ce_temp, a.multi_ce_temp, decomp=True, multi_hot=self.multi_hot, group=False)
