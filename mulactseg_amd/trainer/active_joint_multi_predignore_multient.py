"""Sharpening the candidate sets during stage-1 training -- reference
``trainer/active_joint_multi_predignore_multient.py:72-146``:

    loss = coeff * merged_positive_CE + group_loss + entcoeff * ent_loss

``ent_loss`` (``utils.loss.MultiChoiceEnt_``, ``csrc/teacher_terms.h``) is the entropy of the softmax restricted to the candidate set
of every selected multi-hot pixel, at ``--multi_ce_temp``.  Meters as the reference's: ``train-loss``, ``pos-loss``, ``group-loss``,
``ent-loss``.  No teacher forward.  By default (``args.lowres_loss``) the three terms come from one forward scan and one backward
scan over the quarter-resolution logits (``FusedTeacherTermLoss.forward_lowres``); ``args.lowres_loss = False`` is the reference's
step on full-resolution logits with the three drop-in modules.
"""
from ..utils.loss import MultiChoiceEnt_
from .active_joint_multi_predignore_top1plbl import TeacherTermTrainer


class ActiveTrainer(TeacherTermTrainer):
    term = 'ent'
    term_meter = 'ent-loss'

    def term_temperature(self):
        return self.args.multi_ce_temp

    def get_criterion(self):
        super().get_criterion()
        self.multi_ent_loss = MultiChoiceEnt_(num_class=self.num_classes, temperature=self.args.multi_ce_temp)

    def term_module(self):
        return self.multi_ent_loss

    def term_weight(self, iteration, total_itrs):
        return self.args.entcoeff
