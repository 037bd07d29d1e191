"""Self-training on the candidate sets during stage-1 training -- reference
``trainer/active_joint_multi_predignore_top1plbl.py:84-166``:

    loss = coeff * merged_positive_CE + group_loss + lambda * top1_loss,   lambda = ramp_up(it / total, lamparam, lamscale, dorampup)

At every step an eval-mode "teacher" forward of the same weights (under ``no_grad``) decides which selected multi-hot pixels are
confident enough (``--plbl_th``, ``--within_filtering``), and the training-mode logits get ``-log max_{c in Y} p_c`` on those pixels
only (``utils.loss.TopOnePlbl``, ``csrc/teacher_terms.h``).  Meters as the reference's: ``train-loss``, ``pos-loss``, ``group-loss``,
``top1-loss``.

By default (``args.lowres_loss``) the step runs at quarter resolution: ``forward_train(images, lowres=True)``, the teacher's
``net(images, lowres=True)`` and ``FusedTeacherTermLoss.forward_lowres`` -- the three terms from one forward scan and one backward
scan, the student's and the teacher's logits interpolated in registers, no ``[N,C,H,W]`` tensor of either.  With
``args.lowres_loss = False`` the step is the reference's: full-resolution logits and the three drop-in modules.

As in the reference the top-1 term is built with ``temperature=1.0`` whatever ``--multi_ce_temp`` says (:92).

One deliberate difference: the reference calls ``net.train()`` after the teacher forward (:119), which un-freezes BatchNorm under
``--freeze_bn`` from the second iteration on.  Here every module goes back to the mode it had before the teacher forward.
"""
from ..utils.loss import FusedTeacherTermLoss, GroupMultiLabelCE_, MultiChoiceCE_, TopOnePlbl
from ..utils.scheduler import ramp_up
from . import active_joint_multi_predignore


class TeacherTermTrainer(active_joint_multi_predignore.ActiveTrainer):
    """What the two trainers with a teacher-gated candidate term share: ``coeff * pos + group + weight * term``."""
    term = None                     # 'top1' | 'ent'
    term_meter = None
    needs_teacher = False

    def term_temperature(self):
        raise NotImplementedError

    def term_weight(self, iteration, total_itrs):
        raise NotImplementedError

    def term_module(self):
        raise NotImplementedError

    def get_criterion(self):
        super().get_criterion()                                     # group_multi_loss, multi_pos_loss (the drop-in surface)
        a = self.args
        self.fused_loss = FusedTeacherTermLoss(a.nseg, self.term, a.group_ce_temp, a.multi_ce_temp, self.term_temperature(),
                                               within_filtering=getattr(a, 'within_filtering', False),
                                               filtering_threshold=getattr(a, 'plbl_th', 0.0))

    def step_losses(self, images, labels, superpixels, spmasks):
        """(pos, group, term) of one batch."""
        lowres = getattr(self.args, 'lowres_loss', True) and images.is_cuda
        preds = self.forward_train(images, lowres=True) if lowres else self.forward_train(images)
        teacher = self.teacher_forward(images, lowres) if self.needs_teacher else None
        if lowres:
            return self.fused_loss.forward_lowres(preds, teacher, images.shape[-2:], labels, superpixels, spmasks)
        group = self.group_multi_loss(preds, labels, superpixels, spmasks)
        pos = self.multi_pos_loss(preds, labels, superpixels, spmasks)
        args = (preds, teacher, labels, superpixels, spmasks) if self.needs_teacher else (preds, labels, superpixels, spmasks)
        return pos, group, self.term_module()(*args)

    def step(self, iteration, total_itrs, *batch):
        pos_loss, group_loss, term_loss = self.step_losses(*batch)
        loss = self.args.coeff * pos_loss + group_loss + self.term_weight(iteration, total_itrs) * term_loss
        return loss, {'pos-loss': pos_loss, 'group-loss': group_loss, self.term_meter: term_loss}


class ActiveTrainer(TeacherTermTrainer):
    term = 'top1'
    term_meter = 'top1-loss'
    needs_teacher = True

    def term_temperature(self):
        return 1.0

    def get_criterion(self):
        super().get_criterion()
        a = self.args
        self.multi_top1_loss = TopOnePlbl(num_class=self.num_classes, within_filtering=a.within_filtering, filtering_threshold=a.plbl_th,
                                          temperature=1.0)

    def term_module(self):
        return self.multi_top1_loss

    def term_weight(self, iteration, total_itrs):
        a = self.args
        return ramp_up(iteration / total_itrs, lamparam=a.lamparam, scale=a.lamscale, dorampup=a.dorampup)
