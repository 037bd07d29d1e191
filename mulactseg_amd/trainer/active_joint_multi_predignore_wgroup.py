"""Teacher-weighted group loss during stage-1 training -- reference
``trainer/active_joint_multi_predignore_wgroup.py:84-160``:

    loss = coeff * merged_positive_CE + weighted_group_loss            (no ramp, :122)

At every step an eval-mode "teacher" forward of the same weights (under ``no_grad``) gives, per superpixel and candidate class, its
maximum probability over the selected pixels; that value weights the class's ``-log max p`` of the group term
(``utils.loss.WeightedGroupMultiLabelCE``, ``csrc/teacher_terms.h``).  ``--group_only_single`` keeps only superpixels with more than
one target bit in the term.  Meters as the reference's: ``train-loss``, ``pos-loss``, ``group-loss``.

By default (``args.lowres_loss``) the step runs at quarter resolution: ``forward_train(images, lowres=True)``, the teacher's
``net(images, lowres=True)`` and ``FusedWGroupLoss.forward_lowres`` -- both terms from one forward scan and one backward scan, the
student's and the teacher's logits interpolated in registers, no ``[N,C,H,W]`` tensor of either.  With ``args.lowres_loss = False``
the step is the reference's: full-resolution logits and the two drop-in modules.

One deliberate difference, the same as ``active_joint_multi_predignore_top1plbl``: the reference calls ``net.train()`` after the
teacher forward (:117), which un-freezes BatchNorm under ``--freeze_bn`` from the second iteration on.  Here every module goes back
to the mode it had before the teacher forward, so a frozen BatchNorm stays frozen.
"""
from ..utils.loss import FusedWGroupLoss, MultiChoiceCE_, WeightedGroupMultiLabelCE
from . import active_joint_multi_predignore


class ActiveTrainer(active_joint_multi_predignore.ActiveTrainer):
    def get_criterion(self):
        a = self.args
        self.group_multi_loss = WeightedGroupMultiLabelCE(args=a, num_class=self.num_classes, num_superpixel=a.nseg,
                                                          temperature=a.group_ce_temp)
        self.multi_pos_loss = MultiChoiceCE_(num_class=self.num_classes, temperature=a.multi_ce_temp)
        self.fused_loss = FusedWGroupLoss(a.nseg, a.group_ce_temp, a.multi_ce_temp, group_only_single=getattr(a, 'group_only_single', False))

    def step_losses(self, images, labels, superpixels, spmasks):
        """(pos, group) of one batch."""
        lowres = getattr(self.args, 'lowres_loss', True) and images.is_cuda
        preds = self.forward_train(images, lowres=True) if lowres else self.forward_train(images)
        teacher = self.teacher_forward(images, lowres)
        if lowres:
            return self.fused_loss.forward_lowres(preds, teacher, images.shape[-2:], labels, superpixels, spmasks)
        group = self.group_multi_loss(preds, teacher, labels, superpixels, spmasks)
        pos = self.multi_pos_loss(preds, labels, superpixels, spmasks)
        return pos, group
