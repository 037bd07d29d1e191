"""Cross-view hierarchical group loss during stage-1 training -- reference ``trainer/active_joint_hier_multi_async.py:9-96``:

    loss = coeff * merged_positive_CE + cross_view_hierarchical_group_loss            (:58)

Every labelled sample carries two views of one picture (the loader ``region_cityscapes_or_tensor_ignore_async``): the augmented crop
the student trains on, and a WEAK view -- the whole picture, resized only (``batch['image_weak']``, ``'spx_weak'``,
``'spx_small_weak'``, ``'spmask_weak'``).  At every step an eval-mode "teacher" forward of the same weights (under ``no_grad``) looks
at the weak view and decides, per (superpixel, candidate class), the fine superpixel around its arg-pixel; the student pays for those
(fine superpixel, class) pairs on its crop (``utils.loss.AsyncHierGroupMultiLabelCE``; ``csrc/hier_group.h``).  The group softmaxes
run at temperature 1.0 whatever ``--group_ce_temp`` says; the merged-positive term keeps ``--multi_ce_temp``.  Meters as the
reference's: ``train-loss``, ``pos-loss``, ``group-loss``.

Deliberate differences from the reference:

* as written the reference's ``get_criterion`` raises ``TypeError`` (it does not pass ``args`` to the loss constructor, ``:15``);
  here ``args`` is passed;
* after the teacher forward the reference calls ``net.train()``, which puts a BatchNorm frozen by ``--freeze_bn`` back into training
  mode until the next validation; here every module goes back to the mode it had (``eval_mode``, as ``top1plbl`` / ``wgroup``);
* the reference's ``check_loss_sanity`` skips the step on a zero loss AND on a NaN loss, silently; ``update`` here skips on zero and
  RAISES on NaN -- the project's policy for every stage-1 trainer.

By default (``args.lowres_loss``) both forwards run at quarter resolution and the ``forward_lowres`` forms interpolate the logits in
registers: no full-resolution tensor of either view exists.  With ``args.lowres_loss = False`` the same kernels run on full-resolution
logits.
"""
from ..utils.loss import AsyncHierGroupMultiLabelCE, MultiChoiceCE
from . import active_joint_hier_multi


class ActiveTrainer(active_joint_hier_multi.ActiveTrainer):
    batch_keys = ('images', 'image_weak', 'labels', 'spx', 'spx_weak', 'spx_small', 'spx_small_weak', 'spmask', 'spmask_weak')

    def group_criterion(self):
        a = self.args
        return AsyncHierGroupMultiLabelCE(args=a, num_class=self.num_classes, num_superpixel=a.nseg,
                                          only_single=getattr(a, 'group_only_single', False), gumbel_scale=getattr(a, 'gumbel_scale', -1),
                                          temperature=a.group_ce_temp)

    def get_criterion(self):
        self.hier_group_multi_loss = self.group_criterion()
        self.multi_pos_loss = MultiChoiceCE(num_class=self.num_classes, temperature=self.args.multi_ce_temp)

    def step_losses(self, images, images_weak, labels, superpixels, superpixels_weak, superpixel_smalls, spx_smalls_weak, spmasks, spmasks_weak):
        """(pos, group) of one batch."""
        lowres = getattr(self.args, 'lowres_loss', True) and images.is_cuda
        preds_weak = self.teacher_forward(images_weak, lowres)
        preds = self.forward_train(images, lowres=True) if lowres else self.forward_train(images)
        size = images.shape[-2:] if lowres else None
        hier = self.hier_group_multi_loss
        if lowres:
            group = hier.forward_lowres(preds, size, preds_weak, images_weak.shape[-2:], labels, spmasks, spmasks_weak, superpixels,
                                        superpixels_weak, superpixel_smalls, spx_smalls_weak)
        else:
            group = hier(preds, preds_weak, labels, spmasks, spmasks_weak, superpixels, superpixels_weak, superpixel_smalls, spx_smalls_weak)
        pos = hier.merged_positive(preds, size, superpixels, spmasks, self.multi_pos_loss.temp)
        return pos, group
