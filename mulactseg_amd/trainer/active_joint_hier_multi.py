"""Hierarchical group loss during stage-1 training -- reference ``trainer/active_joint_hier_multi.py:9-91``:

    loss = coeff * merged_positive_CE + hierarchical_group_loss            (:53)

The network has one output per class (19 on Cityscapes; no "undefined" output, so both terms drop the last target column).  The
group term (``utils.loss.HierGroupMultiLabelCE``, or ``AugHierGroupMultiLabelCE`` with ``--nocropsp``; ``csrc/hier_group.h``) chooses
the arg-pixel of every (superpixel, candidate class) as the plain group term does and then sums ``-log(p_c + eps)`` over every
selected pixel of the FINE superpixel (``batch['spx_small']``, ``--load_smaller_spx`` / ``--small_nseg``) that arg-pixel lies in.  Its
softmax runs at temperature 1.0 whatever ``--group_ce_temp`` says (the reference's constructor discards it); the merged-positive
term keeps ``--multi_ce_temp``.  ``--group_only_single`` keeps only superpixels with more than one target bit among the arg-pixels.
Meters as the reference's: ``train-loss``, ``pos-loss``, ``group-loss``.

``--nocropsp``: the reference clears the target rows of the superpixels on the crop's border in place, inside the group loss, and
calls the merged-positive loss afterwards on the same tensor; both terms therefore miss those rows.  Here the group loss clears a
copy of the bits table on the device and ``merged_positive`` evaluates the second term on that copy; ``labels`` is not modified.

By default (``args.lowres_loss``) the step runs at quarter resolution: ``forward_train(images, lowres=True)`` and the
``forward_lowres`` forms, the logits interpolated in registers, no ``[N,C,H,W]`` tensor.  With ``args.lowres_loss = False`` the step
runs the same kernels on full-resolution logits.

Skipping: the reference's ``check_loss_sanity`` (:21-27) skips the step on a zero loss AND on a NaN loss, silently.  This trainer
uses ``active_joint_multi.ActiveTrainer.update`` like its siblings: a zero loss skips the optimizer step, a NaN loss RAISES -- the
project's policy for every stage-1 trainer, kept as it is.
"""
from ..utils.loss import AugHierGroupMultiLabelCE, HierGroupMultiLabelCE, MultiChoiceCE
from . import active_joint_multi


class ActiveTrainer(active_joint_multi.ActiveTrainer):
    batch_keys = ('images', 'labels', 'spx', 'spx_small', 'spmask')

    def get_criterion(self):
        a = self.args
        cls = AugHierGroupMultiLabelCE if getattr(a, 'nocropsp', False) else HierGroupMultiLabelCE
        self.hier_group_multi_loss = cls(args=a, num_class=self.num_classes, num_superpixel=a.nseg,
                                         only_single=getattr(a, 'group_only_single', False), gumbel_scale=getattr(a, 'gumbel_scale', -1),
                                         temperature=a.group_ce_temp)
        self.multi_pos_loss = MultiChoiceCE(num_class=self.num_classes, temperature=a.multi_ce_temp)

    def step_losses(self, images, labels, superpixels, superpixel_smalls, spmasks):
        """(pos, group) of one batch."""
        lowres = getattr(self.args, 'lowres_loss', True) and images.is_cuda
        preds = self.forward_train(images, lowres=True) if lowres else self.forward_train(images)
        size = images.shape[-2:] if lowres else None
        hier = self.hier_group_multi_loss
        if lowres:
            group = hier.forward_lowres(preds, size, labels, spmasks, superpixels, superpixel_smalls)
        else:
            group = hier(preds, labels, spmasks, superpixels, superpixel_smalls)
        # the bits the group term saw (rows cleared under --nocropsp): the reference's second term reads the tensor the first one modified
        pos = hier.merged_positive(preds, size, superpixels, spmasks, self.multi_pos_loss.temp)
        return pos, group
