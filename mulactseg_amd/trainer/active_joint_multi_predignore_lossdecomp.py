"""The production stage-1 trainer (Cityscapes) -- reference
``trainer/active_joint_multi_predignore_lossdecomp.py:74-116``:

    loss = coeff * ce(one-hot regions) + coeff_mc * mc(multi-hot regions) + coeff_gm * group(multi-hot regions)

The three losses come from ONE forward scan and ONE backward scan of the logits
(``utils.loss.FusedPartialLabelLoss`` over ``csrc/losses.hip``) instead of two modules that each
re-compute the softmax; by default (``args.lowres_loss``, True) the scans take the model's quarter-resolution logits and
evaluate the final x4 bilinear upsampling (``models/segmentation/utils.py:25``) per selected pixel.  Under data parallelism the normalisers ``1 + n`` are global over the batch
(SURVEY.md section 5.8): the fixed-point sums and counts are all-reduced before the division so that
N GPUs x batch 4 optimise exactly the single-GPU objective of batch 4N.

``--partial_loss rc|topone`` swaps the term of the multi-hot pixels (``mc``) for the risk-consistent weighting or the top-1 candidate
(``csrc/partial_label.h``); ``ce`` and ``group`` stay, and so do the scans.
"""

from ..utils.loss import (FusedPartialLabelLoss, GroupMultiLabelCE_onlymulti, OnehotCEMultihotChoice, OnehotCEMultihotRC,
                          OnehotCEMultihotTopone)
from . import active_joint_multi_predignore


class ActiveTrainer(active_joint_multi_predignore.ActiveTrainer):
    group_term = True               # False: no group term in the objective or among the meters (lossdecomp_rc, lossdecomp_topone)

    def get_criterion(self):
        a = self.args
        # the reference's two modules stay available under their names (drop-in surface) ...
        self.group_multi_loss = GroupMultiLabelCE_onlymulti(args=a, num_class=self.num_classes, num_superpixel=a.nseg, temperature=a.group_ce_temp)
        multi_hot = getattr(a, 'partial_loss', 'choice')
        decomp = {'choice': OnehotCEMultihotChoice, 'rc': OnehotCEMultihotRC, 'topone': OnehotCEMultihotTopone}[multi_hot]
        self.multi_pos_loss = decomp(num_class=self.num_classes, temperature=a.multi_ce_temp)
        # ... and step uses the fused scan when both temperatures agree (they do in every script)
        self.fused_loss = None
        if a.group_ce_temp == a.multi_ce_temp:
            self.fused_loss = FusedPartialLabelLoss(a.nseg, a.group_ce_temp, a.multi_ce_temp, only_multi=True, decomp=True, multi_hot=multi_hot)

    def losses(self, preds, labels, superpixels, spmasks):
        if self.fused_loss is not None:
            return self.fused_loss(preds, labels, superpixels, spmasks)
        group = self.group_multi_loss(preds, labels, superpixels, spmasks)
        ce, mc = self.multi_pos_loss(preds, labels, superpixels, spmasks)
        return group, ce, mc

    def step(self, iteration, total_itrs, images, labels, superpixels, spmasks):
        a = self.args
        coeff_gm = a.coeff_gm if self.group_term else 0.0
        if self.fused_loss is not None and getattr(a, 'lowres_loss', True) and images.is_cuda:
            # quarter-resolution logits in, upsampling inside the loss scans (no [N,C,H,W] logit / gradient tensors)
            preds_q = self.forward_train(images, lowres=True)
            loss, group_loss, ce_loss, mc_loss = self.fused_loss.weighted_lowres(preds_q, images.shape[-2:], labels, superpixels, spmasks,
                                                                                 a.coeff, a.coeff_mc, coeff_gm)
        else:
            group_loss, ce_loss, mc_loss = self.losses(self.forward_train(images), labels, superpixels, spmasks)
            loss = (a.coeff * ce_loss) + (a.coeff_mc * mc_loss)
            if self.group_term:
                loss = loss + (coeff_gm * group_loss)
        meters = {'ce-loss': ce_loss, 'pos-loss': mc_loss}
        if self.group_term:
            meters['group-loss'] = group_loss
        return loss, meters
