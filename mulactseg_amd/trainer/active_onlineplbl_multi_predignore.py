"""Online local-prototype pseudo labelling during stage-1 training -- reference
``trainer/active_onlineplbl_multi_predignore.py:143-194``:

    loss = coeff * merged_positive_CE + lambda * local_proto_CE,   lambda = ramp_up(it / total, lamparam, lamscale, dorampup)

At every step the network labels its own selected multi-hot superpixels (a second, eval-mode forward under ``no_grad``) and the
training-mode logits learn from those labels (``utils.loss.LocalProtoCE``).  Meters as the reference's: ``train-loss``, ``pos-loss``,
``local-proto-loss``.

By default (``args.lowres_loss``) the step runs at quarter resolution: ``forward_train(images, lowres=True)``,
``net.feat_forward_quarter(images)`` and the losses' ``forward_lowres``, so neither ``feat_forward``'s ``[N,256,H,W]`` features nor
any ``[N,C,H,W]`` logit tensor exists, and nothing between forward and backward waits for the host.

One deliberate difference: the reference calls ``net.eval()`` inside the loop and never ``net.train()`` again, so from its second
iteration on it trains with frozen BatchNorm statistics.  Here the pseudo-label forward runs in eval mode and every module's previous
mode is restored after it (``active_joint_multi.ActiveTrainer.pseudo_label_forward``): every step trains with batch statistics, unless
``args.freeze_bn`` froze them.  The loss classes themselves are exact.
"""
from ..utils.loss import FusedPartialLabelLoss, LocalProtoCE, MultiChoiceCE_
from ..utils.scheduler import ramp_up
from . import active_joint_multi_predignore


class ActiveTrainer(active_joint_multi_predignore.ActiveTrainer):
    proto_loss_class = LocalProtoCE
    proto_meter = 'local-proto-loss'
    uses_pos_loss = True            # False: the pseudo-label loss is the whole objective (active_onlinewplblonly_multi_predignore)

    def get_criterion(self):
        a = self.args
        self.multi_local_proto_loss = self.proto_loss_class(args=a, num_superpixel=a.nseg, temperature=a.group_ce_temp)
        self.multi_pos_loss = MultiChoiceCE_(num_class=self.num_classes, temperature=a.multi_ce_temp)       # (drop-in surface)
        # the same merged-positive CE from the quarter-resolution logits: the CE-only form of the fused scans
        self.pos_lowres = FusedPartialLabelLoss(a.nseg, a.multi_ce_temp, a.multi_ce_temp, decomp=False, group=False)

    def proto_weight(self, iteration, total_itrs):
        a = self.args
        return ramp_up(iteration / total_itrs, lamparam=a.lamparam, scale=a.lamscale, dorampup=a.dorampup)

    def step_losses(self, images, labels, superpixels, spmasks):
        """(pos_loss or None, proto_loss) of one batch."""
        a = self.args
        if getattr(a, 'lowres_loss', True) and images.is_cuda:
            size = images.shape[-2:]
            preds_q = self.forward_train(images, lowres=True)
            feats_plbl, preds_plbl = self.pseudo_label_forward(images, True)
            pos = self.pos_lowres.forward_lowres(preds_q, size, labels, superpixels, spmasks)[1] if self.uses_pos_loss else None
            return pos, self.multi_local_proto_loss.forward_lowres(preds_plbl, feats_plbl, preds_q, size, labels, superpixels, spmasks)
        preds = self.forward_train(images)
        feats_plbl, preds_plbl = self.pseudo_label_forward(images, False)
        pos = self.multi_pos_loss(preds, labels, superpixels, spmasks) if self.uses_pos_loss else None
        return pos, self.multi_local_proto_loss(preds_plbl, feats_plbl, preds, labels, superpixels, spmasks)

    def step(self, iteration, total_itrs, *batch):
        pos_loss, proto_loss = self.step_losses(*batch)
        if not self.uses_pos_loss:
            return proto_loss, {}
        loss = self.args.coeff * pos_loss + self.proto_weight(iteration, total_itrs) * proto_loss
        return loss, {'pos-loss': pos_loss, self.proto_meter: proto_loss}
