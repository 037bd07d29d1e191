"""Risk-consistent partial-label baseline -- reference ``trainer/active_joint_multi_lossdecomp_rc.py``:

    loss = coeff * ce(one-hot regions) + coeff_mc * mc(multi-hot regions)          (no group term)

with ``mc`` the risk-consistent weighting of ``utils/loss.py:653-707`` over the multi-hot pixels (the reference's own\n``OnehotCEMultihotRC`` raises at ``:54``; see ``utils/loss.py`` here).  Meters as the reference's: ``train-loss``, ``ce-loss``, ``pos-loss``.  Both losses come
from one forward and one backward scan of ``utils.loss.FusedPartialLabelLoss(group=False, multi_hot='rc')``; by default
(``args.lowres_loss``) the scans take the model's quarter-resolution logits, so no full-resolution logit tensor exists.
"""
from ..utils.loss import FusedPartialLabelLoss, OnehotCEMultihotRC
from . import active_joint_multi_lossdecomp


class ActiveTrainer(active_joint_multi_lossdecomp.ActiveTrainer):
    multi_hot = 'rc'

    def get_criterion(self):
        a = self.args
        self.multi_pos_loss = OnehotCEMultihotRC(num_class=self.num_classes, temperature=a.multi_ce_temp)       # (drop-in surface)
        self.fused_loss = FusedPartialLabelLoss(a.nseg, a.multi_ce_temp, a.multi_ce_temp, decomp=True, multi_hot=self.multi_hot, group=False)

    def train_impl(self, total_itrs, val_period):
        a = self.args
        self.net.train()
        for iteration in range(total_itrs):
            images, labels, superpixels, spmasks = self._batch()
            self.optimizer.zero_grad()
            if getattr(a, 'lowres_loss', True) and images.is_cuda:
                preds_q = self.forward_train(images, lowres=True)
                loss, _, ce_loss, mc_loss = self.fused_loss.weighted_lowres(preds_q, images.shape[-2:], labels, superpixels, spmasks,
                                                                            a.coeff, a.coeff_mc, 0.0)
            else:
                _, ce_loss, mc_loss = self.fused_loss(self.forward_train(images), labels, superpixels, spmasks)
                loss = (a.coeff * ce_loss) + (a.coeff_mc * mc_loss)
            self.update(loss)
            self.update_average_meter({'train-loss': loss, 'ce-loss': ce_loss, 'pos-loss': mc_loss})
            self.log_training(iteration, None, total_itrs)
            self.log_validation(iteration, val_period)
        self.flush_meters()
        self.check_stream_k()
