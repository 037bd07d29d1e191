"""Prototype-similarity weighted cross entropy as the ONLY loss -- reference ``trainer/active_pwce_multi_predignore.py:157-211``:
``loss = JointLocalProtoWeightingCE(...)``, one meter (``train-loss``).  At every step the network's eval-mode forward (under
``no_grad``) gives the local prototypes and the features; every selected pixel of a multi-hot superpixel learns from the softmax of its
prototype similarities at temperature ``--simw_temp``.  With ``--simw_temp_schedule`` the temperature is 1000 (targets uniform over
the candidates) for the first 20 000 iterations; the reference writes that into ``args.simw_temp`` each step, here ``simw_temp_at``
returns it and the loss takes it per call, so ``args`` keeps what the user gave.

By default (``args.lowres_loss``) the step runs at quarter resolution, and the module's mode is restored after the eval-mode forward:
both as in ``active_onlineplbl_multi_predignore``, whose documented difference from the reference (which never calls ``net.train()``
again) this trainer shares."""
from ..utils.loss import JointLocalProtoWeightingCE
from . import active_joint_multi_predignore

SIMW_SCHEDULE_ITERATIONS = 20000
SIMW_SCHEDULE_TEMP = 1000.0


class ActiveTrainer(active_joint_multi_predignore.ActiveTrainer):
    def __init__(self, args, logger, selection_iter):
        super().__init__(args, logger, selection_iter)
        self.simw_temp_orig = args.simw_temp

    def get_criterion(self):
        a = self.args
        self.joint_local_proto_weight_loss = JointLocalProtoWeightingCE(args=a, num_superpixel=a.nseg, temperature=a.group_ce_temp)

    def simw_temp_at(self, iteration):
        if getattr(self.args, 'simw_temp_schedule', False) and iteration < SIMW_SCHEDULE_ITERATIONS:
            return SIMW_SCHEDULE_TEMP
        return getattr(self, 'simw_temp_orig', self.args.simw_temp)

    def step_loss(self, images, labels, superpixels, spmasks, simw_temp):
        crit = self.joint_local_proto_weight_loss
        if getattr(self.args, 'lowres_loss', True) and images.is_cuda:
            size = images.shape[-2:]
            preds_q = self.forward_train(images, lowres=True)
            feats_plbl, preds_plbl = self.pseudo_label_forward(images, True)
            return crit.forward_lowres(preds_plbl, feats_plbl, preds_q, size, labels, superpixels, spmasks, simw_temp=simw_temp)
        preds = self.forward_train(images)
        feats_plbl, preds_plbl = self.pseudo_label_forward(images, False)
        return crit(preds_plbl, feats_plbl, preds, labels, superpixels, spmasks, simw_temp=simw_temp)

    def step(self, iteration, total_itrs, *batch):
        return self.step_loss(*batch, self.simw_temp_at(iteration)), {}
