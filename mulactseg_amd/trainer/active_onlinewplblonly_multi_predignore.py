"""The confidence-weighted local-prototype loss as the ONLY loss -- reference
``trainer/active_onlinewplblonly_multi_predignore.py:139-184``: ``loss = JointLocalProtoCE(...)``, one meter (``train-loss``), no
merged-positive term and no ramp.  A batch without a non-zero term gives NaN, which ``update`` raises on, as the reference's
``check_loss_sanity`` does.  The step and the restored training mode are ``active_onlineplbl_multi_predignore``'s."""
from ..utils.loss import JointLocalProtoCE
from . import active_onlineplbl_multi_predignore


class ActiveTrainer(active_onlineplbl_multi_predignore.ActiveTrainer):
    uses_pos_loss = False

    def get_criterion(self):
        a = self.args
        self.joint_local_proto_loss = JointLocalProtoCE(args=a, num_superpixel=a.nseg, temperature=a.group_ce_temp)
        self.multi_local_proto_loss = self.joint_local_proto_loss           # (the name the shared step reads)
