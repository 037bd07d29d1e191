"""Online local-prototype pseudo labelling with confidence-weighted pseudo labels -- reference
``trainer/active_onlinewplbl_multi_predignore.py:150-157``: ``active_onlineplbl_multi_predignore`` with ``utils.loss.LocalWProtoCE``
(every pixel's CE weighted by the network's probability of its pseudo label; ``--weight_wo_proto``: prototype pixels weigh 1;
``--th_wplbl``: a gate instead of a weight).  The step, its meters and the restored training mode are the parent's."""
from ..utils.loss import LocalWProtoCE
from . import active_onlineplbl_multi_predignore


class ActiveTrainer(active_onlineplbl_multi_predignore.ActiveTrainer):
    proto_loss_class = LocalWProtoCE
