"""Online local-prototype pseudo labelling with similarity-weighted pseudo labels -- reference
``trainer/active_onlinesimwplbl_multi_predignore.py:150-157``: ``active_onlineplbl_multi_predignore`` with
``utils.loss.LocalsimWProtoCE`` (every pixel's CE weighted by its inner product with the nearest prototype, negative products included;
``--th_wplbl``: a gate instead of a weight).  ``loss = coeff * pos + lambda * proto``; the step, its meters and the restored training
mode are the parent's."""
from ..utils.loss import LocalsimWProtoCE
from . import active_onlineplbl_multi_predignore


class ActiveTrainer(active_onlineplbl_multi_predignore.ActiveTrainer):
    proto_loss_class = LocalsimWProtoCE
