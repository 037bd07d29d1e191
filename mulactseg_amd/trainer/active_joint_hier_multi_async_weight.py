"""Teacher-weighted cross-view hierarchical group loss -- reference ``trainer/active_joint_hier_multi_async_weight.py:9-21``:
``active_joint_hier_multi_async`` with ``utils.loss.WeightAsyncHierGroupMultiLabelCE``: every (fine superpixel, class) pair is weighted
by the ``--weight_reduce`` (``max``, the default, or ``mean``) of the teacher's probability of that class over the selected weak-view
pixels of the fine superpixel.  As written the reference raises ``TypeError`` here too (no ``args`` for the constructor); see the
sibling module for the other deliberate differences."""
from ..utils.loss import WeightAsyncHierGroupMultiLabelCE
from . import active_joint_hier_multi_async


class ActiveTrainer(active_joint_hier_multi_async.ActiveTrainer):
    def group_criterion(self):
        a = self.args
        return WeightAsyncHierGroupMultiLabelCE(args=a, num_class=self.num_classes, num_superpixel=a.nseg,
                                                only_single=getattr(a, 'group_only_single', False),
                                                gumbel_scale=getattr(a, 'gumbel_scale', -1), temperature=a.group_ce_temp,
                                                weight_reduce=getattr(a, 'weight_reduce', 'max'))
