"""The local-prototype labels inside the queried superpixels beside the classifier's own similarity -- reference
``trainer/eval_maxcosplbl_within_multihot.py:18-176`` (``--method eval_maxcosplbl_within_multihot``): the labels and the IoU table of
``eval_cosplbl_within_multihot``; additionally it prints how many valid pixels have a winning local similarity below
``max_c (logit_c * Y_c)`` (``:168-169``, there per picture; here per batch, from ``diag[2]`` of ``ops.within_multihot_eval``, read once
after the loop)."""
from . import eval_cosplbl_within_multihot


class ActiveTrainer(eval_cosplbl_within_multihot.ActiveTrainer):
    tables = ('IoU',)
    counts_below = True
