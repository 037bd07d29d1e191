"""The local-prototype labels inside the queried superpixels, kept only where the model agrees -- reference
``trainer/eval_cosplbl_filt_within_multihot.py:16-173`` (``--method eval_cosplbl_filt_within_multihot``): a label survives where it
equals the arg-max of the model's prediction over all channels, and every prototype pixel then takes its own class back (``:162-169``;
the highest class when it is the prototype of several, the last write of the reference's indexed assignment).  One IoU table (``:63``).
Mode ``'filt'`` of ``ops.within_multihot_eval``."""
from . import eval_cosplbl_within_multihot


class ActiveTrainer(eval_cosplbl_within_multihot.ActiveTrainer):
    mode = 'filt'
    tables = ('IoU',)
