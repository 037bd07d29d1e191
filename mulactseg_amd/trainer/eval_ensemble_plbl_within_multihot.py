"""Reference ``trainer/eval_ensemble_plbl_within_multihot.py:16-173`` (``--method eval_ensemble_plbl_within_multihot``): as executed it
generates the labels of ``eval_cosplbl_within_multihot`` and prints the single IoU table (``:63``)."""
from . import eval_cosplbl_within_multihot


class ActiveTrainer(eval_cosplbl_within_multihot.ActiveTrainer):
    tables = ('IoU',)
