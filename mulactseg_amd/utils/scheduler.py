"""Polynomial learning-rate decay -- reference ``utils/scheduler.py:4-13``:
``lr = max(base_lr * (1 - it/max_iters) ** power, min_lr)`` -- and the loss-weight ramp of the online pseudo-label trainers
(``utils/scheduler.py:15-28``)."""
import math

from torch.optim.lr_scheduler import _LRScheduler


class PolyLR(_LRScheduler):
    def __init__(self, optimizer, max_iters, power=0.9, last_epoch=-1, min_lr=1e-6):
        self.power = power
        self.max_iters = max_iters
        self.min_lr = min_lr
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        decay = (1 - self.last_epoch / self.max_iters) ** self.power
        return [max(base_lr * decay, self.min_lr) for base_lr in self.base_lrs]


def ramp_up(x, lamparam=0.1, scale=1.0, dorampup=True):
    """Weight of the pseudo-label loss at the fraction ``x`` of the training run -- reference ``utils/scheduler.py:15-23``: without
    ``dorampup`` (or past the end) it is 1.0 -- NOT ``scale`` --, else ``sigmoid_ramp_up``."""
    if not dorampup or x > 1.0:
        return 1.0
    return sigmoid_ramp_up(x, lamparam, scale)


def sigmoid_ramp_up(x, lamparam, scale):
    """``scale * (2 / (1 + exp(-x / lamparam)) - 1)``: 0 at x = 0, towards ``scale`` with damping ``lamparam`` (:25-28)."""
    den = 1.0 + math.exp(-x / lamparam)
    return (2.0 / den - 1.0) * scale
