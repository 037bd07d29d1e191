"""IoU meters with the reference's interface (``utils/miou.py``, ``utils/miou_evalignore.py``), counting
on the device (``csrc/metrics.hip``) instead of 19 x 3 host-synchronising reductions per batch.

``MeanIoU(num_classes, ignore_label)``: ``_before_epoch()``, ``_after_step({'outputs', 'targets'})``,
``_after_epoch()`` -> per-class IoU x 100 where an unseen class counts as 100 (``utils/miou.py:63-70``).
``IoUIgnore``: IoU of the extra "undefined" class (label ``num_classes`` in the prediction,
``ignore_label`` in the ground truth).
``LogitsIoU`` (new): both meters from one read of the logits (fused arg-max).
``LowresLogitsIoU`` (new): the same counters from the quarter-resolution logits (``net(x, lowres=True)``), upsampled per pixel in
registers: the full-resolution logits never exist.
``MultiScaleLogitsIoU`` (new): the same counters of the mean logits of scaled and flipped copies of a picture, from their
quarter-resolution logits in one launch.
``WithinMultihotIoU`` (new): the counters of the local-prototype labels inside the queried superpixels, from the quarter-resolution
logits and features in one call; neither the labels nor a full-resolution tensor need exist.
The only host synchronisation is in ``_after_epoch`` / ``total_*`` (one copy of 3C+3 integers).
"""
import numpy as np
import torch

from .. import ops


class MeanIoU:
    def __init__(self, num_classes, ignore_label, output_tensor='outputs', target_tensor='targets', name='iou'):
        self.num_classes = num_classes
        self.ignore_label = ignore_label
        self.name = name
        self.output_tensor = output_tensor
        self.target_tensor = target_tensor
        self._counts = None

    def _before_epoch(self):
        self._counts = None

    def _ensure(self, device):
        if self._counts is None:
            self._counts = torch.zeros(3 * self.num_classes + 3, dtype=torch.int64, device=device)
        return self._counts

    def _after_step(self, output_dict):
        outputs = output_dict[self.output_tensor]
        targets = output_dict[self.target_tensor]
        ops.iou_counts(outputs.contiguous(), None, targets.contiguous(), self.num_classes, self.ignore_label,
                       self._ensure(targets.device))

    def _host_counts(self):
        if self._counts is None:
            return np.zeros(3 * self.num_classes + 3, dtype=np.float64)
        return self._counts.cpu().numpy().astype(np.float64)

    def all_reduce(self, device=None):
        """Sum the integer counters over the ranks of an initialised process group (validation / stage-2 sets are
        sharded by rank).  A rank that saw no batch contributes zeros (``device`` tells it where to allocate them)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            if self._counts is None and device is not None:
                self._ensure(device)
            if self._counts is not None:
                dist.all_reduce(self._counts)

    @property
    def total_seen(self):
        return self._host_counts()[:self.num_classes]

    @property
    def total_correct(self):
        return self._host_counts()[self.num_classes:2 * self.num_classes]

    @property
    def total_positive(self):
        return self._host_counts()[2 * self.num_classes:3 * self.num_classes]

    def _after_epoch(self, ignore_label_list=None):
        c = self._host_counts()
        C = self.num_classes
        ious = []
        for i in range(C):
            if ignore_label_list is not None and i in ignore_label_list:
                continue
            seen, correct, positive = c[i], c[C + i], c[2 * C + i]
            ious.append(1 if seen == 0 else correct / (seen + positive - correct))
        return [v * 100 for v in ious]

    def _after_epoch_ipr(self):
        c = self._host_counts()
        C = self.num_classes
        ious, precs, recs = [], [], []
        for i in range(C):
            seen, correct, positive = c[i], c[C + i], c[2 * C + i]
            if seen == 0:
                ious.append(1); precs.append(1); recs.append(1)
            else:
                ious.append(correct / (seen + positive - correct))
                precs.append(correct / positive)
                recs.append(correct / seen)
        return ([v * 100 for v in ious], [v * 100 for v in precs], [v * 100 for v in recs])


class IoUIgnore(MeanIoU):
    """IoU of the "undefined" class -- ``utils/miou_evalignore.py:8-62``."""

    def _after_step(self, output_dict):
        outputs_all = output_dict[self.output_tensor]
        targets_all = output_dict[self.target_tensor]
        assert type(outputs_all) == torch.Tensor
        ops.iou_counts(None, outputs_all.contiguous(), targets_all.contiguous(), self.num_classes, self.ignore_label,
                       self._ensure(targets_all.device))

    def _ignore_counts(self):
        c = self._host_counts()
        return c[3 * self.num_classes], c[3 * self.num_classes + 1], c[3 * self.num_classes + 2]

    @property
    def total_seen(self):
        return self._ignore_counts()[0]

    @property
    def total_correct(self):
        return self._ignore_counts()[1]

    @property
    def total_positive(self):
        return self._ignore_counts()[2]

    def _after_epoch(self, ignore_label_list=None):
        seen, correct, positive = self._ignore_counts()
        if seen == 0:
            return 100.0
        return correct / (seen + positive - correct) * 100


class LogitsIoU(MeanIoU):
    """Both meters of ``ActiveTrainer.inference`` (``trainer/active_joint_multi_predignore.py:175-215``)
    from one pass over the logits: ``step(logits, labels)``; ``ious()`` / ``ignore_iou()``."""

    def step(self, logits, labels):
        ops.logits_iou_counts(logits.contiguous(), labels.contiguous(), self.num_classes, self.ignore_label,
                              self._ensure(logits.device))

    def ious(self):
        return self._after_epoch()

    def ignore_iou(self):
        c = self._host_counts()
        seen, correct, positive = c[3 * self.num_classes:3 * self.num_classes + 3]
        return 100.0 if seen == 0 else correct / (seen + positive - correct) * 100


class LowresLogitsIoU(LogitsIoU):
    """``LogitsIoU`` fed the network's quarter-resolution logits: ``step_lowres(z_q, labels)`` counts what ``step`` counts on
    ``ops.upsample_bilinear(z_q, labels.shape[-2:])``, counter for counter (``ops.lowres_iou_counts``)."""

    def step_lowres(self, z_q, labels):
        ops.lowres_iou_counts(z_q.contiguous(), labels.contiguous(), labels.shape[-2:], self.num_classes, self.ignore_label,
                              self._ensure(z_q.device))


class MultiScaleLogitsIoU(LogitsIoU):
    """``LogitsIoU`` for multi-scale + flip evaluation: ``step_ms(logits_q, sizes, flips, labels)`` counts what ``step`` counts on the
    mean logits of the copies (``ops.ms_ensemble``'s logits) against ``labels`` [1,H,W], from the copies' quarter-resolution logits
    (``ops.ms_iou_counts``)."""

    def step_ms(self, logits_q, sizes, flips, labels):
        ops.ms_iou_counts([z.contiguous() for z in logits_q], sizes, flips, labels.shape[-2:], labels.contiguous(), self.num_classes,
                          self.ignore_label, self._ensure(logits_q[0].device))


class WithinMultihotIoU(MeanIoU):
    """``MeanIoU`` of the local-prototype labels inside the queried superpixels (``trainer/eval_cosplbl_within_multihot.py:84-179`` and
    its ``filt`` sibling): ``step_within(zq, featq, spx, mask, targets, labels, mode)`` counts what ``_after_step`` counts on the label
    map those generate from ``feat_forward``'s tensors, from the quarter-resolution logits and features (``ops.within_multihot_eval``).
    ``diag`` int64 [4] on the device, added to by every step: valid pixels, prototypes, valid pixels whose winning similarity is below
    ``max_c (logit_c * Y_c)``, labels removed by the filter."""

    diag = None

    def _before_epoch(self):
        super()._before_epoch()
        self.diag = None

    def step_within(self, zq, featq, spx, mask, targets, labels, mode='proto', want_labels=False):
        if self.diag is None:
            self.diag = torch.zeros(4, dtype=torch.int64, device=zq.device)
        targets = targets if targets.dtype == torch.uint8 else targets.to(torch.uint8)
        return ops.within_multihot_eval(zq.contiguous(), featq.contiguous(), labels.shape[-2:], spx.contiguous(), mask.contiguous(),
                                        labels.contiguous(), targets=targets.contiguous(), mode=mode, num_classes=self.num_classes,
                                        ignore_label=self.ignore_label, counts=self._ensure(zq.device), diag=self.diag,
                                        want_labels=want_labels)[2]
