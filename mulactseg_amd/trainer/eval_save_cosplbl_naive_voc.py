"""Naive arg-max pseudo labels for PASCAL VOC, the README's "Naive Inference" -- reference ``trainer/eval_save_cosplbl_naive_voc.py:29-124``
(``--method eval_save_cosplbl_naive_voc --train_transform eval_spx_identity --loader eval_region_voc_all --plbl_type naive_argmax``):
per picture, at its own size, ``outputs.max(dim=1)[1]`` over all C = 21 channels -- every pixel gets a label, no mask, no 255 --
counted by ``MeanIoU(num_classes + 1, ignore_idx)`` against the class map whose void 255 the loader turned into class 21 (so class 21
is seen and never predicted: IoU 0, precision nan).  Saved as uint8 PNGs under ``plbl_gen_<plbl_type>/round_RR`` (``plbl_gen``
without a type) with the ``--save_vis`` pictures of ``eval_save_cosplbl_prop_includeonehot_voc``; three tables (IoU, precision,
recall) are printed (:107-122).

On the GPU the network stops at quarter resolution (``net(x, lowres=True)``) and one kernel (``ops.ms_naive_labels``,
csrc/ms_naive.hip) upsamples, takes the arg-max and adds the IoU counters to the meter: the full-resolution logits never exist.
``MAS_MS_NAIVE=aten`` takes the reference's ATen chain instead.  The pictures go through the threaded loop of
``eval_save_cosplbl_prop.inference``."""
import numpy as np
import torch

from .. import ops
from . import eval_save_cosplbl_prop_includeonehot_voc


class ActiveTrainer(eval_save_cosplbl_prop_includeonehot_voc.ActiveTrainer):
    threaded_generation = True          # (no state between pictures)

    def sources(self, batch):
        """-> (quarter-resolution logits [1,C,hq,wq] per source, the scaled sizes the network saw, flips): the picture itself."""
        images = batch['images'].to(self.device, dtype=torch.float32)
        return [self.net(images, lowres=True).contiguous()], [tuple(images.shape[-2:])], [False]

    def pseudo_labels(self, images, labels, targets, spmasks, superpixels):
        return ops.ms_naive_labels([self.net(images, lowres=True).contiguous()], [tuple(images.shape[-2:])], [False], images.shape[-2:])

    def generate_batch(self, batch, meter):
        """Labels and counters from one launch: the kernel adds ``MeanIoU._after_step``'s counts to the meter's buffer itself."""
        labels = batch['labels'].to(self.device, dtype=torch.long)
        logits_q, sizes, flips = self.sources(batch)
        plbl = ops.ms_naive_labels(logits_q, sizes, flips, labels.shape[-2:], targets=labels.contiguous(),
                                   counts=meter._ensure(labels.device), num_classes=meter.num_classes, ignore_label=meter.ignore_label)
        self.after_batch(batch, plbl)

    def report(self, meter, prefix):
        """The three tables of the reference (:96-122): mean + per class, ``%.2f``; returns (mIoU, IoU table)."""
        ious, precisions, recalls = meter._after_epoch_ipr()
        tables = [','.join(['%.2f' % np.mean(v)] + ['%.2f' % x for x in v]) for v in (ious, precisions, recalls)]
        for name, table in zip(('IoU', 'Precision', 'Recall'), tables):
            print("\n[AL {}-round] {}: {}\n{}".format(self.selection_iter, name, prefix, table), flush=True)
        return np.mean(ious), tables[0]
