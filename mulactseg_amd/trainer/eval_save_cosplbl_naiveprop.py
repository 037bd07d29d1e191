"""Prototype labels inside the selected superpixels, a confidence-thresholded top-1 everywhere else -- reference
``trainer/eval_save_cosplbl_naiveprop.py:14-108`` (``--method eval_save_cosplbl_naiveprop --plbl_th P --ce_temp T --loader
eval_region_cityscapes_all --train_transform eval_spx --or_labeling``): the labels of ``eval_save_cosplbl`` under the mask; outside it
the arg-max of the logits where ``softmax(logits / ce_temp).max > plbl_th`` (the line runs for every ``plbl_th``, 0 included: then every
unselected pixel gets its top-1), 255 elsewhere.  The usual self-training baseline the prototype expansion is compared with.

On the GPU the network stops at quarter resolution; the assignment runs on the quarter-resolution features
(``ops.stage2_pseudo_labels(expand=False)``) and one kernel (``ops.candidate_pseudo_labels``, csrc/candidate_plbl.hip) upsamples the
logits per pixel, merges the assignment with the thresholded top-1 and adds the IoU counters to the meter.
``MAS_CANDIDATE_PLBL=aten`` takes the reference's ATen lines instead."""
import torch.nn.functional as F

from .. import ops
from . import eval_save_cosplbl


class ActiveTrainer(eval_save_cosplbl.ActiveTrainer):
    def _labels(self, images, labels, targets, spmasks, superpixels, meter=None):
        size = images.shape[-2:]
        if hasattr(self.net, 'feat_forward_quarter'):
            feats, z = self.net.feat_forward_quarter(images)
            z = z.contiguous()
            if z.is_cuda and ops.upsample_bilinear_supported(z, size):     # (the assignment's prototype table reads full-resolution logits)
                outputs = ops.upsample_bilinear(z, size)
            else:
                outputs = F.interpolate(z, size=size, mode='bilinear', align_corners=False)
        else:
            feats, outputs = self.net.feat_forward_lowres(images)
            z = outputs
        inner = self.pseudo_label_generation(labels, feats, outputs, targets, spmasks, superpixels)
        count = {} if meter is None else dict(targets=labels.contiguous(), counts=meter._ensure(labels.device),
                                              num_classes=meter.num_classes, ignore_label=meter.ignore_label)
        return ops.candidate_pseudo_labels(z.contiguous(), size, spmasks, inner=inner, fallback=True,
                                           th=getattr(self.args, 'plbl_th', 0.0), ce_temp=getattr(self.args, 'ce_temp', 1.0), **count)

    def pseudo_labels(self, images, labels, targets, spmasks, superpixels):
        return self._labels(images, labels, targets, spmasks, superpixels)

    def generate_batch(self, batch, meter):
        """Labels and counters from one launch: the kernel adds ``MeanIoU._after_step``'s counts to the meter's buffer itself."""
        images, labels, superpixels, spmasks, targets = self._batch(batch)
        self.after_batch(batch, self._labels(images, labels, targets, spmasks, superpixels, meter))
