"""Top-1 within the candidate set -- reference ``trainer/eval_save_candidateplbl.py:13-95`` (``--method eval_save_candidateplbl --loader
eval_region_cityscapes_all --train_transform eval_spx --or_labeling``): every selected pixel gets ``argmax_c (logit_c * Y_c)`` over its
superpixel's multi-hot row Y (``top_pseudo_label_generation``; raw logits, so a row whose candidate logits are all negative yields the
first excluded channel -- replicated), everything else 255.  Saved as uint8 PNGs under ``plbl_gen_<plbl_type>/round_RR`` (``plbl_gen``
without a type).

On the GPU the network stops at quarter resolution and one kernel (``ops.candidate_pseudo_labels``, csrc/candidate_plbl.hip) upsamples,
takes the arg-max within the row's bits and adds the IoU counters to the meter: neither the full-resolution logits nor the per-pixel copy
of the rows exist.  ``MAS_CANDIDATE_PLBL=aten`` takes the reference's ATen lines instead.  The pictures go through the threaded loop of
``eval_save_cosplbl_prop.inference``."""
from .. import ops
from . import eval_save_cosplbl_prop


class ActiveTrainer(eval_save_cosplbl_prop.ActiveTrainer):
    threaded_generation = True          # (no state between pictures)
    fallback = False                    # eval_save_candidateplbl_prop: the thresholded top-1 outside the selected superpixels

    def _labels(self, images, labels, targets, spmasks, superpixels, meter=None):
        if getattr(self.net, 'lowres_logits', False):
            z = self.net(images, lowres=True)
        else:
            z = self.net(images)
        count = {} if meter is None else dict(targets=labels.contiguous(), counts=meter._ensure(labels.device),
                                              num_classes=meter.num_classes, ignore_label=meter.ignore_label)
        return ops.candidate_pseudo_labels(z.contiguous(), images.shape[-2:], spmasks, targets_rows=targets.contiguous(),
                                           superpixels=superpixels.contiguous(), fallback=self.fallback,
                                           th=getattr(self.args, 'plbl_th', 0.0), ce_temp=getattr(self.args, 'ce_temp', 1.0), **count)

    def pseudo_labels(self, images, labels, targets, spmasks, superpixels):
        return self._labels(images, labels, targets, spmasks, superpixels)

    def generate_batch(self, batch, meter):
        """Labels and counters from one launch: the kernel adds ``MeanIoU._after_step``'s counts to the meter's buffer itself."""
        images, labels, superpixels, spmasks, targets = self._batch(batch)
        self.after_batch(batch, self._labels(images, labels, targets, spmasks, superpixels, meter))
