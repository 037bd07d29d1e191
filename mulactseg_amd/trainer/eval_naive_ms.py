"""Multi-scale + flip evaluation of a stage-2 checkpoint: ``--method eval_naive_ms`` with the argument sets of ``eval_AL.py`` and
``eval_AL_voc.py``.  The reference evaluates one pass (``trainer/eval_naive.py:11-80``) and leaves VOC evaluation as a README TODO; this
is the protocol of its multi-scale generators (``trainer/eval_save_cosplbl_naive_voc_ms.py:55-92``: five scales, then the same five
flipped, logits flipped back, resized to the picture and averaged) applied to ``eval_naive``'s counters: every picture of
``--val_datalist`` at its own size, ``--ms_factors`` scales (and their flips unless ``--ms_noflip``), the table of ``eval_naive`` (mIoU,
per-class IoUs, "undefined" IoU).  ``--ms_factors 1.0 --ms_noflip`` is the plain evaluation on whole pictures.

Every forward stops at quarter resolution (``net(x, lowres=True)``) and one kernel per picture (``ops.ms_iou_counts``,
csrc/ms_naive.hip) upsamples, flips back, resizes, averages, takes both arg-maxes and counts: no full-resolution logits exist.
``MAS_MS_EVAL=aten`` materialises the chain in ATen from the same quarter-resolution logits.  A model without quarter-resolution
logits, or a geometry ``ops.ms_iou_supported`` declines, takes ``net(x)`` per copy, the average in ATen and ``LogitsIoU``."""
import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..dataloader.eval_ms import get_ms_eval_dataset
from ..dataloader.utils import ResidentProvider
from ..utils.miou import MultiScaleLogitsIoU
from . import eval_naive


class ActiveTrainer(eval_naive.ActiveTrainer):
    def eval(self, active_set, selection_iter):
        a = self.args
        dataset = get_ms_eval_dataset(a.val_dataset, a.val_data_dir, a.val_datalist, factors=a.ms_factors, flip=not a.ms_noflip)
        self.eval_dataset_loader = self.get_ownsize_loader(dataset)
        miou, table = self.inference(loader=self.eval_dataset_loader, prefix='evaluation')
        self.logger.info('[Evaluation Result]')
        self.logger.info('%s' % table)
        self.logger.info('Current eval miou is %.3f %%' % miou)
        return table

    def get_ownsize_loader(self, dataset):
        """``get_valloader`` with one picture per batch: the pictures keep their own sizes and do not stack."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dataset = torch.utils.data.Subset(dataset, range(dist.get_rank(), len(dataset), dist.get_world_size()))
        return ResidentProvider(dataset, batch_size=1, drop_last=False, shuffle=False)

    def _mean_full(self, images, flips, size):
        """The mean logits [1,CH,H,W] from full-resolution forwards (the fall-back)."""
        acc = None
        for img, fl in zip(images, flips):
            z = self.net(img[None]).detach()
            v = F.interpolate(z.flip(-1) if fl else z, size=size, mode='bilinear', align_corners=False)
            acc = v if acc is None else acc + v
        return acc / len(images)

    def inference(self, loader, prefix=''):
        meter = MultiScaleLogitsIoU(self.num_classes, self.args.ignore_idx)
        meter._before_epoch()
        lowres = getattr(self.net, 'lowres_logits', False)
        self.net.eval()
        with torch.no_grad():
            for _ in range(len(loader)):
                batch = next(loader)
                images = [img.to(self.device, dtype=torch.float32) for img in batch['image_list'][0]]
                labels = batch['labels'].to(self.device, dtype=torch.long)
                n = len(images)
                flips = [not self.args.ms_noflip and k >= n // 2 for k in range(n)]
                sizes = [tuple(img.shape[-2:]) for img in images]
                if lowres:
                    logits_q = [self.net(img[None], lowres=True).contiguous() for img in images]
                    if ops.ms_iou_supported(logits_q, sizes, flips, labels.shape[-2:]):
                        meter.step_ms(logits_q, sizes, flips, labels)
                        continue
                    del logits_q
                meter.step(self._mean_full(images, flips, tuple(labels.shape[-2:])), labels)
        meter.all_reduce(self.device)
        ious = meter.ious()
        miou = np.mean(ious)
        table = ','.join(['%.2f' % miou] + ['%.2f' % v for v in ious] + ['%.2f' % meter.ignore_iou()])
        print("\n[AL {}-round]: {}\n{}".format(self.selection_iter, prefix, table), flush=True)
        return miou, table
