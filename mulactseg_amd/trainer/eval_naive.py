"""Evaluation of a stage-2 checkpoint -- reference ``trainer/eval_naive.py:11-80`` (``script/open_source/eval_city_mul_res50.sh``:
``eval_AL.py --init_checkpoint checkpoint/stage2_checkpoint0N.tar --stage2 --method eval_naive --loader region_cityscapes_all
--train_transform eval_spx --val_batch_size 1``): the (num_classes + 1)-channel model of ``active_joint_multi_predignore`` on the
evaluation set, one table of mIoU, the per-class IoUs and the IoU of the "undefined" class.  Unlike ``BaseTrainer.eval`` nothing goes
to wandb or ``wandb_iou_table`` (the reference's ``eval_naive`` does neither).

The network stops at quarter resolution (``net(images, lowres=True)``) and ``LowresLogitsIoU`` (``csrc/lowres_iou.hip``) upsamples
per pixel in registers while it counts: the full-resolution logits (168 MB per 1024 x 2048 picture) never exist, and the counters
equal those of ``LogitsIoU`` on ``net(images)``.  ``MAS_EVAL_NAIVE=full``, a model without quarter-resolution logits or a geometry
``ops.lowres_iou_supported`` declines take ``net(images)`` + ``LogitsIoU``."""
import os

import numpy as np
import torch

from .. import ops
from ..dataloader import get_dataset
from ..utils.miou import LowresLogitsIoU
from . import active_joint_multi_predignore


class ActiveTrainer(active_joint_multi_predignore.ActiveTrainer):
    def eval(self, active_set, selection_iter):
        """The evaluation set of ``--val_dataset`` / ``--val_data_dir`` / ``--val_datalist`` (``active_set`` is not read, as in the
        reference); logs and returns the table."""
        a = self.args
        eval_dataset = get_dataset(a, name=a.val_dataset, data_root=a.val_data_dir, datalist=a.val_datalist, imageset='eval')
        self.eval_dataset_loader = self.get_valloader(eval_dataset)
        miou, table = self.inference(loader=self.eval_dataset_loader, prefix='evaluation')
        self.logger.info('[Evaluation Result]')
        self.logger.info('%s' % table)
        self.logger.info('Current eval miou is %.3f %%' % miou)
        return table

    def _lowres(self):
        return os.environ.get("MAS_EVAL_NAIVE", "lowres") != "full" and getattr(self.net, 'lowres_logits', False)

    def inference(self, loader, prefix=''):
        """(mIoU, table): ``'%.2f'`` of the mIoU, the C per-class IoUs and the "undefined" IoU, comma-joined; counters summed over
        the ranks.  The round printed is the constructor's ``selection_iter`` (the reference's)."""
        meter = LowresLogitsIoU(self.num_classes, self.args.ignore_idx)
        meter._before_epoch()
        lowres = self._lowres()
        self.net.eval()
        with torch.no_grad():
            for _ in range(len(loader)):
                batch = next(loader)
                images = batch['images'].to(self.device, dtype=torch.float32)
                labels = batch['labels'].to(self.device, dtype=torch.long)
                if lowres:
                    z_q = self.net(images, lowres=True)
                    if ops.lowres_iou_supported(z_q, labels.shape[-2:]):
                        meter.step_lowres(z_q, labels)
                        continue
                meter.step(self.net(images).detach(), labels)
        meter.all_reduce(self.device)
        ious = meter.ious()
        miou = np.mean(ious)
        table = ','.join(['%.2f' % miou] + ['%.2f' % v for v in ious] + ['%.2f' % meter.ignore_iou()])
        print("\n[AL {}-round]: {}\n{}".format(self.selection_iter, prefix, table), flush=True)
        return miou, table
