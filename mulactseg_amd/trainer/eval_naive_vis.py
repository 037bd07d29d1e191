"""``eval_naive`` with pictures -- reference ``trainer/eval_naive_vis.py`` (the qualitative figures of the paper's supplement): the same
table, plus for the FIRST picture of every batch ``vis/neurips23_supp_qual/round_RR/<lbl_id>.png``, the colour image of
``preds[:, :-1].max(1)[1]`` (RR = ``init_checkpoint[-6:-4]``; relative to the working directory), and with ``--save_vis``
``vis/neurips23_supp_qual/gt/<lbl_id>.png``, the ground truth with 255 painted as "undefined" (19).  Both are exact palette colours
(no ``mark_boundaries``).

On the quarter-resolution path the prediction image comes from ``ops.render_lowres_pred`` (``csrc/render.hip``): the full-resolution
logits never exist, as for the counters.  ``MAS_EVAL_NAIVE=full`` renders ``net(images)[:, :-1].max(1)[1]`` with
``ops.render_labels``.  The PNGs are encoded by a small writer pool, so the encoding of the 6 MB pictures does not hold up the loop."""
import collections
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import ops
from ..dataloader.constant import train_id_to_color
from ..utils.miou import LowresLogitsIoU
from . import eval_naive

VIS_ROOT = 'vis/neurips23_supp_qual'
WRITERS = 4


class ActiveTrainer(eval_naive.ActiveTrainer):
    vis_palette = train_id_to_color
    gt_fill = 19

    def _palette(self, dev):
        pal = getattr(self, '_vis_pal', None)
        if pal is None or pal.device != dev:
            pal = self._vis_pal = torch.from_numpy(self.vis_palette.astype('uint8')).to(dev)
        return pal

    def inference(self, loader, prefix=''):
        """``eval_naive.inference`` plus the pictures; same table, same return value."""
        from PIL import Image
        a = self.args
        rnd = a.init_checkpoint.split('/')[-1][-6:-4]
        save_dir_gt, save_dir = '{}/gt'.format(VIS_ROOT), '{}/round_{}'.format(VIS_ROOT, rnd)
        os.makedirs(save_dir_gt, exist_ok=True)
        os.makedirs(save_dir, exist_ok=True)
        save_vis = getattr(a, 'save_vis', False)
        meter = LowresLogitsIoU(self.num_classes, a.ignore_idx)
        meter._before_epoch()
        lowres = self._lowres()
        self.net.eval()
        pending = collections.deque()

        def write(rgb, path):
            """rgb: a [1,H,W,3] device tensor; its copy waits for this stream, the encoding goes to the pool."""
            arr = rgb[0].cpu().numpy()
            while len(pending) >= 2 * WRITERS:              # (bounded: at most 2 x WRITERS pictures held on the host)
                pending.popleft().result()
            pending.append(pool.submit(lambda: Image.fromarray(arr).save(path)))

        with ThreadPoolExecutor(max_workers=WRITERS) as pool, torch.no_grad():
            for _ in range(len(loader)):
                batch = next(loader)
                images = batch['images'].to(self.device, dtype=torch.float32)
                labels = batch['labels'].to(self.device, dtype=torch.long)
                lbl_id = batch['fnames'][0][1].split('/')[-1].split('.')[0]
                pal = self._palette(labels.device)
                if save_vis:
                    write(ops.render_labels(labels[:1].contiguous(), pal, self.gt_fill), "{}/{}.png".format(save_dir_gt, lbl_id))
                if lowres:
                    z_q = self.net(images, lowres=True)
                    if ops.lowres_iou_supported(z_q, labels.shape[-2:]):
                        meter.step_lowres(z_q, labels)
                        write(ops.render_lowres_pred(z_q[:1].contiguous(), labels.shape[-2:], pal), "{}/{}.png".format(save_dir, lbl_id))
                        continue
                preds = self.net(images).detach()
                meter.step(preds, labels)
                pred_within = preds[:1, :-1].max(dim=1)[1]
                write(ops.render_labels(pred_within.contiguous(), pal, self.gt_fill), "{}/{}.png".format(save_dir, lbl_id))
            while pending:
                pending.popleft().result()
        meter.all_reduce(self.device)
        ious = meter.ious()
        miou = np.mean(ious)
        table = ','.join(['%.2f' % miou] + ['%.2f' % v for v in ious] + ['%.2f' % meter.ignore_iou()])
        print("\n[AL {}-round]: {}\n{}".format(self.selection_iter, prefix, table), flush=True)
        return miou, table
