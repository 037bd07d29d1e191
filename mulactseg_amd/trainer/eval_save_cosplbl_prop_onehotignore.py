"""Cosine prototypes + propagation from DOMINANT-label queries, the stage-2 ablation of paper Fig. 7 (b) -- reference
``trainer/eval_save_cosplbl_prop_onehotignore.py:29-58,84-105`` (``--method eval_save_cosplbl_prop_onehotignore --dominant_labeling
--loader region_cityscapes_dom_w_gt --train_transform eval_dom_gt_spx``).  Per picture the query mask is ``target != 255`` and each
superpixel's target row is the one-hot of its largest target value (``scatter_max``; 255 read as class 19); the rest is the
``_includeonehot`` generator (every masked pixel takes part, no multi-hot restriction).  Both the mask and the rows come from one
kernel pass (``ops.spx_max_onehot``, csrc/labels.hip).  The reference prints IoU, precision and recall tables (:84-105)."""
import numpy as np
import torch

from .. import ops
from . import eval_save_cosplbl_prop


class ActiveTrainer(eval_save_cosplbl_prop.ActiveTrainer):
    include_onehot = True
    threaded_generation = True          # (no state between pictures)

    def pseudo_labels(self, images, labels, targets, spmasks, superpixels):
        rows, masks = [], []
        for i in range(targets.shape[0]):
            r, m = ops.spx_max_onehot(targets[i].contiguous(), superpixels[i].contiguous(), self.args.nseg, self.num_classes + 1)
            rows.append(r), masks.append(m)
        return super().pseudo_labels(images, labels, torch.stack(rows), torch.stack(masks), superpixels)

    def report(self, meter, prefix):
        ious, precisions, recalls = meter._after_epoch_ipr()
        tables = [','.join(['%.2f' % np.mean(v)] + ['%.2f' % x for x in v]) for v in (ious, precisions, recalls)]
        for name, table in zip(('IoU', 'Precision', 'Recall'), tables):
            print("\n[AL {}-round] {}: {}\n{}".format(self.selection_iter, name, prefix, table), flush=True)
        return np.mean(ious), tables[0]
