"""Quality of the local-prototype pseudo labels where they are made: inside the queried superpixels of the labelled set -- reference
``trainer/eval_cosplbl_within_multihot.py:16-179`` (``--method eval_cosplbl_within_multihot``).  Every selected pixel of a superpixel
with a non-empty row takes the candidate class whose local prototype (the superpixel's pixel with the largest softmax probability of
that class) is nearest to its own feature; the result is measured against the ground truth: IoU, precision and recall per class.

The reference runs ``feat_forward`` ([N,256,H,W] features, 2.1 GB per 1024 x 2048 picture) and a dense prototypes x pixels product
per picture.  Here the network stops at quarter resolution (``feat_forward_quarter``) and one library call per batch
(``ops.within_multihot_eval``, csrc/within_eval.hip) interpolates both maps per pixel, picks the prototypes, labels and counts: no
label map, no full-resolution tensor, no host round trip inside the loop.  ``MAS_WITHIN_EVAL=aten`` takes ``pseudo_label_generation``
instead, the reference's lines restated with torch operations on ``feat_forward``'s materialised tensors (for comparison).

A selected superpixel with an empty row makes the reference raise (``:162``, a size mismatch); here its pixels stay 255.

The three siblings derive from this class: ``eval_cosplbl_filt_within_multihot`` (``mode = 'filt'``), ``eval_maxcosplbl_within_multihot``
(``counts_below``) and ``eval_ensemble_plbl_within_multihot``; each prints what its reference file prints."""
import os

import numpy as np
import torch

from ..utils.miou import WithinMultihotIoU
from . import eval_within_multihot


class ActiveTrainer(eval_within_multihot.ActiveTrainer):
    meter_class = WithinMultihotIoU
    mode = 'proto'
    tables = ('IoU', 'Precision', 'Recall')     # (:78-80); the siblings print the single table of the base class
    counts_below = False                        # eval_maxcosplbl_within_multihot: print the count of diag[2] of every batch

    def fused(self):
        return (os.environ.get("MAS_WITHIN_EVAL", "fused") != "aten" and torch.device(self.device).type == 'cuda'
                and hasattr(self.net, 'feat_forward_quarter'))

    def generate_batch(self, batch, meter):
        images, labels, superpixels, spmasks, targets = self._batch(batch)
        log = self.__dict__.setdefault('_below', [])            # running totals on the device: no host wait inside the loop
        if self.fused():
            feats, outputs = self.net.feat_forward_quarter(images)
            meter.step_within(outputs.detach(), feats.detach(), superpixels, spmasks, targets, labels, mode=self.mode)
            log.append(meter.diag[2:3].clone())
        else:
            feats, outputs = self.net.feat_forward(images)
            plbl, n_below = self.pseudo_label_generation(labels, feats.detach(), outputs.detach(), targets, spmasks, superpixels,
                                                         with_below=True)
            meter._after_step({'outputs': plbl, 'targets': labels})
            log.append(n_below + log[-1] if log else n_below)

    def inference(self, loader, prefix=''):
        self._below = []
        return super().inference(loader, prefix)

    def report(self, meter, prefix):
        if self.counts_below:                   # (eval_maxcosplbl_within_multihot.py:169, there per picture)
            prev = 0
            for t in self.__dict__.get('_below', []):
                now = int(t.item())
                print(now - prev)
                prev = now
        if len(self.tables) == 1:
            return super().report(meter, prefix)
        rows = meter._after_epoch_ipr()
        strings = [','.join(['%.2f' % np.mean(r)] + ['%.2f' % v for v in r]) for r in rows]
        for name, s in zip(self.tables, strings):
            print("\n[AL {}-round] {}: {}\n{}".format(self.selection_iter, name, prefix, s), flush=True)
        return np.mean(rows[0]), strings[0]

    def pseudo_label_generation(self, labels, feats, inputs, targets, spmasks, superpixels, with_below=False):
        """The reference's signature (:84): ``feats`` [N,Ch,H,W] and ``inputs`` [N,C,H,W] at full resolution -> label map int64 [N,H,W]
        (255 off the valid pixels); with ``with_below`` also the number of valid pixels whose winning similarity is below
        ``max_c (logit_c * Y_c)`` (int64 [1])."""
        N, C, H, W = inputs.shape
        S, Ch = targets.shape[1], feats.shape[1]
        prob = torch.softmax(inputs, dim=1).reshape(N, C, -1)
        out = torch.full((N, H * W), 255, dtype=torch.long, device=inputs.device)
        n_below = torch.zeros(1, dtype=torch.int64, device=inputs.device)
        for i in range(N):
            ids = superpixels[i].reshape(-1).long()
            rows = targets[i] != 0                                                  # S x cols
            valid = spmasks[i].reshape(-1).bool() & (ids >= 0) & (ids < S)
            valid = valid & rows.any(dim=1)[ids.clamp(0, S - 1)]
            vpx = valid.nonzero().squeeze(1)
            nv = vpx.numel()
            if nv == 0:
                continue
            vid = ids[vpx]
            p = prob[i][:, vpx].t()                                                 # nv x C
            z = inputs[i].reshape(C, -1)[:, vpx].t()
            f = feats[i].reshape(Ch, -1)[:, vpx].t()                                # nv x Ch
            cand = rows[vid][:, :C]                                                 # nv x C
            index = vid[:, None].expand(-1, C)
            top = torch.full((S, C), -1.0, dtype=p.dtype, device=p.device).scatter_reduce(0, index, p, 'amax')
            pos = torch.arange(nv, device=p.device)[:, None].expand(-1, C)
            first = torch.full((S, C), nv, dtype=torch.long, device=p.device).scatter_reduce(
                0, index, torch.where(p == top[vid], pos, torch.full_like(pos, nv)), 'amin')      # S x C: the prototype, as a valid index
            best = torch.full((nv,), float('-inf'), dtype=f.dtype, device=f.device)
            lab = torch.full((nv,), 255, dtype=torch.long, device=f.device)
            own = torch.full((nv,), -1, dtype=torch.long, device=f.device)          # the highest class the pixel is the prototype of
            for c in range(C):
                sel = cand[:, c].nonzero().squeeze(1)
                if sel.numel() == 0:
                    continue
                proto = first[vid[sel], c]
                sim = (f[sel] * f[proto]).sum(dim=1)
                better = sim > best[sel]
                best[sel] = torch.where(better, sim, best[sel])
                lab[sel] = torch.where(better, torch.full_like(sel, c), lab[sel])
                own[sel] = torch.where(proto == sel, torch.full_like(sel, c), own[sel])
            n_below += ((best < (z * cand.to(z.dtype)).max(dim=1)[0]) & (lab != 255)).sum()
            if self.mode == 'filt':                                                 # (eval_cosplbl_filt_within_multihot.py:162-169)
                lab = torch.where(p.argmax(dim=1) == lab, lab, torch.full_like(lab, 255))
                lab = torch.where(own >= 0, own, lab)
            out[i, vpx] = lab
        out = out.reshape(N, H, W)
        return (out, n_below) if with_below else out
