"""Float64 torch restatement of the partial-label baselines (not collected: no ``test_`` prefix) -- the yardstick that is not the code
under test.  From the definitions, not from csrc/partial_label.h:

  * ``rc_merged``      reference ``utils/loss.py:653-707`` (RCMultiChoiceCE): one merged sum over every selected pixel with a target,
                       each candidate's ``-log(p_c + eps)`` weighted by the detached ``p_c / sum_Y p``;
  * ``decomp(mode)``   (ce over one-hot pixels, mc over multi-hot pixels), mc = 'choice' ``-log(sum_Y p + eps)``,
                       'topone' ``-log(max_Y p + eps)`` (``trainer/active_joint_multi_lossdecomp_topone.py:14-71``) or 'rc' (the
                       term above restricted to multi-hot pixels -- what ``..._lossdecomp_rc.py`` means).

Every normaliser is 1 + n (``utils/loss.py:556``).  ``per_pixel`` returns the three multi-hot terms pixel by pixel for the
mathematical ordering choice <= topone <= rc: a maximum is at most the sum, and a weighted mean of ``-log p_c`` is at least
``-log max p_c``."""
import numpy as np
import torch

EPS = 1e-8


def _pixels(z, tgt, spx, msk, T, cols=None):
    """(probabilities [P,C] f64 with grad, multi-hot rows [P,C] f64) of the selected pixels that have a target, and the leaf z."""
    zt = torch.from_numpy(np.asarray(z, dtype=np.float32)).to(torch.float64).requires_grad_(True)
    N, C, H, W = zt.shape
    p = torch.softmax(zt.permute(0, 2, 3, 1).reshape(N, H * W, C) / T, dim=2)
    tg = torch.from_numpy(np.asarray(tgt)).to(torch.float64)
    if cols is not None:
        tg = tg[..., :cols]
    if tg.shape[-1] < C:
        tg = torch.cat([tg, torch.zeros(tg.shape[:-1] + (C - tg.shape[-1],), dtype=torch.float64)], dim=-1)
    sp = torch.from_numpy(np.asarray(spx, dtype=np.int64)).reshape(N, H * W)
    mk = torch.from_numpy(np.asarray(msk).astype(bool)).reshape(N, H * W)
    ps, ys = [], []
    for i in range(N):
        ps.append(p[i][mk[i]])
        ys.append(tg[i][sp[i][mk[i]]])
    p, y = torch.cat(ps), torch.cat(ys)
    keep = y.sum(dim=1) > 0
    return p[keep], y[keep], zt


def _terms(p, y):
    """per pixel: (choice, topone, rc) terms"""
    q = p * y
    s = q.sum(dim=1)
    choice = -torch.log(s + EPS)
    topone = -torch.log(q.max(dim=1)[0] + EPS)
    w = (q / s[:, None]).detach()
    rc = (w * -torch.log(q + EPS)).sum(dim=1)
    return choice, topone, rc


def per_pixel(z, tgt, spx, msk, T):
    """The three terms of the MULTI-HOT pixels, numpy f64 [P'] each."""
    p, y, _ = _pixels(z, tgt, spx, msk, T)
    multi = y.sum(dim=1) > 1
    with torch.no_grad():
        return tuple(t[multi].numpy() for t in _terms(p, y))


def tie_count(z, tgt, spx, msk, T, rel=1e-5):
    """(multi-hot pixels whose two largest candidate probabilities differ by less than ``rel`` relative, multi-hot pixels)."""
    p, y, _ = _pixels(z, tgt, spx, msk, T)
    multi = y.sum(dim=1) > 1
    with torch.no_grad():
        q = (p * y)[multi]
        if q.shape[0] == 0:
            return 0, 0
        top = torch.topk(q, 2, dim=1)[0]
        return int(((top[:, 0] - top[:, 1]) < rel * top[:, 0]).sum()), int(q.shape[0])


def _with_grad(zt, ce, mc, w_ce, w_mc):
    (g,) = torch.autograd.grad(w_ce * ce + w_mc * mc, zt)
    return float(ce), float(mc), g.numpy()


def decomp(mode, z, tgt, spx, msk, T, w_ce=16.0, w_mc=8.0):
    """(ce, mc, gradient of w_ce * ce + w_mc * mc with respect to z) in float64."""
    p, y, zt = _pixels(z, tgt, spx, msk, T)
    nb = y.sum(dim=1)
    choice, topone, rc = _terms(p, y)
    one, multi = nb == 1, nb > 1
    ce = choice[one].sum() / (1 + int(one.sum()))
    mc = {'choice': choice, 'topone': topone, 'rc': rc}[mode][multi].sum() / (1 + int(multi.sum()))
    return _with_grad(zt, ce, mc, w_ce, w_mc)


def rc_merged(z, tgt, spx, msk, T, w=16.0):
    """RCMultiChoiceCE: (loss, 0, gradient of w * loss); the last target column is dropped."""
    p, y, zt = _pixels(z, tgt, spx, msk, T, cols=np.asarray(tgt).shape[-1] - 1)
    rc = _terms(p, y)[2]
    loss = rc.sum() / (1 + rc.shape[0])
    return _with_grad(zt, loss, loss * 0.0, w, 0.0)
