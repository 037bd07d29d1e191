"""Float64 torch restatement of the teacher-gated candidate terms (not collected: no ``test_`` prefix) -- the yardstick that is not the
code under test.  Written from the formulas, not from csrc/teacher_terms.h and not from the reference's code:

  * ``top1``  over the selected pixels of multi-hot superpixels: p = softmax(z / T), t = softmax(z_teacher / T);
              g = max_{c in Y} t_c (``within``: divided by sum_{c in Y} t_c); the pixel counts iff th < g;
              l = -log(max_{c in Y} p_c + eps); the term is sum l / (1 + n_counted); the teacher carries no gradient.
  * ``ent``   over the same pixels: q = softmax over {c in Y : z_c != 0} of z_c / T; h = -sum q_c log(q_c + eps); sum h / (1 + n).
              A pixel whose candidates all have a zero logit contributes h = 0 and still counts.

``top1`` also returns the relative distance of every gate value from the threshold and the relative gap of the two largest student
candidate probabilities: the two discrete decisions a float32 implementation could take differently."""
import numpy as np
import torch

EPS = 1e-8


def _multi_hot_pixels(tgt, spx, msk, *planes):
    """rows of every [N,C,H,W] plane at the selected pixels whose superpixel has more than one target bit, and their target rows"""
    tg = torch.from_numpy(np.asarray(tgt)).to(torch.float64)
    N, H, W = np.asarray(spx).shape
    sp = torch.from_numpy(np.asarray(spx, dtype=np.int64)).reshape(N, H * W)
    mk = torch.from_numpy(np.asarray(msk).astype(bool)).reshape(N, H * W)
    rows, ys = [[] for _ in planes], []
    for i in range(N):
        y = tg[i][sp[i][mk[i]]]
        multi = y.sum(dim=1) > 1
        ys.append(y[multi])
        for k, p in enumerate(planes):
            rows[k].append(p[i].permute(1, 2, 0).reshape(H * W, -1)[mk[i]][multi])
    return [torch.cat(r) for r in rows], torch.cat(ys)


def _leaf(z):
    return torch.from_numpy(np.asarray(z, dtype=np.float32)).to(torch.float64).requires_grad_(True)


def top1(z, zt, tgt, spx, msk, T, th, within, w=1.0):
    """(loss, n_counted, gradient of w * loss, relative gate margins [P], relative top-2 gaps [P]) in float64."""
    zs = _leaf(z)
    zteach = torch.from_numpy(np.asarray(zt, dtype=np.float32)).to(torch.float64)
    (ls, lt), y = _multi_hot_pixels(tgt, spx, msk, zs, zteach)
    p = torch.softmax(ls / T, dim=1) * y
    t = torch.softmax(lt / T, dim=1) * y
    g = t.max(dim=1)[0]
    if within:
        g = g / t.sum(dim=1)
    counted = g > th
    loss = (-torch.log(p.max(dim=1)[0][counted] + EPS)).sum() / (1 + int(counted.sum()))
    grad = torch.autograd.grad(w * loss, zs)[0].numpy() if p.shape[0] else np.zeros(np.shape(z))
    with torch.no_grad():
        margin = ((g - th).abs() / max(abs(th), 1e-300)).numpy() if th != 0 else np.full(g.shape[0], np.inf)
        top = torch.topk(p, 2, dim=1)[0]
        gap = ((top[:, 0] - top[:, 1]) / top[:, 0]).numpy()
    return float(loss), int(counted.sum()), grad, margin, gap


def ent(z, tgt, spx, msk, T, w=1.0):
    """(loss, n, gradient of w * loss) in float64."""
    zs = _leaf(z)
    (ls,), y = _multi_hot_pixels(tgt, spx, msk, zs)
    if ls.shape[0] == 0:
        return 0.0, 0, np.zeros(np.shape(z))
    member = (y > 0) & (ls != 0)
    live = member.any(dim=1)
    x = torch.where(member, ls / T, torch.full_like(ls, -float('inf')))[live]
    q = torch.softmax(x, dim=1)
    h = -(q * torch.log(q + EPS)).sum(dim=1)
    loss = h.sum() / (1 + int(ls.shape[0]))
    grad = torch.autograd.grad(w * loss, zs)[0].numpy() if bool(live.any()) else np.zeros(np.shape(z))
    return float(loss), int(ls.shape[0]), grad
