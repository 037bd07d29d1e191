"""Records tests/golden/g16_simw_plbl.npz by EXECUTING the reference's similarity-weighted online pseudo-label losses on the CPU (not
collected; the only file of the simw-plbl tests that reads the reference tree).  Run:  ``python tests/record_simw_plbl_golden.py``.

  LocalsimWProtoCE             ``trainer/active_onlinesimwplbl_multi_predignore.py:15-148``  -> labels, simw (the similarity weights),
                               simw_loss, simw_gradq; with ``--th_wplbl``: simw_th_loss, simw_th_gradq
  JointLocalProtoWeightingCE   ``trainer/active_pwce_multi_predignore.py:17-155`` at tau = 0.1 and 0.01  -> pwce_loss [2],
                               pwce_gradq [2,...], softw [2, valid pixels, C] (its soft weights, 0 off the candidates), pwce_count

Inputs are recorded by seed (``online_plbl_restated.inputs``, the g15 case); the reference sees their ``F.interpolate(bilinear)`` to the
picture size.  The reference's gradients are with respect to the full-resolution logits; four of them ([2,20,40,44] float32, dense on
the selected pixels) would take the file past the size this golden holds itself to, so each is stored pushed through the transpose of
the bilinear upsampling (``*_gradq`` [N,C,hq,wq], the push done here in float64) -- the form the tests compare in.

The stand-in ``torch_scatter`` has no ``scatter_softmax`` / ``scatter_log_softmax``; they are set on it here, written from
torch_scatter's documented semantics (a softmax within the groups of ``index`` along ``dim``), and the softmax records what it
returns: that is how the reference's soft weights, local to its ``forward``, are read.

Also recorded: ``sim_err_ref`` and ``softw_err_ref`` [2] (the largest |float32 - float64| of the reference's own similarities and soft
weights on these inputs, the float64 side from tests/simw_plbl_restated.py), ``simw_abs`` / ``simw_th_abs`` (the mean |weight * CE|
over the counted pixels: the scale of a sum whose terms may cancel).  The conditions the tests rely on are asserted here; if one
fails, change the seed, not the bound."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from online_plbl_restated import SEED, N, C, CH, H, W, HQ, WQ, S, T, inputs, upsample  # noqa: E402

TAUS = (0.1, 0.01)
TH_SIM = 0.25           # --th_wplbl on a similarity: between the typical product of two different pixels and a prototype's own
NEAR = 1e-5
MAX_BYTES = 192 * 1024
CAPTURED = []


def _gather_groups(per_group, index, dim):
    return per_group.gather(dim, index)


def scatter_softmax(src, index, dim=-1, dim_size=None):
    """softmax of ``src`` within the groups ``index`` names along ``dim`` (``index`` 1-D along ``dim``, broadcast over the rest)"""
    import torch_scatter
    dim = dim % src.dim()
    shape = [1] * src.dim()
    shape[dim] = -1
    idx = index.view(shape).expand_as(src)
    groups = int(index.max()) + 1 if dim_size is None else dim_size
    top = torch_scatter.scatter_max(src, idx, dim=dim, dim_size=groups)[0]
    e = (src - _gather_groups(top, idx, dim)).exp()
    out = e / _gather_groups(torch_scatter.scatter_sum(e, idx, dim=dim, dim_size=groups), idx, dim)
    CAPTURED.append((index.clone(), out.detach().clone()))
    return out


def scatter_log_softmax(src, index, dim=-1, dim_size=None):
    import torch_scatter
    dim = dim % src.dim()
    shape = [1] * src.dim()
    shape[dim] = -1
    idx = index.view(shape).expand_as(src)
    groups = int(index.max()) + 1 if dim_size is None else dim_size
    top = torch_scatter.scatter_max(src, idx, dim=dim, dim_size=groups)[0]
    z = src - _gather_groups(top, idx, dim)
    return z - _gather_groups(torch_scatter.scatter_sum(z.exp(), idx, dim=dim, dim_size=groups), idx, dim).log()


def main():
    import install as refshim
    import online_plbl_restated as R
    import simw_plbl_restated as Q
    refshim.install()
    import torch_scatter
    torch_scatter.scatter_softmax, torch_scatter.scatter_log_softmax = scatter_softmax, scatter_log_softmax
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules['tqdm'] = types.ModuleType('tqdm')
            sys.modules['tqdm'].tqdm = lambda it, **k: it
    from trainer.active_onlinesimwplbl_multi_predignore import LocalsimWProtoCE
    from trainer.active_onlineplbl_multi_predignore import LocalProtoCE
    from trainer.active_pwce_multi_predignore import JointLocalProtoWeightingCE

    zq_p, featq, zq, tgt, spx, msk = inputs()
    logits_p, feats, logits = upsample(zq_p, (H, W)), upsample(featq, (H, W)), upsample(zq, (H, W))
    tt, ts, tm = torch.from_numpy(tgt), torch.from_numpy(spx), torch.from_numpy(msk)

    def args(**kw):
        return types.SimpleNamespace(nseg=S, weight_wo_proto=False, th_wplbl=kw.get('th'), ce_temp=T, simw_temp=kw.get('tau', 0.1))

    def pushed(g):
        """the full-resolution gradient through the transpose of the upsampling, in float64"""
        zt = torch.from_numpy(zq).double().requires_grad_(True)
        (q,) = torch.autograd.grad(upsample(zt, (H, W)), zt, grad_outputs=g.double())
        return q.float().numpy()

    def run(cls, **kw):
        crit = cls(args=args(**kw), num_superpixel=S, temperature=T)
        z = logits.clone().requires_grad_(True)
        loss = crit(logits_p, feats, z, tt, ts, tm)
        (g,) = torch.autograd.grad(loss, z)
        return np.float32(float(loss.detach())), pushed(g)

    out = dict(seed=SEED, N=N, C=C, Ch=CH, H=H, W=W, hq=HQ, wq=WQ, S=S, temp=T, th=TH_SIM, taus=np.asarray(TAUS))
    out['simw_loss'], out['simw_gradq'] = run(LocalsimWProtoCE)
    out['simw_th_loss'], out['simw_th_gradq'] = run(LocalsimWProtoCE, th=TH_SIM)
    with torch.no_grad():
        w, lab = LocalsimWProtoCE(args=args(), num_superpixel=S, temperature=T).generate_plbl(logits_p, feats, tt, ts, tm)
        lab_plain = LocalProtoCE(args=args(), num_superpixel=S, temperature=T).generate_plbl(logits_p, feats, tt, ts, tm)
    assert torch.equal(lab, lab_plain), "the similarity weight changed a label"
    valid = (lab != 255).numpy()
    n_valid = int(valid.sum())
    out['labels'], out['simw'] = lab.numpy().astype(np.uint8), w.numpy()[valid]
    n_neg = int((out['simw'] < 0).sum())
    assert n_neg >= 1, "no similarity weight is negative: the signed sum would not be exercised"
    ce = F.cross_entropy(logits.double() / T, lab.long(), ignore_index=255, reduction='none')
    assert float(ce[lab != 255].min()) >= 1e-6, "a labelled pixel has ce < 1e-6: the non-zero count would be ambiguous"
    term = (w.double() * ce)[lab != 255]
    assert bool((term != 0).all())
    out['simw_abs'] = np.float64(term.abs().mean())
    gate = (TH_SIM < w)[lab != 255]
    assert 0.05 * n_valid <= int(gate.sum()) <= 0.95 * n_valid, "the threshold passes %d of %d" % (int(gate.sum()), n_valid)
    out['simw_th_abs'] = np.float64(ce[lab != 255][gate].mean())
    out['simw_th_count'] = np.int64(gate.sum())

    # the float64 side
    d = Q.similarities(logits_p, feats, tgt, spx, msk, T, near=NEAR)
    assert np.array_equal(d['valid'], valid)
    loose = d['loose'][valid]
    assert 200 * int(loose.sum()) <= n_valid, "%d of %d valid pixels lie in superpixels with an undecided prototype" % (loose.sum(), n_valid)
    err = 0.0
    for i in range(N):
        vf = feats[i].permute(1, 2, 0).reshape(-1, CH)[tm[i].reshape(-1)]
        err = max(err, float((torch.mm(vf, vf.T).double() - torch.mm(vf.double(), vf.double().T)).abs().max()))
    out['sim_err_ref'] = np.float64(err)
    lab64, w64 = Q.sim_weight(d['sims'])
    gap = R.generate(logits_p, feats, tgt, spx, msk, T)[2].numpy()
    close = int((gap[valid] <= 8 * err).sum())
    assert 200 * close < n_valid, "%d of %d valid pixels lie within 8 * sim_err_ref of a tie" % (close, n_valid)
    out['gap64'] = gap[valid].astype(np.float32)

    # JointLocalProtoWeightingCE: losses, gradients and the soft weights its forward builds
    softw, losses, grads, soft_err = [], [], [], []
    for tau in TAUS:
        del CAPTURED[:]
        loss, g = run(JointLocalProtoWeightingCE, tau=tau)
        losses.append(loss)
        grads.append(g)
        live = [i for i in range(N) if d['valid'][i].any()]
        assert len(CAPTURED) == len(live)
        full = np.zeros((N, C, H * W), dtype=np.float32)
        for (index, prob), i in zip(CAPTURED, live):
            vpix = np.nonzero(d['valid'][i].reshape(-1))[0]                         # columns: the valid pixels in raster order
            vspx = np.unique(spx[i].reshape(-1)[vpix])                              # groups: the valid superpixels, ascending
            rows = [(int(s), int(c)) for s in vspx for c in np.nonzero(tgt[i, s])[0]]       # rows: (superpixel, class) ascending
            assert prob.shape == (len(rows), len(vpix)) and np.array_equal(index.numpy(), [np.searchsorted(vspx, s) for s, _ in rows])
            ids = spx[i].reshape(-1)[vpix]
            for r, (s, c) in enumerate(rows):
                sel = ids == s
                full[i, c, vpix[sel]] = prob[r].numpy()[sel]
        full = full.reshape(N, C, H, W)
        sw64 = Q.soft_weights(d['sims'], tau)
        assert np.array_equal(full != 0, ~np.isnan(sw64)) or tau < 0.05              # (at a small tau a weight may underflow to 0)
        keep = ~np.isnan(sw64) & ~d['loose'][:, None]
        soft_err.append(float(np.abs(full - np.nan_to_num(sw64))[keep].max()))
        softw.append(np.moveaxis(full, 1, -1)[valid])                                # [valid pixels, C]
        count = sum(int(msk[i].sum()) for i in live)
    out['pwce_loss'], out['pwce_gradq'], out['softw'] = np.asarray(losses), np.stack(grads), np.stack(softw)
    out['softw_err_ref'], out['pwce_count'] = np.asarray(soft_err), np.int64(count)

    path = os.path.join(ROOT, "tests", "golden", "g16_simw_plbl.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print({k: (v if np.ndim(v) == 0 else np.shape(v)) for k, v in out.items()})
    print("valid pixels %d, negative weights %d, gated in %d, near ties %d, loose %d, float64 label agreement %.6f, counted %d, bytes %d"
          % (n_valid, n_neg, int(gate.sum()), close, int(loose.sum()), float((lab64[valid] == lab.numpy()[valid]).mean()), count, size))
    assert size <= MAX_BYTES, "the golden grew to %d bytes" % size


if __name__ == "__main__":
    main()
