"""numpy restatement of the two stage-2 ablation kernels (csrc/naive_plbl.hip, k_spx_max_onehot of csrc/labels.hip), written from
their normative comments, and the reference's torch lines they replace."""
import numpy as np

F32 = np.float32


def taps(n_in, n_out):
    """(i0, i1, l0, l1) per output index: upsample.hip's make_tap in float32, scale = (float)n_in / (float)n_out."""
    scale = F32(n_in) / F32(n_out)
    o = np.arange(n_out, dtype=F32)
    s = (scale * (o + F32(0.5))).astype(F32) - F32(0.5)
    s = np.maximum(s, F32(0)).astype(F32)
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def upsample(zq, H, W):
    """[N,C,h,w] f32 -> [N,C,H,W]: y = l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11), each operation rounded to float32; the
    identity geometry returns the logits themselves."""
    zq = np.asarray(zq, dtype=F32)
    h, w = zq.shape[2:]
    if (h, w) == (H, W):
        return zq.copy()
    yi0, yi1, yl0, yl1 = taps(h, H)
    xi0, xi1, xl0, xl1 = taps(w, W)
    r0, r1 = zq[:, :, yi0, :], zq[:, :, yi1, :]
    a = (xl0 * r0[..., xi0]).astype(F32) + (xl1 * r0[..., xi1]).astype(F32)
    b = (xl0 * r1[..., xi0]).astype(F32) + (xl1 * r1[..., xi1]).astype(F32)
    return ((yl0[:, None] * a).astype(F32) + (yl1[:, None] * b).astype(F32)).astype(F32)


def first_argmax(z):
    """Arg-max over axis 1, the first maximum; a NaN wins where it first appears (torch.max / np.argmax agree on both)."""
    return np.argmax(z, axis=1)


def pmax(z):
    """1 / sum_c exp(z_c - z_max), channel order, in float32 (the kernel's expression; its expf is not numpy's exp)."""
    m = np.max(z, axis=1)
    nan = np.isnan(z).any(axis=1)
    s = np.zeros(m.shape, dtype=F32)
    for c in range(z.shape[1]):
        s = (s + np.exp((z[:, c] - m).astype(F32))).astype(F32)
    p = (F32(1) / s).astype(F32)
    p[nan] = np.nan
    return p


def naive_labels(zq, H, W, mask, th):
    """int64 [N,H,W]: 255 where the pixel is not kept; th <= 0: kept where mask, th > 0: kept where pmax > th."""
    z = upsample(zq, H, W)
    lab = first_argmax(z).astype(np.int64)
    keep = pmax(z) > th if th > 0 else np.asarray(mask, dtype=bool)
    return np.where(keep, lab, 255)


def reference_lines(zq, H, W, spmask, th):
    """The reference (eval_save_naiveplbl.py:52-56) in torch on the CPU, with feat_forward's F.interpolate."""
    import torch
    import torch.nn.functional as F
    z = torch.from_numpy(np.asarray(zq, dtype=F32))
    if tuple(z.shape[2:]) != (H, W):
        z = F.interpolate(z, size=(H, W), mode='bilinear', align_corners=False)
    spmask = torch.from_numpy(np.asarray(spmask, dtype=bool))
    if th > 0:
        spmask = torch.softmax(z, dim=1).max(dim=1)[0] > th
    lab = z.max(dim=1)[1]
    return torch.masked_fill(lab, torch.logical_not(spmask), 255).numpy()


def spx_max_onehot(target, spx, nseg, C):
    """(rows u8 [nseg, C], mask bool [H,W]): per id in [0, nseg) the largest target value (255 -> C - 1), one-hot; an id with no pixel
    gets the row of 0; mask = target != 255."""
    t = np.asarray(target).reshape(-1).astype(np.int64)
    s = np.asarray(spx).reshape(-1).astype(np.int64)
    ok = (s >= 0) & (s < nseg)
    m = np.full(nseg, -1, dtype=np.int64)
    np.maximum.at(m, s[ok], t[ok])
    v = np.where(m < 0, 0, np.where(m == 255, C - 1, m))
    rows = (np.arange(C)[None, :] == v[:, None]).astype(np.uint8)
    return rows, np.asarray(target) != 255


def spx_max_onehot_loop(target, spx, C):
    """The reference's lines (``scatter_max`` over ``max(id) + 1`` segments, 255 -> 19, ``one_hot``) as a per-id loop."""
    t = np.asarray(target).reshape(-1).astype(np.int64)
    s = np.asarray(spx).reshape(-1).astype(np.int64)
    n = int(s.max()) + 1
    rows = np.zeros((n, C), dtype=np.uint8)
    for p in range(n):
        sel = t[s == p]
        m = int(sel.max()) if sel.size else 0          # torch_scatter fills an empty segment with 0
        rows[p, C - 1 if m == 255 else m] = 1
    return rows
