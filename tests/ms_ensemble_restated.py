"""numpy float32 restatement of ``mas_ms_ensemble`` (mulactseg_amd/csrc/ms_ensemble.hip): every operation rounded separately, in the
order the header comment of the kernel prescribes -- the yardstick the GPU tests compare the kernel with bit for bit.

Per source k: stage 1 = the network's x4 bilinear upsampling (quarter -> (Hs, Ws)), the flip, stage 2 = F.interpolate(bilinear,
align_corners=False) to (H, W); the sources summed in list order and divided by n; the features divided by
max(sqrt(sum over channels of m*m), 1e-12)."""
import numpy as np

F32 = np.float32


def quarter_size(n):
    """The side the network emits at quarter resolution (stride-2 stem convolution, stride-2 max-pool)."""
    return ((int(n) - 1) // 2) // 2 + 1


def taps(n_in, n_out):
    """(i0, i1, l0, l1) per output index: s = max(0, scale*(o+0.5)-0.5) with scale = (float)n_in / (float)n_out, i0 = (int)s,
    i1 = i0 + (i0 < n_in-1), l1 = s - i0, l0 = 1 - l1."""
    scale = F32(n_in) / F32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    s = scale * (o + F32(0.5)) - F32(0.5)
    s = np.maximum(s, F32(0.0))
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(np.float32)
    l0 = F32(1.0) - l1
    return i0, i1, l0, l1


def resize(x, Ho, Wo):
    """x f32 [Ch,Hi,Wi] -> [Ch,Ho,Wo]: y = l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11)."""
    x = np.asarray(x, dtype=np.float32)
    yi0, yi1, yl0, yl1 = taps(x.shape[1], Ho)
    xi0, xi1, xl0, xl1 = taps(x.shape[2], Wo)
    r0, r1 = x[:, yi0, :], x[:, yi1, :]
    top = xl0 * r0[:, :, xi0] + xl1 * r0[:, :, xi1]
    bot = xl0 * r1[:, :, xi0] + xl1 * r1[:, :, xi1]
    return (yl0[:, None] * top + yl1[:, None] * bot).astype(np.float32)


def stage1(q, Hs, Ws):
    """The x4 upsampling of feat_forward: quarter [Ch,hq,wq] -> [Ch,Hs,Ws]."""
    return resize(q, Hs, Ws)


def source(q, Hs, Ws, flip, H, W):
    """One source at the original size: stage 1, the flip, stage 2."""
    s = stage1(q, Hs, Ws)
    if flip:
        s = np.ascontiguousarray(s[:, :, ::-1])
    return resize(s, H, W)


def mean(qs, sizes, flips, H, W):
    acc = None
    for q, (Hs, Ws), fl in zip(qs, sizes, flips):
        v = source(q, Hs, Ws, fl, H, W)
        acc = v if acc is None else (acc + v).astype(np.float32)
    return (acc / F32(len(qs))).astype(np.float32)


def normalise(m):
    """m / max(sqrt(sum_c m_c * m_c), 1e-12), the squares summed in channel order."""
    ss = np.zeros(m.shape[1:], dtype=np.float32)
    for c in range(m.shape[0]):
        ss = (ss + m[c] * m[c]).astype(np.float32)
    d = np.maximum(np.sqrt(ss), F32(1e-12))
    return (m / d).astype(np.float32)


def ms_ensemble(feats_q, logits_q, sizes, flips, out_size):
    """feats_q / logits_q: lists of f32 [Ch,hq,wq] / [C,hq,wq] -> (features [Ch,H,W], logits [C,H,W])."""
    H, W = out_size
    return normalise(mean(feats_q, sizes, flips, H, W)), mean(logits_q, sizes, flips, H, W)


def tta_sizes(H, W, factors=(0.5, 0.75, 1.0, 1.25, 1.5)):
    """(sizes, flips) of TestTimeAugmentation on an H x W picture, in its order."""
    sizes = [(int(f * H), int(f * W)) for _ in (False, True) for f in factors]
    flips = [fl for fl in (False, True) for _ in factors]
    return sizes, flips
