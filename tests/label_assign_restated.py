"""numpy restatement of the data-generation step (mulactseg_amd/label_assignment.py, csrc/labels.hip), for the tests.

Two forms: a vectorised one (boundary by shifted comparisons with edge replication, trim by a clipped box-OR, histograms by
``bincount``) and a literal per-id loop that follows the reference's steps (``dataloader/region_cityscapes_tensor.py:23-86``,
``region_cityscapes_dominant_all[_sample].py:24-62``: ``np.unique`` per id, the fallback to the untrimmed region, ``argmax``, the
multinomial draw)."""
import numpy as np

IGNORE = 255


def thick_boundary(spx):
    """find_boundaries(mode='thick'): some 4-neighbour differs; the edge is replicated, so the border alone is no boundary."""
    p = np.pad(spx, 1, mode='edge')
    c = p[1:-1, 1:-1]
    return (p[:-2, 1:-1] != c) | (p[2:, 1:-1] != c) | (p[1:-1, :-2] != c) | (p[1:-1, 2:] != c)


def dilate(b, k):
    """binary_dilation with a k x k square of ones, the window clipped at the edge (border_value 0)."""
    h = k // 2
    H, W = b.shape
    p = np.pad(b, h, mode='constant')
    rows = np.zeros((H + 2 * h, W), dtype=bool)
    for d in range(k):
        rows |= p[:, d:d + W]
    out = np.zeros((H, W), dtype=bool)
    for d in range(k):
        out |= rows[d:d + H]
    return out


def trimmed_map(spx, nseg, k):
    return np.where(dilate(thick_boundary(spx), k), nseg, spx)


def _check_labels(labels, C):
    bad = (labels >= C) & (labels != IGNORE)
    if np.any(bad) or np.any(labels < 0):
        raise ValueError("label values outside [0, C) and 255")


def histograms(labels, spx, nseg, C, mask=None):
    """int64 [nseg, C+1]: pixels of id p with label c (column C: 255)."""
    labels = np.asarray(labels).astype(np.int64)
    spx = np.asarray(spx).astype(np.int64)
    ok = (spx >= 0) & (spx < nseg)
    if mask is not None:
        ok &= mask
    col = np.where(labels == IGNORE, C, labels)
    return np.bincount((spx[ok] * (C + 1) + col[ok]).ravel(), minlength=nseg * (C + 1)).reshape(nseg, C + 1)


def multi_hot(labels, spx, ids, nseg, C, k=0):
    """(cls uint8 [nseg, C+1], size int64 [nseg]), vectorised."""
    _check_labels(labels, C)
    full = histograms(labels, spx, nseg, C)
    use = full
    if k:
        band = dilate(thick_boundary(np.asarray(spx)), k)
        trim = histograms(labels, spx, nseg, C, ~band)
        use = np.where(trim.sum(1, keepdims=True) > 0, trim, full)
    listed = np.zeros(nseg, dtype=bool)
    listed[np.asarray(ids, dtype=np.int64)] = True
    cls = np.where(listed[:, None], use > 0, False).astype(np.uint8)
    size = np.where(listed, use.sum(1), -1).astype(np.int64)
    return cls, size


def multi_hot_loop(labels, spx, ids, nseg, C, k=0):
    """The reference's per-id loop (region_cityscapes_tensor.py:38-84)."""
    _check_labels(labels, C)
    target = np.asarray(labels).astype(np.int64).reshape(-1)
    sp = np.asarray(spx).astype(np.int64)
    cls = np.zeros((nseg, C + 1), dtype=np.uint8)
    size = np.full(nseg, -1, dtype=np.int64)
    trim = trimmed_map(sp, nseg, k).reshape(-1) if k else None
    sp = sp.reshape(-1)
    for p in ids:
        if k:
            m = trim == p
            m = m if m.any() else sp == p
        else:
            m = sp == p
        u, c = np.unique(target[m], return_counts=True)
        isignore = IGNORE in u
        allignore = isignore and len(u) == 1
        npx = m.sum()
        if not allignore:
            uv, cv = u[u != IGNORE], c[u != IGNORE]
            lst = uv[cv.argsort()[::-1]].tolist()
        else:
            lst = []
        if isignore:
            lst.append(-1)
        cls[p, lst] = 1
        size[p] = npx
    return cls, size


def sample_generator(seed):
    import torch
    g = torch.Generator()
    g.manual_seed(int(seed))
    torch.empty((), dtype=torch.int64).random_(generator=g)       # the DataLoader iterator's base seed
    return g


def dominant(labels, spx, ids, nseg, C, generate_ignore=False, generator=None):
    """uint8 [H,W] dominant-label map, vectorised (the draw replays the reference's call order)."""
    _check_labels(labels, C)
    lab = np.asarray(labels).astype(np.int64)
    sp = np.asarray(spx).astype(np.int64)
    full = histograms(lab, sp, nseg, C)
    hi = C + 1 if generate_ignore else C
    h = full[:, :hi]
    choice = np.full(nseg, -1, dtype=np.int64)
    if generator is None:
        nonempty = h.sum(1) > 0
        best = np.argmax(h, axis=1)                           # first maximum: the smaller value
        listed = np.zeros(nseg, dtype=bool)
        listed[np.asarray(ids, dtype=np.int64)] = True
        choice = np.where(listed & nonempty, best, -1)
    else:
        import torch
        done = set()
        for p in ids:
            p = int(p)
            if p in done:
                n = int(h[p].sum())
                if n:
                    torch.multinomial(torch.Tensor(np.array([n])), 1, False, generator=generator)
                continue
            done.add(p)
            nz = np.nonzero(h[p])[0]
            if nz.size:
                choice[p] = nz[torch.multinomial(torch.Tensor(h[p][nz]), 1, False, generator=generator).item()]
    val = np.where(choice == C, IGNORE, choice)
    ok = (sp >= 0) & (sp < nseg)
    v = np.where(ok, val[np.clip(sp, 0, nseg - 1)], -1)
    paint = (v >= 0) & (generate_ignore | (lab != IGNORE))
    return np.where(paint, v, lab).astype(np.uint8)


def dominant_loop(labels, spx, ids, generate_ignore=False, generator=None):
    """The reference's per-id loop (region_cityscapes_dominant_all.py:35-53, the _sample form with ``generator``)."""
    import torch
    target = np.asarray(labels).astype(np.int64).reshape(-1).copy()
    h, w = np.asarray(labels).shape
    ignore_mask = target == IGNORE
    sp = np.asarray(spx).astype(np.int64).reshape(-1)
    for p in ids:
        m = (sp == p) if generate_ignore else ((sp == p) & ~ignore_mask)
        u, c = np.unique(target[m], return_counts=True)
        if c.size != 0:
            if generator is None:
                target[m] = u[c.argmax()]
            else:
                target[m] = u[torch.multinomial(torch.Tensor(c), num_samples=1, replacement=False, generator=generator).item()]
    if not generate_ignore:
        target[ignore_mask] = IGNORE
    return target.reshape(h, w).astype(np.uint8)


def voronoi(seed, H, W, nseg):
    """Voronoi-like superpixel map on a jittered grid (nearest of the 9 neighbouring cells), plus thin stripes and one-pixel
    regions; some ids of [0, nseg) may be absent."""
    rs = np.random.RandomState(seed)
    gy = int(np.round(np.sqrt(nseg * H / W))) or 1
    gx = max(1, nseg // gy)
    ch, cw = H / gy, W / gx
    cy = (np.arange(gy)[:, None] + rs.uniform(0.1, 0.9, (gy, gx))) * ch
    cx = (np.arange(gx)[None, :] + rs.uniform(0.1, 0.9, (gy, gx))) * cw
    perm = rs.permutation(nseg)[:gy * gx].reshape(gy, gx)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    by, bx = np.minimum((yy / ch).astype(int), gy - 1), np.minimum((xx / cw).astype(int), gx - 1)
    best = np.full((H, W), np.inf)
    out = np.zeros((H, W), dtype=np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ny, nx = np.clip(by + dy, 0, gy - 1), np.clip(bx + dx, 0, gx - 1)
            d = (yy - cy[ny, nx]) ** 2 + (xx - cx[ny, nx]) ** 2
            better = d < best
            best = np.where(better, d, best)
            out = np.where(better, perm[ny, nx], out)
    # thin and one-pixel regions
    for i in range(4):
        r = rs.randint(0, H)
        c0 = rs.randint(0, W)
        out[r, c0:c0 + 40] = rs.randint(0, nseg)
    for i in range(6):
        out[rs.randint(0, H), rs.randint(0, W)] = rs.randint(0, nseg)
    return out


def labels_for(seed, spx, C, ignore_frac=0.1):
    """Labels mostly constant per superpixel, with a second class and ignore pixels sprinkled in."""
    rs = np.random.RandomState(seed)
    base = rs.randint(0, C, int(spx.max()) + 1)
    lab = base[np.clip(spx, 0, None)].astype(np.int64)
    noise = rs.uniform(size=spx.shape)
    lab = np.where(noise < 0.08, rs.randint(0, C, spx.shape), lab)
    lab = np.where(noise > 1 - ignore_frac, IGNORE, lab)
    return lab.astype(np.uint8)
