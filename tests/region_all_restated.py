"""numpy restatement of the per-region entries of ``dataloader/region_cityscapes_all.py`` (the reference's loop over the listed ids:
one ``np.unique`` of the labels under each id), for pictures given as arrays."""
import numpy as np


def superpixel_info(target, superpixel, ids, ignore=255):
    """{id: {'cls', 'cpx', 'npx', 'isignore', 'allignore'}} of label map ``target`` [H,W] and id map ``superpixel`` [H,W]."""
    t = np.asarray(target).reshape(-1)
    s = np.asarray(superpixel).reshape(-1)
    info = {}
    for p in ids:
        sel = s == p
        values, counts = np.unique(t[sel], return_counts=True)
        isignore = bool(ignore in values)
        allignore = bool(np.all(values != ignore))         # (True when NO pixel is ignore: the reference's flag as it is)
        cls, cpx = [], []
        if not allignore:
            keep = values != ignore
            kv, kc = values[keep], counts[keep]
            order = kc.argsort()[::-1]
            cls, cpx = [int(v) for v in kv[order]], [int(v) for v in kc[order]]
        info[p] = {'cls': cls, 'cpx': cpx, 'npx': int(sel.sum()), 'isignore': isignore, 'allignore': allignore}
    return info
