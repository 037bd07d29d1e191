"""numpy restatement of csrc/render.hip, written from the semantics of INTEGRATION.md section 5 (the reference's ``--save_vis`` lines
and ``eval_naive_vis``): no skimage, no scipy.

``mark_boundaries(colours, s) * 255`` cast to uint8, skimage defaults (mode 'outer', background 0, colour (1, 1, 0)):
  thick = max of s over the 3 x 3 cross != min over the cross
  bg    = s == 0;  inv = s with bg set to the dtype's maximum
  mark  = thick & (bg | (max of s over the 3 x 3 square != min of inv over the square))
with the neighbour outside the picture = the edge pixel.  Marked pixels are (255, 255, 0); every other byte c becomes
uint8(float64(c) * (1.0 / 255) * 255)."""
import numpy as np

INT64_MAX = np.iinfo(np.int64).max


def round_trip(c):
    """The float64 round trip of ``img_as_float`` (``* (1.0 / 255)``) and the reference's ``* 255`` / ``astype('uint8')``."""
    return (np.asarray(c, dtype=np.uint8).astype(np.float64) * (1.0 / 255) * 255).astype(np.uint8)


def _windows(s):
    """The 3 x 3 neighbourhoods of a 2-D map, edges replicated: [9, H, W], index 3 r + c for offset (r - 1, c - 1)."""
    H, W = s.shape
    p = np.pad(s, 1, mode='edge')
    return np.stack([p[r:r + H, c:c + W] for r in range(3) for c in range(3)])


def outer_boundaries(s):
    """Boolean [H,W]: the pixels ``find_boundaries(s, mode='outer', background=0)`` marks."""
    s = np.asarray(s, dtype=np.int64)
    w = _windows(s)
    cross = w[[1, 3, 4, 5, 7]]
    thick = cross.max(0) != cross.min(0)
    bg = s == 0
    inv = np.where(w == 0, INT64_MAX, w)
    adjacent = (w.max(0) != inv.min(0)) & ~bg
    return thick & (bg | adjacent)


def colours(labels, palette, fill):
    """``palette[masked_fill(labels, labels == 255, fill)]`` [.., 3] uint8; a label outside the palette raises."""
    lab = np.asarray(labels).astype(np.int64)
    lab = np.where(lab == 255, fill, lab)
    pal = np.asarray(palette, dtype=np.uint8)
    if lab.min() < 0 or lab.max() >= len(pal):
        raise IndexError("label outside the palette")
    return pal[lab]


def render_labels(labels, palette, fill, superpixels=None):
    """[N,H,W,3] uint8: the plain colours, or with ``superpixels`` the ``mark_boundaries`` image."""
    rgb = colours(labels, palette, fill)
    if superpixels is None:
        return rgb
    out = round_trip(rgb)
    for i in range(out.shape[0]):
        out[i][outer_boundaries(superpixels[i])] = (255, 255, 0)
    return out


def first_argmax(z):
    """``torch.max(z, 1)[1]`` of [N,C,H,W] float32: the first maximum in channel order, the first NaN where there is one."""
    z = np.asarray(z)
    nan = np.isnan(z)
    idx = np.argmax(np.where(nan, -np.inf, z), axis=1)
    has_nan = nan.any(axis=1)
    return np.where(has_nan, np.argmax(nan, axis=1), idx)


def render_pred(z_full, palette):
    """``palette[max(z_full[:, :-1], 1)[1]]`` of full-resolution logits [N,CH,H,W]."""
    return np.asarray(palette, dtype=np.uint8)[first_argmax(np.asarray(z_full)[:, :-1])]
