"""Tensor-level wrappers over the C ABI: contiguous ROCm tensors in, ROCm tensors out.

Every function launches on the current torch stream and never synchronises with the host.
These are the only callers of ``_lib``; the plugin-level code (``active_selection``, ``utils.loss``)
is written against this module.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

_ID_CODES = {torch.int64: _lib.ID_I64, torch.int32: _lib.ID_I32, torch.uint16: _lib.ID_U16,
             torch.int16: _lib.ID_U16}


def inv_temperature(T):
    """invT as the ABI defines it: float32(1 / float32(T))."""
    return float(np.float32(1.0) / np.float32(T))


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need(t, name, dtype=None):
    if not t.is_cuda:
        raise _lib.MulActSegHipError("%s must live on the GPU (no CPU path exists)" % name)
    if dtype is not None and t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _opt(t):
    return t.data_ptr() if t is not None else None


def _stream_key(dev):
    return (dev, torch.cuda.current_stream(dev).cuda_stream)


def _stream_scratch(table, dev, alloc, n=0):
    """``table``'s entry for the current stream of ``dev``, from ``alloc()`` when there is none yet or it holds fewer than ``n``
    elements.  The launches of one stream run in order, so they can share scratch memory; two streams never do."""
    key = _stream_key(dev)
    ent = table.get(key)
    if ent is None or (n and ent.numel() < n):
        ent = table[key] = alloc()
    return ent


def _id_code(spx):
    try:
        return _ID_CODES[spx.dtype]
    except KeyError:
        raise TypeError("superpixel ids must be int64, int32 or uint16, got %s" % spx.dtype)


def class_prob_sum(z, invT, out=None):
    """K2: per-image fixed-point class-probability sums ``[B,C]`` (int64 holding uint64 bits).
    Reference: my_bvsb_predclsbal_pwr_banignore.py:41-42."""
    _need(z, "z", torch.float32)
    B, C, H, W = z.shape
    if out is None:
        out = torch.zeros((B, C), dtype=torch.int64, device=z.device)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().mas_class_prob_sum(z.data_ptr(), B, C, H, W, invT, out.data_ptr(), _stream(z)),
                   "mas_class_prob_sum")
    return out


def bvsb_region_accum(z, spx, cls_w, S, invT, score_sum=None, hist=None):
    """K1+K3: fixed-point region sums ``[B,S]`` (int64 bits of uint64) and arg-max-class histogram
    ``[B,S,C]`` (int32 bits of uint32).  Reference: my_bvsb.py:19-27, ..._pwr_banignore.py:57-69."""
    _need(z, "z", torch.float32)
    _need(spx, "spx")
    B, C, H, W = z.shape
    if tuple(spx.shape) != (B, H, W):
        raise ValueError("spx shape %s does not match logits %s" % (tuple(spx.shape), tuple(z.shape)))
    if cls_w is not None:
        _need(cls_w, "cls_w", torch.float32)
        if cls_w.numel() != C:
            raise ValueError("cls_w must have C=%d entries" % C)
    if score_sum is None:
        score_sum = torch.zeros((B, S), dtype=torch.int64, device=z.device)
    if hist is None:
        hist = torch.zeros((B, S, C), dtype=torch.int32, device=z.device)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().mas_bvsb_region_accum(
            z.data_ptr(), spx.data_ptr(), _id_code(spx), cls_w.data_ptr() if cls_w is not None else None,
            B, C, H, W, S, invT, score_sum.data_ptr(), hist.data_ptr(), _stream(z)), "mas_bvsb_region_accum")
    return score_sum, hist


def region_finalize(score_sum, hist, ban_class=-1, want_hist_i64=False):
    """K3 tail + ban: returns (score f32, dominant i32, count i32, hist_i64 or None), shaped like
    ``score_sum``.  Reference: ..._pwr_banignore.py:79-84."""
    _need(score_sum, "score_sum", torch.int64)
    _need(hist, "hist", torch.int32)
    C = hist.shape[-1]
    n = score_sum.numel()
    dev = score_sum.device
    score = torch.empty(score_sum.shape, dtype=torch.float32, device=dev)
    dom = torch.empty(score_sum.shape, dtype=torch.int32, device=dev)
    cnt = torch.empty(score_sum.shape, dtype=torch.int32, device=dev)
    h64 = torch.empty(hist.shape, dtype=torch.int64, device=dev) if want_hist_i64 else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_region_finalize(
            score_sum.data_ptr(), hist.data_ptr(), n, C, ban_class, score.data_ptr(), dom.data_ptr(),
            cnt.data_ptr(), h64.data_ptr() if h64 is not None else None, _stream(score_sum)),
            "mas_region_finalize")
    return score, dom, cnt, h64


# ------------------------------------------------------------------------------------------------
# stage-1 partial-label losses
# ------------------------------------------------------------------------------------------------
def target_bits(targets, cols_used=None):
    """u8 multi-hot rows [..., cols] -> int32 bit masks [...] over the first ``cols_used`` columns."""
    _need(targets, "targets", torch.uint8)
    cols = targets.shape[-1]
    cols_used = cols if cols_used is None else cols_used
    bits = torch.empty(targets.shape[:-1], dtype=torch.int32, device=targets.device)
    with torch.cuda.device(targets.device):
        _lib.check(_lib.load().mas_target_bits(targets.data_ptr(), bits.numel(), cols, cols_used, bits.data_ptr(),
                                               _stream(targets)), "mas_target_bits")
    return bits


def _mask_u8(mask):
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    return _need(mask, "spmasks", torch.uint8)


def _loss_shapes(z, zt, size, spx, mask, bits, grad_out=None, host=False, bits_dtype=torch.int32):
    """The tensor / shape check of every loss family and of the host references: ``z`` [N,C,H,W] (``size`` None) or [N,C,h,w] to be
    upsampled to ``size`` = (H, W); ``zt`` (optional) the teacher's logits, shaped as ``z``; ``bits`` int32 [N,S] (the fused forward alone asks for
    ``bits_dtype`` u8: the target rows [N,S,cols] it forms them from); ``grad_out`` (optional) the backward's upstream gradients.  Returns (mask
    as u8, N, C, H, W, S, (h, w)) with (h, w) = (0, 0) at full resolution, as the entry points that take both resolutions want it."""
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    for t, name, dt in ((z, "inputs", torch.float32), (zt, "plbl_inputs", torch.float32), (spx, "superpixels", None),
                        (mask, "spmasks", torch.uint8), (bits, "bits", bits_dtype),
                        (grad_out, "grad_out", torch.float32)):
        if t is None:
            continue
        if host:
            if t.is_cuda or not t.is_contiguous():
                raise ValueError("%s must be a contiguous host tensor" % name)
            if dt is not None and t.dtype != dt:
                raise TypeError("%s must be %s, got %s" % (name, dt, t.dtype))
        else:
            _need(t, name, dt)
    if zt is not None and (zt.shape != z.shape or zt.device != z.device):
        raise ValueError("teacher logits %s do not match the student's %s" % (tuple(zt.shape), tuple(z.shape)))
    N, C, h, w = z.shape
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    if tuple(spx.shape) != (N, H, W) or tuple(mask.shape) != (N, H, W) or bits.shape[0] != N:
        raise ValueError("shape mismatch between inputs %s%s, superpixels %s, spmasks %s, targets %s"
                         % (tuple(z.shape), "" if size is None else " at size %s" % ((H, W),), tuple(spx.shape), tuple(mask.shape),
                            tuple(bits.shape)))
    return mask, N, C, H, W, bits.shape[1], (0, 0) if size is None else (h, w)


def _loss_buffers(N, S, C, flags, dev, words=_lib.ACC_WORDS, wgroup=False):
    """(acc i64 [words], gmax i64 [N,S,C], tmax int32 [N,S,C]) as views of ONE zero-filled allocation (one memset): the arg-pixel table
    only with LOSS_GROUP, the teacher's table only for the wgroup family; None for what is not there."""
    n = N * S * C if flags & _lib.LOSS_GROUP else 0
    buf = torch.zeros(words + n + ((n + 1) // 2 if wgroup else 0), dtype=torch.int64, device=dev)
    gmax = buf[words:words + n].view(N, S, C) if n else None
    tmax = buf[words + n:].view(torch.int32)[:n].view(N, S, C) if wgroup else None
    return buf[:words], gmax, tmax


def _loss_fwd(z, acc, gmax, n_losses, reduce_acc, entry, head, values_entry, values_head, finalizes=False):
    """The forward body every family shares.  ``entry(*head, stream)`` is the scan, followed by the group finalize when there is a
    table, ``reduce_acc(acc)`` (data parallel: between the sums and the division), and ``values_entry(acc, *values_head, losses,
    stream)``.  ``finalizes``: the entry finalizes itself, ``entry(*head, losses, stream)``, and leaves the values too unless
    ``reduce_acc`` has to run first.  Returns losses f32 [n_losses]."""
    losses = torch.empty(n_losses, dtype=torch.float32, device=z.device)
    lib = _lib.load()
    with torch.cuda.device(z.device):
        st = _stream(z)
        own = (None if reduce_acc is not None else losses.data_ptr(),) if finalizes else ()
        _lib.check(getattr(lib, entry)(*head, *own, st), entry)
        if gmax is not None and not finalizes:
            _lib.check(lib.mas_group_finalize(gmax.data_ptr(), gmax.numel(), acc.data_ptr(), st), "mas_group_finalize")
        if reduce_acc is not None:
            reduce_acc(acc)
        if reduce_acc is not None or not finalizes:
            _lib.check(getattr(lib, values_entry)(acc.data_ptr(), *values_head, losses.data_ptr(), st), values_entry)
    return losses


def _loss_bwd(z, size, acc, n_scale, want_fix, scales_entry, scales_head, entry, head, dims, both=True):
    """The backward body every family shares: ``scales_entry(acc, *scales_head, scale, stream)``, the scan ``entry(*head, scale, *dims,
    dz, fix, stream)`` (``both`` False: the plain family's entries take dz or fix alone) and, at low resolution (``size`` given),
    the pass that rounds the int64 fixed-point sums ``fix`` to f32.  Returns dz, or (dz, fix)."""
    dev = z.device
    scale = torch.empty(n_scale, dtype=torch.float32, device=dev)
    fix = None if size is None else torch.zeros(z.shape, dtype=torch.int64, device=dev)
    dz = torch.empty_like(z)
    out = (dz.data_ptr(), _opt(fix)) if both else ((dz if fix is None else fix).data_ptr(),)
    lib = _lib.load()
    with torch.cuda.device(dev):
        st = _stream(z)
        _lib.check(getattr(lib, scales_entry)(acc.data_ptr(), *scales_head, scale.data_ptr(), st), scales_entry)
        _lib.check(getattr(lib, entry)(*head, scale.data_ptr(), *dims, *out, st), entry)
        if fix is not None:
            _lib.check(lib.mas_fix_to_float(fix.data_ptr(), fix.numel(), _lib.GRAD_FRAC, dz.data_ptr(), st), "mas_fix_to_float")
    return (dz, fix) if want_fix else dz


def _values_call(flags, weights):
    """The values entry of the plain family and its head: three losses, or four with the weighted objective."""
    if weights is None:
        return "mas_loss_values", (flags,)
    return "mas_loss_values_weighted", (flags, _need(weights, "weights", torch.float32).data_ptr())


def _partial_loss_fwd(z, size, spx, mask, bits, invT, flags, reduce_acc, weights):
    """The step-by-step forward on ``z`` [N,C,H,W] (``size`` None) or on the bilinear upsampling of ``z`` [N,C,h,w] to ``size`` =
    (H, W), which is never materialised: scan, group finalize, ``reduce_acc``, loss values."""
    mask, N, C, H, W, S, hw = _loss_shapes(z, None, size, spx, mask, bits)
    acc, gmax, _ = _loss_buffers(N, S, C, flags, z.device)
    head = (z.data_ptr(), *(() if size is None else hw), spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(), N, C, H, W, S, invT,
            flags, _opt(gmax), acc.data_ptr())
    values_entry, values_head = _values_call(flags, weights)
    losses = _loss_fwd(z, acc, gmax, n_losses=3 if weights is None else 4, reduce_acc=reduce_acc,
                       entry="mas_partial_loss_fwd" if size is None else "mas_partial_loss_fwd_lowres", head=head,
                       values_entry=values_entry, values_head=values_head)
    return losses, acc, gmax


def _partial_loss_bwd(z, size, spx, mask, bits, gmax, acc, grad_out, invT, flags, want_fix, weights):
    """The step-by-step backward of ``_partial_loss_fwd``: the gradient with respect to ``z``.  At low resolution (``size`` given) it
    is summed in int64 fixed point and rounded to f32 by a pass of its own."""
    mask, N, C, H, W, S, hw = _loss_shapes(z, None, size, spx, mask, bits, grad_out)
    # with weights, grad_out is dL/d(total) [1]; the chain rule through the weighted sum happens in the kernel
    scales_entry, scales_head = (("mas_loss_scales", (grad_out.data_ptr(), flags)) if weights is None
                                 else ("mas_loss_scales_weighted", (grad_out.data_ptr(), weights.data_ptr(), flags)))
    head = (z.data_ptr(), *(() if size is None else hw), spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(), _opt(gmax))
    return _loss_bwd(z, size, acc, n_scale=3, want_fix=want_fix, scales_entry=scales_entry, scales_head=scales_head,
                     entry="mas_partial_loss_bwd" if size is None else "mas_partial_loss_bwd_lowres", head=head,
                     dims=(N, C, H, W, S, invT, flags), both=False)


def partial_loss_fwd(z, spx, mask, bits, invT, flags, reduce_acc=None):
    """Forward scan + group finalize + loss values.  Returns (losses f32[3], acc i64[8], gmax i64[N,S,C])
    -- all on the device, no host synchronisation.  ``reduce_acc(acc)`` (optional) runs between the scans
    and the division: data-parallel training all-reduces the integer sums / counts there so that the
    normalisers 1 + n are global over the batch, as on one GPU."""
    return _partial_loss_fwd(z, None, spx, mask, bits, invT, flags, reduce_acc, None)


def partial_loss_bwd(z, spx, mask, bits, gmax, acc, grad_out, invT, flags):
    """Backward scan: dz [N,C,H,W] for upstream gradients ``grad_out`` f32[3] (device tensor)."""
    return _partial_loss_bwd(z, None, spx, mask, bits, gmax, acc, grad_out, invT, flags, False, None)


def partial_loss_fwd_lowres(zq, size, spx, mask, bits, invT, flags, reduce_acc=None, weights=None):
    """As ``partial_loss_fwd`` for the logits ``F.interpolate(zq, size, 'bilinear', align_corners=False)`` without
    materialising them: ``zq`` [N,C,h,w] quarter-resolution logits, ``size`` = (H, W) of ids / masks.  ``weights`` (f32 [3]
    device tensor: w_ce, w_mc, w_group): ``losses`` gets a fourth entry, the weighted objective (w_ce*ce + w_mc*mc) + w_group*group."""
    return _partial_loss_fwd(zq, size, spx, mask, bits, invT, flags, reduce_acc, weights)


def partial_loss_bwd_lowres(zq, size, spx, mask, bits, gmax, acc, grad_out, invT, flags, want_fix=False, weights=None):
    """Gradient of the losses with respect to the quarter-resolution logits: dzq [N,C,h,w] f32 (and the int64 fixed-point
    sums it was rounded from when ``want_fix``).  With ``weights`` [3], ``grad_out`` is the upstream gradient of the weighted
    objective, a one-element tensor."""
    return _partial_loss_bwd(zq, size, spx, mask, bits, gmax, acc, grad_out, invT, flags, want_fix, weights)


# `flags` of the partial-label entry points (MAS_LOSS_* of include/mulactseg_hip.h); LOSS_RC / LOSS_TOPONE: csrc/partial_label.h
LOSS_CE, LOSS_GROUP, LOSS_GROUP_ONLY_MULTI, LOSS_DECOMP, LOSS_TCE = (_lib.LOSS_CE, _lib.LOSS_GROUP, _lib.LOSS_GROUP_ONLY_MULTI,
                                                                    _lib.LOSS_DECOMP, _lib.LOSS_TCE)
LOSS_RC, LOSS_TOPONE = _lib.LOSS_RC, _lib.LOSS_TOPONE


def partial_loss_reference(z, spx, mask, bits, invT, flags, grad_out=None):
    """The CE-family sums and the full-resolution gradient on HOST tensors: the library's plain loop over the selected pixels through
    csrc/partial_label.h (``mas_partial_loss_reference``), the CPU-side statement of the arithmetic the scans are checked against.
    ``flags``: LOSS_CE, optionally with LOSS_DECOMP and one of LOSS_RC / LOSS_TOPONE.  Returns (losses f32[3], acc i64[8]) and, with
    ``grad_out`` (f32[3], the upstream gradients of (ce, mc, group)), dz [N,C,H,W] as a third value.  Needs no GPU."""
    mask, N, C, H, W, S, _ = _loss_shapes(z, None, None, spx, mask, bits, grad_out, host=True)
    acc = torch.zeros(_lib.ACC_WORDS, dtype=torch.int64)
    losses = torch.zeros(3, dtype=torch.float32)
    dz = torch.empty_like(z) if grad_out is not None else None
    _lib.check(_lib.load().mas_partial_loss_reference(z.data_ptr(), spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(), N, C, H, W,
                                                      S, invT, flags, _opt(grad_out), acc.data_ptr(), losses.data_ptr(), _opt(dz)),
               "mas_partial_loss_reference")
    return (losses, acc) if dz is None else (losses, acc, dz)


class LossState:
    """What a fused forward leaves for its backward: the work buffer (accumulators | arg-pixel table | target bit masks) and views."""
    __slots__ = ("work", "acc", "gmax", "bits", "N", "S", "C", "flags")


def partial_loss_fwd_fused(z, size, spx, mask, invT, flags, targets=None, cols_used=None, bits=None, weights=None, reduce_acc=None):
    """Everything the forward direction launches in ONE library call (mas_partial_loss_fwd_fused: prep, scan, finalize + values).
    ``z`` [N,C,H,W] with ``size`` None, or the quarter-resolution logits [N,C,h,w] with ``size`` = (H, W).  Either ``targets``
    (u8 [N,S,cols], masks over the first ``cols_used`` columns are formed in the prep launch) or ready ``bits`` (int32 [N,S]).
    ``weights`` f32 [3]: losses gets a fourth entry, the weighted objective.  ``reduce_acc`` (data parallel): called on the
    accumulators between the scans and the division.  Returns (losses, LossState)."""
    if targets is None:
        mask, N, C, H, W, S, (h, w) = _loss_shapes(z, None, size, spx, mask, bits)
    else:
        mask, N, C, H, W, S, (h, w) = _loss_shapes(z, None, size, spx, mask, targets, bits_dtype=torch.uint8)
    cols = 0 if targets is None else targets.shape[2]
    cols_used = 0 if targets is None else cols if cols_used is None else int(cols_used)
    values_entry, values_head = _values_call(flags, weights)
    nbytes = int(_lib.load().mas_partial_loss_work_bytes(N, S, C, flags))
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=z.device)     # (zeroed by the prep launch)
    st8 = LossState()
    st8.work, st8.acc, st8.N, st8.S, st8.C, st8.flags = work, work[:_lib.ACC_WORDS], N, S, C, flags
    st8.gmax = work[_lib.ACC_WORDS:_lib.ACC_WORDS + N * S * C].view(N, S, C) if flags & _lib.LOSS_GROUP else None
    st8.bits = bits
    head = (z.data_ptr(), h, w, spx.data_ptr(), _id_code(spx), mask.data_ptr(), _opt(targets), cols, cols_used, _opt(bits), N, C, H, W, S, invT,
            flags, _opt(weights), work.data_ptr(), work.numel() * 8)
    losses = _loss_fwd(z, st8.acc, st8.gmax, n_losses=3 if weights is None else 4, reduce_acc=reduce_acc, entry="mas_partial_loss_fwd_fused",
                       head=head, values_entry=values_entry, values_head=values_head, finalizes=True)
    return losses, st8


def partial_loss_bwd_fused(z, size, spx, mask, state, grad, invT, weights=None, want_fix=False):
    """The backward direction in ONE library call (mas_partial_loss_bwd_fused): dz [N,C,H,W] (``size`` None) or dzq [N,C,h,w]."""
    mask = _mask_u8(mask)
    _need(grad, "grad_out", torch.float32)
    N, C = z.shape[0], z.shape[1]
    low = size is not None
    H, W = (int(size[0]), int(size[1])) if low else (z.shape[2], z.shape[3])
    h, w = (z.shape[2], z.shape[3]) if low else (0, 0)
    dz = torch.empty_like(z)
    fix = torch.empty((N, C, h, w), dtype=torch.int64, device=z.device) if low else None      # (zeroed inside the call)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().mas_partial_loss_bwd_fused(z.data_ptr(), h, w, spx.data_ptr(), _id_code(spx), mask.data_ptr(), _opt(state.bits),
                                                          state.work.data_ptr(), grad.data_ptr(), _opt(weights), N, C, H, W, state.S, invT,
                                                          state.flags, dz.data_ptr(), _opt(fix), _stream(z)), "mas_partial_loss_bwd_fused")
    return (dz, fix) if want_fix else dz


# ------------------------------------------------------------------------------------------------
# teacher-gated candidate terms: a fourth loss slot in the same scans (csrc/teacher_terms.h, k_teacher_loss_fwd / _bwd)
# ------------------------------------------------------------------------------------------------
LOSS_TOP1, LOSS_ENT, LOSS_WITHIN = _lib.LOSS_TOP1, _lib.LOSS_ENT, _lib.LOSS_WITHIN


def _teacher_shapes(z, zt, size, spx, mask, bits, flags, grad_out=None, host=False):
    if (flags & _lib.LOSS_TOP1) and zt is None:
        raise ValueError("LOSS_TOP1 needs the teacher's logits")
    return _loss_shapes(z, zt, size, spx, mask, bits, grad_out, host)


def _teacher_head(z, zt, hw, spx, mask, bits):
    """What the scan entry points of both teacher families begin with."""
    return (z.data_ptr(), _opt(zt), *hw, spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr())


def teacher_loss_fwd(z, zt, size, spx, mask, bits, invT, invT_x, plbl_th, flags, reduce_acc=None):
    """Forward scan with the fourth loss slot: ``flags`` hold LOSS_TOP1 (optionally LOSS_WITHIN; ``zt`` = the eval-mode teacher's
    logits, shaped as ``z``) or LOSS_ENT (``zt`` None) beside LOSS_CE / LOSS_DECOMP / the group flags.  ``invT``: the ce / group
    terms' inverse temperature, ``invT_x``: the fourth slot's own.  ``z`` [N,C,H,W] with ``size`` None, or quarter-resolution
    [N,C,h,w] upsampled in-kernel to ``size``.  Returns (losses f32[4] = ce, mc, group, x; acc i64[16]; gmax or None)."""
    mask, N, C, H, W, S, hw = _teacher_shapes(z, zt, size, spx, mask, bits, flags)
    acc, gmax, _ = _loss_buffers(N, S, C, flags, z.device, words=_lib.TEACHER_ACC_WORDS)
    head = (*_teacher_head(z, zt, hw, spx, mask, bits), N, C, H, W, S, invT, invT_x, plbl_th, flags, _opt(gmax), acc.data_ptr())
    losses = _loss_fwd(z, acc, gmax, n_losses=4, reduce_acc=reduce_acc, entry="mas_teacher_loss_fwd", head=head,
                       values_entry="mas_teacher_loss_values", values_head=(flags,))
    return losses, acc, gmax


def teacher_loss_bwd(z, zt, size, spx, mask, bits, gmax, acc, grad_out, invT, invT_x, plbl_th, flags, want_fix=False):
    """Backward scan of ``teacher_loss_fwd``: the gradient with respect to ``z`` for upstream gradients ``grad_out`` f32[4]; the
    teacher is a constant.  At quarter resolution the sums are int64 fixed point (``want_fix`` returns them too)."""
    mask, N, C, H, W, S, hw = _teacher_shapes(z, zt, size, spx, mask, bits, flags, grad_out)
    return _loss_bwd(z, size, acc, n_scale=4, want_fix=want_fix, scales_entry="mas_teacher_loss_scales", scales_head=(grad_out.data_ptr(), flags),
                     entry="mas_teacher_loss_bwd", head=(*_teacher_head(z, zt, hw, spx, mask, bits), _opt(gmax)),
                     dims=(N, C, H, W, S, invT, invT_x, plbl_th, flags))


def teacher_loss_reference(z, zt, spx, mask, bits, invT, invT_x, plbl_th, flags, grad_out=None):
    """Every term of ``teacher_loss_fwd`` / ``_bwd`` at full resolution on HOST tensors: the library's plain loop through
    csrc/partial_label.h and csrc/teacher_terms.h (``mas_teacher_loss_reference``).  Returns (losses f32[4], acc i64[16], gmax i64
    [N,S,C] or None) and, with ``grad_out`` f32[4], dz [N,C,H,W] as a fourth value.  Needs no GPU."""
    mask, N, C, H, W, S, _ = _teacher_shapes(z, zt, None, spx, mask, bits, flags, grad_out, host=True)
    acc = torch.zeros(_lib.TEACHER_ACC_WORDS, dtype=torch.int64)
    gmax = torch.zeros((N, S, C), dtype=torch.int64) if flags & _lib.LOSS_GROUP else None
    losses = torch.zeros(4, dtype=torch.float32)
    dz = torch.empty_like(z) if grad_out is not None else None
    _lib.check(_lib.load().mas_teacher_loss_reference(z.data_ptr(), _opt(zt), spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(), N,
                                                      C, H, W, S, invT, invT_x, plbl_th, flags, _opt(grad_out), acc.data_ptr(), _opt(gmax),
                                                      losses.data_ptr(), _opt(dz)), "mas_teacher_loss_reference")
    return (losses, acc, gmax) if dz is None else (losses, acc, gmax, dz)


# ------------------------------------------------------------------------------------------------
# teacher-weighted group term: a second (superpixel, class) table beside the student's (csrc/teacher_terms.h, wgroup)
# ------------------------------------------------------------------------------------------------
LOSS_WGROUP = _lib.LOSS_WGROUP


def _wgroup_shapes(z, zt, size, spx, mask, bits, flags, grad_out=None, host=False):
    if not (flags & _lib.LOSS_WGROUP) or not (flags & _lib.LOSS_GROUP):
        raise ValueError("the wgroup entry points take LOSS_WGROUP together with LOSS_GROUP")
    if zt is None:
        raise ValueError("LOSS_WGROUP needs the teacher's logits")
    return _loss_shapes(z, zt, size, spx, mask, bits, grad_out, host)


def wgroup_loss_fwd(z, zt, size, spx, mask, bits, invT, flags, reduce_acc=None):
    """Forward scan and weighted finalize of the teacher-weighted group term: ``flags`` hold LOSS_GROUP | LOSS_WGROUP, optionally with
    LOSS_CE / LOSS_DECOMP / LOSS_GROUP_ONLY_MULTI; ``zt`` = the eval-mode teacher's logits, shaped as ``z``, soft-maxed at the same
    ``invT``.  ``z`` [N,C,H,W] with ``size`` None, or quarter-resolution [N,C,h,w] upsampled in-kernel to ``size``.  Returns (losses
    f32[3] = ce, mc, group; acc i64[8]; gmax i64[N,S,C]; tmax int32[N,S,C], the teacher's maxima as probability bits)."""
    mask, N, C, H, W, S, hw = _wgroup_shapes(z, zt, size, spx, mask, bits, flags)
    acc, gmax, tmax = _loss_buffers(N, S, C, flags, z.device, wgroup=True)
    head = (*_teacher_head(z, zt, hw, spx, mask, bits), N, C, H, W, S, invT, flags, gmax.data_ptr(), tmax.data_ptr(), acc.data_ptr())
    losses = _loss_fwd(z, acc, gmax, n_losses=3, reduce_acc=reduce_acc, entry="mas_wgroup_loss_fwd", head=head,
                       values_entry="mas_loss_values", values_head=(flags & ~_lib.LOSS_WGROUP,), finalizes=True)
    return losses, acc, gmax, tmax


def wgroup_loss_bwd(z, zt, size, spx, mask, bits, gmax, tmax, acc, grad_out, invT, flags, want_fix=False):
    """Backward scan of ``wgroup_loss_fwd``: the gradient with respect to ``z`` for upstream gradients ``grad_out`` f32[3]; both
    tables are read, the teacher is a constant.  At quarter resolution the sums are int64 fixed point (``want_fix`` returns them)."""
    mask, N, C, H, W, S, hw = _wgroup_shapes(z, zt, size, spx, mask, bits, flags, grad_out)
    return _loss_bwd(z, size, acc, n_scale=3, want_fix=want_fix, scales_entry="mas_loss_scales",
                     scales_head=(grad_out.data_ptr(), flags & ~_lib.LOSS_WGROUP), entry="mas_wgroup_loss_bwd",
                     head=(*_teacher_head(z, zt, hw, spx, mask, bits), gmax.data_ptr(), tmax.data_ptr()), dims=(N, C, H, W, S, invT, flags))


def wgroup_loss_reference(z, zt, spx, mask, bits, invT, flags, grad_out=None):
    """Every term of ``wgroup_loss_fwd`` / ``_bwd`` at full resolution on HOST tensors: the library's plain loop through
    csrc/partial_label.h and csrc/teacher_terms.h (``mas_wgroup_loss_reference``).  Returns (losses f32[3], acc i64[8], gmax i64
    [N,S,C], tmax int32[N,S,C]) and, with ``grad_out`` f32[3], dz [N,C,H,W] as a fifth value.  Needs no GPU."""
    mask, N, C, H, W, S, _ = _wgroup_shapes(z, zt, None, spx, mask, bits, flags, grad_out, host=True)
    acc = torch.zeros(_lib.ACC_WORDS, dtype=torch.int64)
    gmax = torch.zeros((N, S, C), dtype=torch.int64)
    tmax = torch.zeros((N, S, C), dtype=torch.int32)
    losses = torch.zeros(3, dtype=torch.float32)
    dz = torch.empty_like(z) if grad_out is not None else None
    _lib.check(_lib.load().mas_wgroup_loss_reference(z.data_ptr(), zt.data_ptr(), spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(),
                                                     N, C, H, W, S, invT, flags, _opt(grad_out), acc.data_ptr(), gmax.data_ptr(),
                                                     tmax.data_ptr(), losses.data_ptr(), _opt(dz)), "mas_wgroup_loss_reference")
    return (losses, acc, gmax, tmax) if dz is None else (losses, acc, gmax, tmax, dz)


# ------------------------------------------------------------------------------------------------
# hierarchical group term: the group scan's arg-pixels spread over the fine superpixels around them (csrc/hier_group.h)
# ------------------------------------------------------------------------------------------------
HIER_ONLY_MULTI, HIER_NOCROPSP = _lib.HIER_ONLY_MULTI, _lib.HIER_NOCROPSP


def _hier_shapes(z, size, spx, small, small_nseg, mask, bits, grad=None, host=False):
    """``_loss_shapes`` plus the fine map: ``small`` ids [N,H,W] of a dtype the id loader knows, ``small_nseg`` > 0.  Full resolution
    (``size`` None) is the same entry points with h = H and w = W, where the taps are exactly (1, 0)."""
    mask, N, C, H, W, S, _ = _loss_shapes(z, None, size, spx, mask, bits, grad, host)
    if host:
        if small.is_cuda or not small.is_contiguous():
            raise ValueError("superpixel_smalls must be a contiguous host tensor")
    else:
        _need(small, "superpixel_smalls")
    if tuple(small.shape) != (N, H, W):
        raise ValueError("superpixel_smalls %s do not match superpixels %s" % (tuple(small.shape), (N, H, W)))
    if int(small_nseg) <= 0:
        raise ValueError("small_nseg must be positive, got %r" % (small_nseg,))
    return mask, N, C, H, W, S, int(small_nseg), z.shape[2], z.shape[3]


def _hier_flags(only_single, nocropsp):
    return (_lib.HIER_ONLY_MULTI if only_single else 0) | (_lib.HIER_NOCROPSP if nocropsp else 0)


def hier_group_loss_fwd(z, size, spx, small, small_nseg, mask, bits, only_single=False, nocropsp=False, reduce_acc=None):
    """Forward of the hierarchical group term in ONE library call: group scan at temperature 1, pair table, tile-queue sum.  ``z``
    [N,C,H,W] with ``size`` None, or quarter-resolution [N,C,h,w] upsampled in-kernel to ``size``; ``bits`` int32 [N,S] over the class
    columns.  Returns a dict: loss f32 [1] = sum / (1 + n); acc i64 [2] = (fixed-point sum, n); mult int32 [N,Ss,C] and any int32
    [N,Ss], the pair table the backward reads; gmax i64 [N,S,C]; bits_eff int32 [N,S] (``nocropsp`` only, else None): ``bits`` with
    the rows of the superpixels on the crop's outermost rows and columns cleared -- ``bits`` itself is not modified."""
    mask, N, C, H, W, S, Ss, h, w = _hier_shapes(z, size, spx, small, small_nseg, mask, bits)
    dev = z.device
    work, gmax, _ = _loss_buffers(N, S, C, _lib.LOSS_GROUP, dev)          # the scan's eight words and its table, contiguous
    tab = torch.empty(N * Ss * C + N * Ss + (N * S if nocropsp else 0), dtype=torch.int32, device=dev)
    mult, any_ = tab[:N * Ss * C].view(N, Ss, C), tab[N * Ss * C:N * Ss * (C + 1)].view(N, Ss)
    bits_eff = tab[N * Ss * (C + 1):].view(N, S) if nocropsp else None
    acc = torch.empty(2, dtype=torch.int64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        st = _stream(z)
        _lib.check(lib.mas_hier_group_fwd(z.data_ptr(), h, w, spx.data_ptr(), _id_code(spx), small.data_ptr(), _id_code(small), mask.data_ptr(),
                                          bits.data_ptr(), N, C, H, W, S, Ss, _hier_flags(only_single, nocropsp), work.data_ptr(),
                                          (work.numel() + gmax.numel()) * 8, _opt(bits_eff), mult.data_ptr(), any_.data_ptr(), acc.data_ptr(),
                                          None if reduce_acc is not None else loss.data_ptr(), st), "mas_hier_group_fwd")
        if reduce_acc is not None:
            reduce_acc(acc)
            _lib.check(lib.mas_hier_group_value(acc.data_ptr(), loss.data_ptr(), st), "mas_hier_group_value")
    return dict(loss=loss, acc=acc, mult=mult, any=any_, gmax=gmax, bits_eff=bits_eff)


def hier_group_loss_bwd(z, size, small, small_nseg, mask, mult, any_, acc, grad, want_fix=False):
    """Backward of ``hier_group_loss_fwd``: the gradient with respect to ``z`` for the upstream gradient ``grad`` f32 [1], summed in
    int64 fixed point (run-to-run identical bytes) and rounded to f32; ``want_fix`` returns (dz, the sums)."""
    _need(z, "inputs", torch.float32)
    _need(small, "superpixel_smalls")
    _need(grad, "grad", torch.float32)
    mask = _mask_u8(mask)
    N, C, h, w = z.shape
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    if tuple(small.shape) != (N, H, W) or tuple(mask.shape) != (N, H, W) or tuple(mult.shape) != (N, int(small_nseg), C):
        raise ValueError("shape mismatch between inputs %s, superpixel_smalls %s, spmasks %s and the pair table %s"
                         % (tuple(z.shape), tuple(small.shape), tuple(mask.shape), tuple(mult.shape)))
    fix = torch.empty(z.shape, dtype=torch.int64, device=z.device)               # (zeroed inside the call)
    dz = torch.empty_like(z)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().mas_hier_group_bwd(z.data_ptr(), h, w, small.data_ptr(), _id_code(small), mask.data_ptr(), mult.data_ptr(),
                                                  any_.data_ptr(), acc.data_ptr(), grad.data_ptr(), N, C, H, W, int(small_nseg),
                                                  fix.data_ptr(), dz.data_ptr(), _stream(z)), "mas_hier_group_bwd")
    return (dz, fix) if want_fix else dz


def hier_group_loss_reference(z, size, spx, small, small_nseg, mask, bits, only_single=False, nocropsp=False, grad=None):
    """``hier_group_loss_fwd`` / ``_bwd`` on HOST tensors: the library's plain loop through csrc/hier_group.h
    (``mas_hier_group_reference``), the statement the kernels are held to bit for bit.  Needs no GPU.  Returns the forward's dict and,
    with ``grad`` f32 [1], dzq_fix i64 (shaped as ``z``) and dz f32."""
    mask, N, C, H, W, S, Ss, h, w = _hier_shapes(z, size, spx, small, small_nseg, mask, bits, grad, host=True)
    gmax = torch.zeros((N, S, C), dtype=torch.int64)
    mult, any_ = torch.zeros((N, Ss, C), dtype=torch.int32), torch.zeros((N, Ss), dtype=torch.int32)
    bits_eff = torch.zeros((N, S), dtype=torch.int32) if nocropsp else None
    acc, loss = torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.float32)
    fix = torch.zeros(z.shape, dtype=torch.int64) if grad is not None else None
    _lib.check(_lib.load().mas_hier_group_reference(z.data_ptr(), h, w, spx.data_ptr(), _id_code(spx), small.data_ptr(), _id_code(small),
                                                    mask.data_ptr(), bits.data_ptr(), N, C, H, W, S, Ss, _hier_flags(only_single, nocropsp),
                                                    _opt(grad), gmax.data_ptr(), _opt(bits_eff), mult.data_ptr(), any_.data_ptr(),
                                                    acc.data_ptr(), loss.data_ptr(), _opt(fix)), "mas_hier_group_reference")
    out = dict(loss=loss, acc=acc, mult=mult, any=any_, gmax=gmax, bits_eff=bits_eff)
    if fix is not None:
        out.update(dzq_fix=fix, dz=(fix.to(torch.float64) * 2.0 ** -_lib.GRAD_FRAC).to(torch.float32))
    return out


# ------------------------------------------------------------------------------------------------
# cross-view hierarchical group term: the pair table of a weak view, the sum over the strong view (csrc/hier_group.h, second section)
# ------------------------------------------------------------------------------------------------
_WEIGHT_MODES = {None: _lib.AHG_WEIGHT_NONE, 'max': _lib.AHG_WEIGHT_MAX, 'mean': _lib.AHG_WEIGHT_MEAN}


def weight_reduce_mode(weight_reduce):
    """``--weight_reduce`` as the library's mode: None (the unweighted class), 'max' or 'mean'."""
    try:
        return _WEIGHT_MODES[weight_reduce]
    except (KeyError, TypeError):
        raise ValueError("weight_reduce must be None, 'max' or 'mean', got %r" % (weight_reduce,))


def async_hier_tables(zq_weak, size_weak, spx_weak, small_weak, small_nseg, mask_weak, bits, weight_reduce=None):
    """The tables of the cross-view hierarchical group term from the WEAK view in ONE library call: the group scan at temperature 1 on
    the teacher's logits ``zq_weak`` [N,C,h_o,w_o] upsampled in-kernel to ``size_weak`` (None: full-resolution logits), the pair table,
    and with ``weight_reduce`` 'max' / 'mean' the teacher's per-pair weight.  Returns a dict: mult int32 [N,Ss,C], any int32 [N,Ss],
    gmax i64 [N,S,C], wgt f32 [N,Ss,C] (None without ``weight_reduce``).  Run-to-run identical bytes."""
    mode = weight_reduce_mode(weight_reduce)
    mask_weak, N, C, H, W, S, Ss, h, w = _hier_shapes(zq_weak, size_weak, spx_weak, small_weak, small_nseg, mask_weak, bits)
    dev = zq_weak.device
    lib = _lib.load()
    nbytes = lib.mas_async_hier_work_bytes(N, S, Ss, C, mode)
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)                  # (zeroed inside the call)
    tab = torch.empty(N * Ss * C + N * Ss, dtype=torch.int32, device=dev)
    mult, any_ = tab[:N * Ss * C].view(N, Ss, C), tab[N * Ss * C:].view(N, Ss)
    wgt = torch.empty((N, Ss, C), dtype=torch.float32, device=dev) if mode else None
    with torch.cuda.device(dev):
        _lib.check(lib.mas_async_hier_tables(zq_weak.data_ptr(), h, w, spx_weak.data_ptr(), _id_code(spx_weak), small_weak.data_ptr(),
                                             _id_code(small_weak), mask_weak.data_ptr(), bits.data_ptr(), N, C, H, W, S, Ss, mode,
                                             work.data_ptr(), nbytes, mult.data_ptr(), any_.data_ptr(), _opt(wgt), _stream(zq_weak)),
                   "mas_async_hier_tables")
    return dict(mult=mult, any=any_, gmax=work[8:8 + N * S * C].view(N, S, C), wgt=wgt)


def _async_strong_shapes(z, size, small, small_nseg, mask, mult, any_, wgt, host=False):
    N, C, h, w = z.shape
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    Ss = int(small_nseg)
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    for t, name, dt in ((z, "inputs", torch.float32), (small, "superpixel_smalls", None), (mask, "spmasks", torch.uint8),
                        (mult, "mult", torch.int32), (any_, "any", torch.int32), (wgt, "wgt", torch.float32)):
        if t is None:
            continue
        if host:
            if t.is_cuda or not t.is_contiguous():
                raise ValueError("%s must be a contiguous host tensor" % name)
            if dt is not None and t.dtype != dt:
                raise TypeError("%s must be %s, got %s" % (name, dt, t.dtype))
        else:
            _need(t, name, dt)
    if (Ss <= 0 or tuple(small.shape) != (N, H, W) or tuple(mask.shape) != (N, H, W) or tuple(mult.shape) != (N, Ss, C)
            or tuple(any_.shape) != (N, Ss) or (wgt is not None and tuple(wgt.shape) != (N, Ss, C))):
        raise ValueError("shape mismatch between inputs %s, superpixel_smalls %s, spmasks %s, the pair table %s / %s and its weights %s"
                         % (tuple(z.shape), tuple(small.shape), tuple(mask.shape), tuple(mult.shape), tuple(any_.shape),
                            None if wgt is None else tuple(wgt.shape)))
    return mask, N, C, H, W, Ss, h, w


def async_hier_loss_fwd(z, size, small, small_nseg, mask, mult, any_, wgt=None, reduce_acc=None):
    """Forward of the cross-view term on GIVEN tables over the STRONG view: ``z`` [N,C,H,W] (``size`` None) or quarter-resolution
    [N,C,h,w] upsampled in-kernel to ``size``.  ``wgt`` None is the unweighted class (the kernels of ``hier_group_loss_fwd``); with
    ``wgt`` every pair's term is multiplied by its weight and a pair of weight 0 is not counted.  Returns (loss f32 [1], acc i64 [2])."""
    mask, N, C, H, W, Ss, h, w = _async_strong_shapes(z, size, small, small_nseg, mask, mult, any_, wgt)
    acc = torch.empty(2, dtype=torch.int64, device=z.device)
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    lib = _lib.load()
    with torch.cuda.device(z.device):
        st = _stream(z)
        _lib.check(lib.mas_async_hier_fwd(z.data_ptr(), h, w, small.data_ptr(), _id_code(small), mask.data_ptr(), mult.data_ptr(),
                                          any_.data_ptr(), _opt(wgt), N, C, H, W, Ss, acc.data_ptr(),
                                          None if reduce_acc is not None else loss.data_ptr(), st), "mas_async_hier_fwd")
        if reduce_acc is not None:
            reduce_acc(acc)
            _lib.check(lib.mas_async_hier_value(acc.data_ptr(), loss.data_ptr(), st), "mas_async_hier_value")
    return loss, acc


def async_hier_loss_bwd(z, size, small, small_nseg, mask, mult, any_, wgt, acc, grad, want_fix=False):
    """Backward of ``async_hier_loss_fwd``: the gradient with respect to ``z`` for the upstream gradient ``grad`` f32 [1], summed in
    int64 fixed point (run-to-run identical bytes) and rounded to f32; ``want_fix`` returns (dz, the sums)."""
    mask, N, C, H, W, Ss, h, w = _async_strong_shapes(z, size, small, small_nseg, mask, mult, any_, wgt)
    _need(grad, "grad", torch.float32)
    fix = torch.empty(z.shape, dtype=torch.int64, device=z.device)               # (zeroed inside the call)
    dz = torch.empty_like(z)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().mas_async_hier_bwd(z.data_ptr(), h, w, small.data_ptr(), _id_code(small), mask.data_ptr(), mult.data_ptr(),
                                                  any_.data_ptr(), _opt(wgt), acc.data_ptr(), grad.data_ptr(), N, C, H, W, Ss,
                                                  fix.data_ptr(), dz.data_ptr(), _stream(z)), "mas_async_hier_bwd")
    return (dz, fix) if want_fix else dz


def async_hier_loss_reference(z, size, small, small_nseg, mask, weak=None, tables=None, weight_reduce=None, grad=None):
    """The cross-view term on HOST tensors: the library's plain loop through csrc/hier_group.h (``mas_async_hier_reference``), the
    statement the kernels are held to bit for bit.  Needs no GPU.  ``weak`` = (zq_weak, size_weak, spx_weak, small_weak, mask_weak,
    bits): the tables are built from that view (``weight_reduce`` None / 'max' / 'mean').  ``tables`` = (mult, any, wgt or None)
    instead: they are used as given (``weight_reduce`` is ignored).  Returns a dict: loss, acc, mult, any, wgt, gmax (None with
    ``tables``) and, with ``grad`` f32 [1], dzq_fix i64 (shaped as ``z``) and dz f32."""
    if (weak is None) == (tables is None):
        raise ValueError("give either the weak view or the tables")
    Ss = int(small_nseg)
    N, C = z.shape[:2]
    gmax = None
    if tables is not None:
        mult, any_, wgt = tables
        mode = _lib.AHG_TABLES_GIVEN | (_lib.AHG_WEIGHT_MAX if wgt is not None else 0)
        head = (None, 0, 0, None, 0, None, 0, None, None, 0, 0, 0)
    else:
        zw, size_w, spx_w, small_w, mask_w, bits = weak
        mask_w, Nw, Cw, Ho, Wo, S, _, ho, wo = _hier_shapes(zw, size_w, spx_w, small_w, Ss, mask_w, bits, host=True)
        if (Nw, Cw) != (N, C):
            raise ValueError("the weak view %s does not match the strong view %s" % (tuple(zw.shape), tuple(z.shape)))
        mode = weight_reduce_mode(weight_reduce)
        gmax = torch.zeros((N, S, C), dtype=torch.int64)
        mult, any_ = torch.zeros((N, Ss, C), dtype=torch.int32), torch.zeros((N, Ss), dtype=torch.int32)
        wgt = torch.zeros((N, Ss, C), dtype=torch.float32) if mode else None
        head = (zw.data_ptr(), ho, wo, spx_w.data_ptr(), _id_code(spx_w), small_w.data_ptr(), _id_code(small_w), mask_w.data_ptr(),
                bits.data_ptr(), Ho, Wo, S)
    mask, N, C, H, W, Ss, h, w = _async_strong_shapes(z, size, small, Ss, mask, mult, any_, wgt, host=True)
    if grad is not None and (grad.is_cuda or grad.dtype != torch.float32):
        raise TypeError("grad must be a float32 host tensor")
    acc, loss = torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.float32)
    fix = torch.zeros(z.shape, dtype=torch.int64) if grad is not None else None
    _lib.check(_lib.load().mas_async_hier_reference(*head, mode, z.data_ptr(), h, w, small.data_ptr(), _id_code(small), mask.data_ptr(), N, C,
                                                    H, W, Ss, _opt(grad), _opt(gmax), mult.data_ptr(), any_.data_ptr(), _opt(wgt),
                                                    acc.data_ptr(), loss.data_ptr(), _opt(fix)), "mas_async_hier_reference")
    out = dict(loss=loss, acc=acc, mult=mult, any=any_, wgt=wgt, gmax=gmax)
    if fix is not None:
        out.update(dzq_fix=fix, dz=(fix.to(torch.float64) * 2.0 ** -_lib.GRAD_FRAC).to(torch.float32))
    return out


# ------------------------------------------------------------------------------------------------
# online local-prototype pseudo labels and the cross entropy on them (csrc/online_plbl.hip)
# ------------------------------------------------------------------------------------------------
LCE_UNWEIGHTED, LCE_WEIGHTED, LCE_THRESHOLD, LCE_EMPTY_NAN = _lib.LCE_UNWEIGHTED, _lib.LCE_WEIGHTED, _lib.LCE_THRESHOLD, _lib.LCE_EMPTY_NAN
LCE_SIGNED = _lib.LCE_SIGNED


def _plbl_bits(targets, bits):
    if (targets is None) == (bits is None):
        raise ValueError("give either targets (u8 [N,S,cols]) or bits (int32 [N,S])")
    if bits is None:
        bits = target_bits(targets.contiguous() if targets.dtype == torch.uint8 else targets.to(torch.uint8).contiguous())
    return bits


def _plbl_shapes(zq_p, featq, size, spx, mask, bits):
    N, C, h, w = zq_p.shape
    H, W = int(size[0]), int(size[1])
    if featq.dim() != 4 or featq.shape[0] != N or tuple(featq.shape[2:]) != (h, w):
        raise ValueError("features %s do not match the logits %s" % (tuple(featq.shape), tuple(zq_p.shape)))
    if tuple(spx.shape) != (N, H, W) or tuple(mask.shape) != (N, H, W) or bits.dim() != 2 or bits.shape[0] != N:
        raise ValueError("shape mismatch between logits %s at size %s, superpixels %s, spmasks %s, targets %s"
                         % (tuple(zq_p.shape), (H, W), tuple(spx.shape), tuple(mask.shape), tuple(bits.shape)))
    return N, C, h, w, H, W, featq.shape[1], bits.shape[1]


def _weight_flags(weight_wo_proto, weight_sim):
    return (_lib.OPL_WEIGHT_WO_PROTO if weight_wo_proto else 0) | (_lib.OPL_WEIGHT_SIM if weight_sim else 0)


def _plbl_args(zq_p, featq, size, spx, mask, targets, bits, work_bytes="mas_online_plbl_work_bytes"):
    """What the per-pixel prototype entry points take: the checked arguments up to S in call order, the work buffer (sized by the entry
    point's own ``work_bytes`` function) and its size, the (N, C, H, W) of the outputs, ``bits``, and the tensors behind the pointers
    that the caller holds until it has made the call."""
    _need(zq_p, "inputs_plbl", torch.float32)
    _need(featq, "feats_plbl", torch.float32)
    _need(spx, "superpixels")
    mask = _mask_u8(mask)
    bits = _need(_plbl_bits(targets, bits), "bits", torch.int32)
    N, C, h, w, H, W, Ch, S = _plbl_shapes(zq_p, featq, size, spx, mask, bits)
    nbytes = int(getattr(_lib.load(), work_bytes)(N, S, C))
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=zq_p.device)  # (zeroed inside the call)
    head = (zq_p.data_ptr(), featq.data_ptr(), Ch, h, w, spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(), N, C, H, W, S)
    return head, (work.data_ptr(), work.numel() * 8), (N, C, H, W), bits, (mask, work)


def online_pseudo_labels(zq_p, featq, size, spx, mask, targets=None, bits=None, invT=1.0, weight_wo_proto=False, weight_sim=False):
    """The reference's ``generate_plbl`` (``trainer/active_onlinewplbl_multi_predignore.py:20-125``) for the whole batch in ONE library
    call and without a host round trip: ``zq_p`` [N,C,h,w] quarter-resolution logits of the eval-mode forward, ``featq`` [N,Ch,h,w]
    its L2-normalised point features, both interpolated to ``size`` = (H, W) per pixel inside the kernel; ``spx`` / ``mask`` [N,H,W];
    ``targets`` u8 [N,S,cols] or ready ``bits`` int32 [N,S].  Returns (labels u8 [N,H,W], 255 = none; weight f32 [N,H,W], 0 = none).
    ``weight_sim``: the weight is the pixel's inner product with the chosen prototype (``LocalsimWProtoCE``), which may be negative,
    instead of the softmax probability of the label; the library refuses it together with ``weight_wo_proto``."""
    head, work, (N, C, H, W), bits, _keep = _plbl_args(zq_p, featq, size, spx, mask, targets, bits)
    dev = zq_p.device
    labels = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    weight = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_online_plbl_labels(*head, invT, _weight_flags(weight_wo_proto, weight_sim), *work, labels.data_ptr(),
                                                      weight.data_ptr(), _stream(zq_p)), "mas_online_plbl_labels")
    return labels, weight


def _label_ce_check(zq, size, labels, weight, flags):
    N, C, h, w = zq.shape
    H, W = int(size[0]), int(size[1])
    if tuple(labels.shape) != (N, H, W) or (weight is not None and tuple(weight.shape) != (N, H, W)):
        raise ValueError("labels %s / weight %s do not match logits %s at size %s"
                         % (tuple(labels.shape), None if weight is None else tuple(weight.shape), tuple(zq.shape), (H, W)))
    if weight is None and (flags & 3) != _lib.LCE_UNWEIGHTED:
        raise ValueError("the weighted and threshold modes need a weight map")
    return N, C, h, w, H, W


def _ce_fwd(zq, reduce_acc, value_flags, entry, head):
    """The forward half both cross entropies share: ``entry(*head, acc, loss, stream)`` fills acc, and loss unless ``reduce_acc`` runs
    first, between the scan and the division.  Returns (loss f32 [1], acc i64 [2])."""
    acc = torch.empty(2, dtype=torch.int64, device=zq.device)                     # (zeroed inside the call)
    loss = torch.empty(1, dtype=torch.float32, device=zq.device)
    lib = _lib.load()
    with torch.cuda.device(zq.device):
        st = _stream(zq)
        _lib.check(getattr(lib, entry)(*head, acc.data_ptr(), None if reduce_acc is not None else loss.data_ptr(), st), entry)
        if reduce_acc is not None:
            reduce_acc(acc)
            _lib.check(lib.mas_label_ce_value(acc.data_ptr(), value_flags, loss.data_ptr(), st), "mas_label_ce_value")
    return loss, acc


def _ce_bwd(zq, want_fix, entry, head):
    """The backward half: ``entry(*head, fix, dzq, stream)`` fills the int64 sums and dzq.  Returns dzq, or (dzq, fix)."""
    fix = torch.empty(zq.shape, dtype=torch.int64, device=zq.device)              # (zeroed inside the call)
    dzq = torch.empty_like(zq)
    with torch.cuda.device(zq.device):
        _lib.check(getattr(_lib.load(), entry)(*head, fix.data_ptr(), dzq.data_ptr(), _stream(zq)), entry)
    return (dzq, fix) if want_fix else dzq


def label_ce_fwd_lowres(zq, size, labels, weight, invT, flags, th=0.0, reduce_acc=None):
    """Forward half of ``label_ce_lowres``: (loss f32 [1], acc i64 [2] = fixed-point sum and count).  ``reduce_acc(acc)`` (data
    parallel) runs between the scan and the division, so the mean is over the global batch."""
    _need(zq, "inputs", torch.float32)
    _need(labels, "labels", torch.uint8)
    if weight is not None:
        _need(weight, "weight", torch.float32)
    N, C, h, w, H, W = _label_ce_check(zq, size, labels, weight, flags)
    return _ce_fwd(zq, reduce_acc, flags, "mas_label_ce_fwd_lowres",
                   (zq.data_ptr(), h, w, labels.data_ptr(), _opt(weight), N, C, H, W, invT, flags, float(th)))


def label_ce_bwd_lowres(zq, size, labels, weight, acc, grad, invT, flags, th=0.0, want_fix=False):
    """Backward half: dzq [N,C,h,w] f32 for the upstream gradient ``grad`` f32 [1] (and the int64 sums it was rounded from)."""
    _need(grad, "grad", torch.float32)
    N, C, h, w, H, W = _label_ce_check(zq, size, labels, weight, flags)
    return _ce_bwd(zq, want_fix, "mas_label_ce_bwd_lowres", (zq.data_ptr(), h, w, labels.data_ptr(), _opt(weight), acc.data_ptr(),
                                                             grad.data_ptr(), N, C, H, W, invT, flags, float(th)))


class _LabelCELowRes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zq, size, labels, weight, invT, flags, th, reduce_acc):
        zq = zq.contiguous()
        loss, acc = label_ce_fwd_lowres(zq, size, labels, weight, invT, flags, th, reduce_acc)
        ctx.save_for_backward(zq, labels, acc, weight if weight is not None else acc)
        ctx.has_w, ctx.size, ctx.invT, ctx.flags, ctx.th = weight is not None, size, invT, flags, th
        ctx.mark_non_differentiable(acc)
        return loss[0], acc

    @staticmethod
    def backward(ctx, g, _g_acc):
        zq, labels, acc, weight = ctx.saved_tensors
        dzq = label_ce_bwd_lowres(zq, ctx.size, labels, weight if ctx.has_w else None, acc, g.reshape(1).to(torch.float32).contiguous(),
                                  ctx.invT, ctx.flags, ctx.th)
        return dzq, None, None, None, None, None, None, None


def label_ce_lowres(zq, size, labels, weight, invT, mode=LCE_UNWEIGHTED, th=0.0, empty_nan=False, reduce_acc=None, signed=False):
    """Mean cross entropy of ``F.interpolate(zq, size, 'bilinear', align_corners=False) * invT`` against ``labels`` u8 [N,H,W]
    (255 = none) with per-pixel weights, differentiable in ``zq``; the upsampled logits and their gradient never exist.  ``mode``:
    LCE_UNWEIGHTED (mean over the labelled pixels), LCE_WEIGHTED (``weight * ce``) or LCE_THRESHOLD (``(th < weight) * ce``), the last
    two averaged over the non-zero terms.  No labelled (non-zero) pixel: 0, or NaN with ``empty_nan``.  ``signed`` (LCE_WEIGHTED only):
    the weights may be negative and a negative term subtracts from the sum; without it such a term adds 0.  Returns (loss, acc).  The
    ``label_ce_fwd_lowres`` / ``_bwd_lowres`` halves take the same bit as ``LCE_SIGNED`` in ``flags``."""
    flags = int(mode) | (_lib.LCE_EMPTY_NAN if empty_nan else 0) | (_lib.LCE_SIGNED if signed else 0)
    return _LabelCELowRes.apply(zq, (int(size[0]), int(size[1])), labels, weight, invT, flags, float(th), reduce_acc)


def online_plbl_reference(zq_p, featq, size, spx, mask, targets=None, bits=None, invT=1.0, weight_wo_proto=False, zq=None, invT_ce=None,
                          mode=LCE_UNWEIGHTED, th=0.0, empty_nan=False, grad=None, labels=None, weight=None, weight_sim=False, signed=False):
    """``online_pseudo_labels`` and ``label_ce_lowres`` on HOST tensors: the library's plain loop through csrc/online_plbl.h
    (``mas_online_plbl_reference``), the CPU-side statement of the arithmetic the kernels are checked against.  Needs no GPU.
    With ``zq_p`` None the label and weight maps are the given ``labels`` / ``weight``.  ``weight_sim`` / ``signed`` as in
    ``online_pseudo_labels`` / ``label_ce_lowres``.  Returns a dict: labels, weight, gmax (the
    arg-pixel table, when labels were generated), and with ``zq``: loss f32 [1], acc i64 [2], and with ``grad`` (f32 [1]) dzq_fix."""
    out = {}
    lib = _lib.load()
    for t in (zq_p, featq, spx, mask, zq, grad, labels, weight, bits, targets):
        if t is not None and (t.is_cuda or not t.is_contiguous()):
            raise ValueError("online_plbl_reference takes contiguous host tensors")
    src = zq_p if zq_p is not None else zq
    N, C, h, w = src.shape
    H, W = int(size[0]), int(size[1])
    if zq_p is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        bits = _plbl_bits_host(targets, bits)
        _plbl_shapes(zq_p, featq, size, spx, mask, bits)
        Ch, S = featq.shape[1], bits.shape[1]
        labels = torch.empty((N, H, W), dtype=torch.uint8)
        weight = torch.empty((N, H, W), dtype=torch.float32)
        gmax = out['gmax'] = torch.zeros((N, S, C), dtype=torch.int64)
        gen = (zq_p.data_ptr(), featq.data_ptr(), Ch, h, w, spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr())
    else:
        S, gmax = 1, None
        gen = (None, None, 1, h, w, None, 0, None, None)
    acc = loss = fix = None
    if zq is not None:
        acc, loss = torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.float32)
        fix = torch.zeros(zq.shape, dtype=torch.int64) if grad is not None else None
    flags = int(mode) | (_lib.LCE_EMPTY_NAN if empty_nan else 0) | (_lib.LCE_SIGNED if signed else 0)
    _lib.check(lib.mas_online_plbl_reference(*gen, N, C, H, W, S, invT, _weight_flags(weight_wo_proto, weight_sim), _opt(gmax),
                                             labels.data_ptr(), _opt(weight), _opt(zq), invT if invT_ce is None else invT_ce, flags, float(th),
                                             _opt(grad), _opt(acc), _opt(loss), _opt(fix)), "mas_online_plbl_reference")
    out.update(labels=labels, weight=weight)
    if zq is not None:
        out.update(loss=loss, acc=acc)
        if fix is not None:
            out['dzq_fix'] = fix
    return out


# ------------------------------------------------------------------------------------------------
# local-prototype label quality inside the queried superpixels (csrc/within_eval.hip)
# ------------------------------------------------------------------------------------------------
WE_MODES = {'proto': _lib.WE_PROTO, 'filt': _lib.WE_FILT}


def _we_mode(mode):
    try:
        return WE_MODES[mode]
    except KeyError:
        raise ValueError("mode must be 'proto' or 'filt', got %r" % (mode,))


def _we_classes(num_classes, C):
    K = C if num_classes is None else int(num_classes)
    if K < C or K > _lib.MAX_CLASSES:
        raise ValueError("num_classes must lie in [C = %d, %d], got %d" % (C, _lib.MAX_CLASSES, K))
    return K


def within_multihot_eval(zq, featq, size, spx, mask, gt, targets=None, bits=None, mode='proto', num_classes=None, ignore_label=255,
                         counts=None, diag=None, want_labels=False):
    """The label generation of the reference's ``eval_cosplbl_within_multihot`` family (``trainer/eval_cosplbl_within_multihot.py:
    84-179``; ``mode='filt'``: ``eval_cosplbl_filt_within_multihot.py:162-169``) and ``MeanIoU._after_step`` on its result, for the whole
    batch in ONE library call: ``zq`` [N,C,h,w] quarter-resolution logits of the eval-mode forward, ``featq`` [N,Ch,h,w] its
    L2-normalised point features, both interpolated to ``size`` = (H, W) per pixel inside the kernel; ``spx`` / ``mask`` / ``gt``
    (int64) [N,H,W]; ``targets`` u8 [N,S,cols] or ready ``bits`` int32 [N,S].  A selected pixel of a superpixel with a non-empty row
    takes the candidate class with the nearest local prototype; every other pixel is 255.  Adds to ``counts`` int64 [3K+3]
    (K = ``num_classes`` >= C, default C) what ``iou_counts`` adds for that map, and to ``diag`` int64 [4] the valid pixels, the
    prototypes, the valid pixels whose winning similarity is below ``max_c (logit_c * Y_c)``, and the labels the filter removed.
    Returns (counts, diag, labels u8 [N,H,W] or None); the label map exists only with ``want_labels``."""
    head, work, (N, C, H, W), bits, _keep = _plbl_args(zq, featq, size, spx, mask, targets, bits, "mas_within_eval_work_bytes")
    _need(gt, "labels", torch.int64)
    if tuple(gt.shape) != (N, H, W):
        raise ValueError("ground truth %s does not match the size %s" % (tuple(gt.shape), (N, H, W)))
    K, dev = _we_classes(num_classes, C), zq.device
    if counts is None:
        counts = torch.zeros(3 * K + 3, dtype=torch.int64, device=dev)
    if diag is None:
        diag = torch.zeros(4, dtype=torch.int64, device=dev)
    _need(counts, "counts", torch.int64)
    _need(diag, "diag", torch.int64)
    if counts.numel() != 3 * K + 3 or diag.numel() != 4:
        raise ValueError("counts must hold 3K+3 = %d and diag 4 elements" % (3 * K + 3))
    labels = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if want_labels else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_within_eval_counts(*head, gt.data_ptr(), _we_mode(mode), K, int(ignore_label), *work, counts.data_ptr(),
                                                      diag.data_ptr(), _opt(labels), _stream(zq)), "mas_within_eval_counts")
    return counts, diag, labels


def within_multihot_reference(zq, featq, size, spx, mask, gt, targets=None, bits=None, mode='proto', num_classes=None, ignore_label=255,
                              counts=None, diag=None):
    """``within_multihot_eval`` on HOST tensors: the library's plain loop through csrc/within_eval.h (``mas_within_eval_reference``),
    the CPU-side statement of the arithmetic the kernel is checked against.  Needs no GPU.  Returns a dict: counts, diag, labels (u8,
    always), gmax (the arg-pixel table)."""
    for t in (zq, featq, spx, mask, gt, bits, targets, counts, diag):
        if t is not None and (t.is_cuda or not t.is_contiguous()):
            raise ValueError("within_multihot_reference takes contiguous host tensors")
    if zq.dtype != torch.float32 or featq.dtype != torch.float32 or gt.dtype != torch.int64:
        raise TypeError("logits and features must be float32, the ground truth int64")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    bits = _plbl_bits_host(targets, bits)
    N, C, h, w, H, W, Ch, S = _plbl_shapes(zq, featq, size, spx, mask, bits)
    if tuple(gt.shape) != (N, H, W):
        raise ValueError("ground truth %s does not match the size %s" % (tuple(gt.shape), (N, H, W)))
    K = _we_classes(num_classes, C)
    counts = torch.zeros(3 * K + 3, dtype=torch.int64) if counts is None else counts
    diag = torch.zeros(4, dtype=torch.int64) if diag is None else diag
    labels = torch.empty((N, H, W), dtype=torch.uint8)
    gmax = torch.zeros((N, S, C), dtype=torch.int64)
    _lib.check(_lib.load().mas_within_eval_reference(zq.data_ptr(), featq.data_ptr(), Ch, h, w, spx.data_ptr(), _id_code(spx), mask.data_ptr(),
                                                     bits.data_ptr(), N, C, H, W, S, gt.data_ptr(), _we_mode(mode), K, int(ignore_label),
                                                     counts.data_ptr(), diag.data_ptr(), labels.data_ptr(), gmax.data_ptr()),
               "mas_within_eval_reference")
    return dict(counts=counts, diag=diag, labels=labels, gmax=gmax)


def online_soft_weights(zq_p, featq, size, spx, mask, targets=None, bits=None, invT=1.0, inv_tau=1.0):
    """The soft targets of the reference's ``JointLocalProtoWeightingCE`` (``trainer/active_pwce_multi_predignore.py:73-139``) for the
    whole batch in ONE library call, no host round trip; arguments as ``online_pseudo_labels``.  Every valid pixel (selected, id in
    range, multi-hot superpixel) gets, over its candidate classes, the softmax of its inner products with the classes' local prototypes
    at ``inv_tau`` = ``inv_temperature(simw_temp)``.  Returns (softw f32 [N,C,H,W], allocated uninitialised: only the candidate planes
    of valid pixels are written or read; live int32 [N]: the pictures with a valid pixel; bits int32 [N,S])."""
    head, work, (N, C, H, W), bits, _keep = _plbl_args(zq_p, featq, size, spx, mask, targets, bits)
    dev = zq_p.device
    softw = torch.empty((N, C, H, W), dtype=torch.float32, device=dev)
    live = torch.empty(N, dtype=torch.int32, device=dev)                           # (zeroed inside the call)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_online_soft_weights(*head, invT, inv_tau, *work, softw.data_ptr(), live.data_ptr(), _stream(zq_p)),
                   "mas_online_soft_weights")
    return softw, live, bits


def _soft_ce_check(zq, size, spx, mask, bits, softw, live):
    N, C, h, w = zq.shape
    H, W = int(size[0]), int(size[1])
    if (tuple(spx.shape) != (N, H, W) or tuple(mask.shape) != (N, H, W) or bits.dim() != 2 or bits.shape[0] != N
            or tuple(softw.shape) != (N, C, H, W) or tuple(live.shape) != (N,)):
        raise ValueError("shape mismatch between logits %s at size %s, superpixels %s, spmasks %s, bits %s, soft weights %s, live %s"
                         % (tuple(zq.shape), (H, W), tuple(spx.shape), tuple(mask.shape), tuple(bits.shape), tuple(softw.shape),
                            tuple(live.shape)))
    return N, C, h, w, H, W, bits.shape[1]


def soft_ce_fwd_lowres(zq, size, spx, mask, bits, softw, live, invT, reduce_acc=None):
    """Forward half of ``soft_ce_lowres``: (loss f32 [1], acc i64 [2] = fixed-point sum and count); ``reduce_acc`` as in
    ``label_ce_fwd_lowres``."""
    _need(zq, "inputs", torch.float32)
    _need(spx, "superpixels")
    _need(mask, "spmasks", torch.uint8)
    _need(bits, "bits", torch.int32)
    _need(softw, "softw", torch.float32)
    _need(live, "live", torch.int32)
    N, C, h, w, H, W, S = _soft_ce_check(zq, size, spx, mask, bits, softw, live)
    return _ce_fwd(zq, reduce_acc, 0, "mas_soft_ce_fwd_lowres",
                   (zq.data_ptr(), h, w, spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(), softw.data_ptr(), live.data_ptr(),
                    N, C, H, W, S, invT))


def soft_ce_bwd_lowres(zq, size, spx, mask, bits, softw, live, acc, grad, invT, want_fix=False):
    """Backward half: dzq [N,C,h,w] f32 for the upstream gradient ``grad`` f32 [1] (and the int64 sums it was rounded from)."""
    _need(grad, "grad", torch.float32)
    N, C, h, w, H, W, S = _soft_ce_check(zq, size, spx, mask, bits, softw, live)
    return _ce_bwd(zq, want_fix, "mas_soft_ce_bwd_lowres",
                   (zq.data_ptr(), h, w, spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(), softw.data_ptr(), live.data_ptr(),
                    acc.data_ptr(), grad.data_ptr(), N, C, H, W, S, invT))


class _SoftCELowRes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zq, size, spx, mask, bits, softw, live, invT, reduce_acc):
        zq = zq.contiguous()
        loss, acc = soft_ce_fwd_lowres(zq, size, spx, mask, bits, softw, live, invT, reduce_acc)
        ctx.save_for_backward(zq, spx, mask, bits, softw, live, acc)
        ctx.size, ctx.invT = size, invT
        ctx.mark_non_differentiable(acc)
        return loss[0], acc

    @staticmethod
    def backward(ctx, g, _g_acc):
        zq, spx, mask, bits, softw, live, acc = ctx.saved_tensors
        dzq = soft_ce_bwd_lowres(zq, ctx.size, spx, mask, bits, softw, live, acc, g.reshape(1).to(torch.float32).contiguous(), ctx.invT)
        return dzq, None, None, None, None, None, None, None, None


def soft_ce_lowres(zq, size, spx, mask, bits, softw, live, invT, reduce_acc=None):
    """Mean over the counted pixels (selected, id in range, in a ``live`` picture) of the cross entropy of
    ``softmax(F.interpolate(zq, size, 'bilinear', align_corners=False) * invT)`` against the soft targets of ``online_soft_weights``:
    ``sum_c softw_c * -log(p_c + 1e-8)`` for a pixel of a multi-hot superpixel, ``-log(p_c + 1e-8)`` for a one-hot one; 0 without a
    counted pixel.  Differentiable in ``zq``; the upsampled logits and their gradient never exist.  Returns (loss, acc)."""
    return _SoftCELowRes.apply(zq, (int(size[0]), int(size[1])), spx.contiguous(), _mask_u8(mask), bits, softw, live, invT, reduce_acc)


def simw_plbl_reference(size, spx, mask, targets=None, bits=None, zq_p=None, featq=None, invT=1.0, inv_tau=1.0, softw=None, live=None,
                        zq=None, invT_ce=None, grad=None):
    """``online_soft_weights`` and ``soft_ce_lowres`` on HOST tensors: the library's plain loop through csrc/online_plbl.h
    (``mas_simw_plbl_reference``).  Needs no GPU.  With ``zq_p`` / ``featq`` the soft weights and the live flags are computed (entries
    that are not defined stay NaN), otherwise they are the given ``softw`` [N,C,H,W] / ``live`` int32 [N].  Returns a dict: softw, live,
    and with ``zq``: loss f32 [1], acc i64 [2], and with ``grad`` (f32 [1]) dzq_fix."""
    lib = _lib.load()
    for t in (zq_p, featq, spx, mask, zq, grad, softw, live, bits, targets):
        if t is not None and (t.is_cuda or not t.is_contiguous()):
            raise ValueError("simw_plbl_reference takes contiguous host tensors")
    src = zq_p if zq_p is not None else zq
    N, C, h, w = src.shape
    H, W = int(size[0]), int(size[1])
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    bits = _plbl_bits_host(targets, bits)
    S, Ch = bits.shape[1], 1
    if zq_p is not None:
        _plbl_shapes(zq_p, featq, size, spx, mask, bits)
        Ch = featq.shape[1]
        softw = torch.full((N, C, H, W), float('nan'), dtype=torch.float32)
        live = torch.zeros(N, dtype=torch.int32)
    acc = loss = fix = None
    if zq is not None:
        _soft_ce_check(zq, size, spx, mask, bits, softw, live)
        acc, loss = torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.float32)
        fix = torch.zeros(zq.shape, dtype=torch.int64) if grad is not None else None
    _lib.check(lib.mas_simw_plbl_reference(_opt(zq_p), _opt(featq), Ch, h, w, spx.data_ptr(), _id_code(spx), mask.data_ptr(), bits.data_ptr(),
                                           N, C, H, W, S, invT, inv_tau, softw.data_ptr(), live.data_ptr(), _opt(zq),
                                           invT if invT_ce is None else invT_ce, _opt(grad), _opt(acc), _opt(loss), _opt(fix)),
               "mas_simw_plbl_reference")
    out = dict(softw=softw, live=live, bits=bits)
    if zq is not None:
        out.update(loss=loss, acc=acc)
        if fix is not None:
            out['dzq_fix'] = fix
    return out


def _plbl_bits_host(targets, bits):
    """``target_bits`` on the host (the reference function has no device to run the kernel on)."""
    if (targets is None) == (bits is None):
        raise ValueError("give either targets (u8 [N,S,cols]) or bits (int32 [N,S])")
    if bits is not None:
        return bits
    cols = targets.shape[-1]
    if cols > _lib.MAX_CLASSES:
        raise ValueError("at most %d target columns" % _lib.MAX_CLASSES)
    v = ((targets != 0).to(torch.int64) << torch.arange(cols, dtype=torch.int64)).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).contiguous()           # (bit 31 set: the same 32 bits as int32)


# ------------------------------------------------------------------------------------------------
# K4: ordering + budgeted selection walk
# ------------------------------------------------------------------------------------------------
def path_ranks(paths):
    """Rank of every image's joined path string in ascending (Python ``str``) order -- the tie-break
    the reference's tuple sort applies after the score (``active_selection/base.py:37``).
    Returns (img_rank[n], img_of_rank[n]) as int32 numpy arrays."""
    order = sorted(range(len(paths)), key=lambda i: paths[i])
    img_of_rank = np.asarray(order, dtype=np.int32)
    img_rank = np.empty(len(paths), dtype=np.int32)
    img_rank[img_of_rank] = np.arange(len(paths), dtype=np.int32)
    return img_rank, img_of_rank


def region_keys(scores, valid, img_rank):
    """64-bit sort keys [n_img*S] (int64 bits of uint64) for scores [n_img,S] f32."""
    _need(scores, "scores", torch.float32)
    _need(img_rank, "img_rank", torch.int32)
    n_img, S = scores.shape
    if valid is not None:
        valid = _mask_u8(valid)
        if tuple(valid.shape) != (n_img, S):
            raise ValueError("valid must be [n_img, S]")
    keys = torch.empty(n_img * S, dtype=torch.int64, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.load().mas_region_keys(scores.data_ptr(), valid.data_ptr() if valid is not None else None,
                                               img_rank.data_ptr(), n_img, S, keys.data_ptr(), _stream(scores)),
                   "mas_region_keys")
    return keys


def sort_keys_desc(keys):
    _need(keys, "keys", torch.int64)
    n = keys.numel()
    lib = _lib.load()
    ws = torch.empty(lib.mas_select_workspace_bytes(n), dtype=torch.uint8, device=keys.device)
    out = torch.empty_like(keys)
    with torch.cuda.device(keys.device):
        _lib.check(lib.mas_sort_keys_desc(keys.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(keys)),
                   "mas_sort_keys_desc")
    return out


def budget_walk(sorted_keys, region_cost, img_of_rank, S, budget, max_out=None):
    """Returns (n_selected int64[1] on device, sel_img i32[max_out], sel_id i32[max_out], sel_score f32[max_out]).
    ``region_cost`` u8 [n_img*S] (``multi_hot_cls[img, id].sum()``) or None for unit cost."""
    _need(sorted_keys, "sorted_keys", torch.int64)
    _need(img_of_rank, "img_of_rank", torch.int32)
    cost_bits = region_cost
    if cost_bits is not None:
        _need(cost_bits, "region_cost", torch.uint8)
    n = sorted_keys.numel()
    # every region costs >= 1 when costs are popcounts of non-empty rows; budget+1 outputs always suffice then
    max_out = n if max_out is None else min(n, max_out)
    dev = sorted_keys.device
    lib = _lib.load()
    ws = torch.empty(lib.mas_select_workspace_bytes(n), dtype=torch.uint8, device=dev)
    nsel = torch.empty(1, dtype=torch.int64, device=dev)
    sel_img = torch.empty(max_out, dtype=torch.int32, device=dev)
    sel_id = torch.empty(max_out, dtype=torch.int32, device=dev)
    sel_score = torch.empty(max_out, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mas_budget_walk(sorted_keys.data_ptr(), n, cost_bits.data_ptr() if cost_bits is not None else None,
                                       img_of_rank.data_ptr(), S, int(budget), max_out, nsel.data_ptr(), sel_img.data_ptr(),
                                       sel_id.data_ptr(), sel_score.data_ptr(), ws.data_ptr(), ws.numel(), _stream(sorted_keys)),
                   "mas_budget_walk")
    return nsel, sel_img, sel_id, sel_score


def minmax_normalize_(scores):
    """In place: (u - min(u[u != 0])) / max(...) over all region scores -- my_bvsb.py:79-81."""
    _need(scores, "scores", torch.float32)
    scratch = torch.empty(2, dtype=torch.int32, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.load().mas_minmax_normalize(scores.data_ptr(), scores.numel(), scratch.data_ptr(), _stream(scores)),
                   "mas_minmax_normalize")
    return scores


# ------------------------------------------------------------------------------------------------
# mIoU counters
# ------------------------------------------------------------------------------------------------
def iou_counts(outputs, outputs_all, targets, num_classes, ignore_label, counts=None):
    """Accumulate seen/correct/positive (+ the 3 "undefined"-class counters) into ``counts`` int64[3C+3].
    Reference: utils/miou.py:23-38, utils/miou_evalignore.py:20-32."""
    _need(targets, "targets", torch.int64)
    if outputs is not None:
        _need(outputs, "outputs", torch.int64)
    if outputs_all is not None:
        _need(outputs_all, "outputs_all", torch.int64)
    if counts is None:
        counts = torch.zeros(3 * num_classes + 3, dtype=torch.int64, device=targets.device)
    with torch.cuda.device(targets.device):
        _lib.check(_lib.load().mas_iou_counts(outputs.data_ptr() if outputs is not None else None,
                                              outputs_all.data_ptr() if outputs_all is not None else None,
                                              targets.data_ptr(), targets.numel(), num_classes, int(ignore_label),
                                              counts.data_ptr(), _stream(targets)), "mas_iou_counts")
    return counts


def logits_iou_counts(z, targets, num_classes, ignore_label, counts=None):
    """Fused argmax + counters from logits [B,channels,H,W] (channels = num_classes or num_classes+1)."""
    _need(z, "logits", torch.float32)
    _need(targets, "targets", torch.int64)
    B, CH, H, W = z.shape
    if tuple(targets.shape) != (B, H, W):
        raise ValueError("targets %s do not match logits %s" % (tuple(targets.shape), tuple(z.shape)))
    if counts is None:
        counts = torch.zeros(3 * num_classes + 3, dtype=torch.int64, device=z.device)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().mas_logits_iou_counts(z.data_ptr(), targets.data_ptr(), B, CH, H, W, num_classes,
                                                     int(ignore_label), counts.data_ptr(), _stream(z)), "mas_logits_iou_counts")
    return counts


def lowres_iou_supported(z_q, size):
    """The geometries ``mas_lowres_iou_counts`` takes for quarter-resolution logits ``z_q`` [B,CH,h,w] and an output ``size`` (H, W):
    those of ``naive_plbl_supported`` (the identity, or h <= H, w <= W, W <= 6 w, H <= 65535), on a GPU tensor."""
    return z_q.is_cuda and naive_plbl_supported(z_q, size)


def lowres_iou_counts(z_q, targets, size, num_classes, ignore_label, counts=None):
    """``logits_iou_counts`` of the bilinear upsampling of quarter-resolution logits ``z_q`` f32 [B,channels,h,w] to ``size`` = (H, W),
    without materialising it (``csrc/lowres_iou.hip``): the counters equal
    ``logits_iou_counts(upsample_bilinear(z_q, size), targets, ...)`` element for element.  targets int64 [B,H,W].  A geometry
    ``lowres_iou_supported`` declines and CPU tensors raise: there is no fall-back."""
    _need(z_q, "z_q", torch.float32)
    _need(targets, "targets", torch.int64)
    H, W = int(size[0]), int(size[1])
    if z_q.dim() != 4:
        raise ValueError("z_q must be [B,channels,h,w], got %s" % (tuple(z_q.shape),))
    B, CH, h, w = z_q.shape
    if tuple(targets.shape) != (B, H, W):
        raise ValueError("targets %s do not match %d pictures of %dx%d" % (tuple(targets.shape), B, H, W))
    if not lowres_iou_supported(z_q, (H, W)):
        raise ValueError("lowres_iou_counts: logits %s cannot be upsampled to %dx%d (an upsampling with W <= 6 w, or the identity)"
                         % (tuple(z_q.shape), H, W))
    if counts is None:
        counts = torch.zeros(3 * num_classes + 3, dtype=torch.int64, device=z_q.device)
    with torch.cuda.device(z_q.device):
        _lib.check(_lib.load().mas_lowres_iou_counts(z_q.data_ptr(), targets.data_ptr(), B, CH, h, w, H, W, num_classes,
                                                     int(ignore_label), counts.data_ptr(), _stream(z_q)), "mas_lowres_iou_counts")
    return counts


def render_labels(labels, palette, fill, superpixels=None):
    """Colour image u8 ``[N,H,W,3]`` of the label maps ``labels`` (int64 or uint8 ``[N,H,W]``) -- the ``--save_vis`` images of the
    stage-2 generators and the ``eval_naive_vis`` pictures (``csrc/render.hip``).  ``palette`` u8 ``[P,3]`` on the GPU (P <= 256), label
    255 painted as ``fill``.  Without ``superpixels``: ``palette[label]``.  With ``superpixels`` (int64 ``[N,H,W]``): the reference's
    ``mark_boundaries(colours, superpixels) * 255`` cast to uint8 (outer boundaries in (255, 255, 0), the other bytes through
    skimage's float64 round trip).  A label outside the palette after the fill raises
    ``MulActSegHipError`` (counted on the device; reading the count waits for this stream).  CPU tensors raise: there is no
    fall-back."""
    _need(labels, "labels")
    _need(palette, "palette", torch.uint8)
    if labels.dtype not in (torch.int64, torch.uint8):
        raise TypeError("labels must be torch.int64 or torch.uint8, got %s" % labels.dtype)
    if labels.dim() != 3:
        raise ValueError("labels must be [N,H,W], got %s" % (tuple(labels.shape),))
    if palette.dim() != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256:
        raise ValueError("palette must be [P,3] with 1 <= P <= 256, got %s" % (tuple(palette.shape),))
    P = int(palette.shape[0])
    if not 0 <= int(fill) < P:
        raise ValueError("fill %d is not an index of the %d-colour palette" % (int(fill), P))
    N, H, W = labels.shape
    if superpixels is not None:
        _need(superpixels, "superpixels", torch.int64)
        if tuple(superpixels.shape) != (N, H, W):
            raise ValueError("superpixels %s do not match labels %s" % (tuple(superpixels.shape), tuple(labels.shape)))
    rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=labels.device)
    bad = torch.zeros(1, dtype=torch.int32, device=labels.device)
    dt = _lib.ID_I64 if labels.dtype == torch.int64 else _lib.MAP_U8
    with torch.cuda.device(labels.device):
        _lib.check(_lib.load().mas_render_labels(labels.data_ptr(), dt, N, H, W, palette.data_ptr(), P, int(fill),
                                                 None if superpixels is None else superpixels.data_ptr(), int(superpixels is not None),
                                                 rgb.data_ptr(), bad.data_ptr(), _stream(labels)), "mas_render_labels")
    n_bad = int(bad.item())
    if n_bad:
        raise _lib.MulActSegHipError("render_labels: %d label(s) outside the %d-colour palette after filling 255 with %d"
                                     % (n_bad, P, int(fill)))
    return rgb


def render_lowres_pred(z_q, size, palette):
    """Colour image u8 ``[N,H,W,3]`` of ``palette[first arg-max over channels 0..CH-2 of upsample_bilinear(z_q, size)]`` --
    ``decode_target(preds[:, :-1].max(1)[1])`` of ``eval_naive_vis`` from the quarter-resolution logits ``z_q`` f32 ``[N,CH,h,w]``,
    equal to ``palette[torch.max(ops.upsample_bilinear(z_q, size)[:, :-1], 1)[1]]`` (first maximum, first NaN) without the
    full-resolution logits.  Geometries: those of ``naive_plbl_supported``; ``palette`` u8 ``[P,3]`` with CH - 1 <= P <= 256.  CPU
    tensors raise: there is no fall-back."""
    _need(z_q, "z_q", torch.float32)
    _need(palette, "palette", torch.uint8)
    H, W = int(size[0]), int(size[1])
    if z_q.dim() != 4:
        raise ValueError("z_q must be [N,CH,h,w], got %s" % (tuple(z_q.shape),))
    N, CH, h, w = z_q.shape
    if not naive_plbl_supported(z_q, (H, W)):
        raise ValueError("render_lowres_pred: logits %s cannot be upsampled to %dx%d (an upsampling with W <= 6 w, or the identity)"
                         % (tuple(z_q.shape), H, W))
    if palette.dim() != 2 or palette.shape[1] != 3 or not CH - 1 <= palette.shape[0] <= 256:
        raise ValueError("palette must be [P,3] with %d <= P <= 256, got %s" % (CH - 1, tuple(palette.shape)))
    rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=z_q.device)
    work = torch.empty((N + 1) * H * W, dtype=torch.uint8, device=z_q.device)
    with torch.cuda.device(z_q.device):
        _lib.check(_lib.load().mas_render_lowres_pred(z_q.data_ptr(), N, CH, h, w, H, W, palette.data_ptr(), int(palette.shape[0]),
                                                      work.data_ptr(), rgb.data_ptr(), _stream(z_q)), "mas_render_lowres_pred")
    return rgb


# ------------------------------------------------------------------------------------------------
# single-pass acquisition scan
# ------------------------------------------------------------------------------------------------
def weights_to_fixed31(cls_w):
    """floor(w * 2^31) as int32-viewed uint32 (host, exact): the integer class weights of the single-pass
    finalize.  ``cls_w``: float32 numpy array or None (-> all ones)."""
    w = np.asarray(cls_w, dtype=np.float32).astype(np.float64)
    return np.floor(w * 2147483648.0).astype(np.uint32)


def class_weight(prob_sum, hw, batch_size, n_batches, coeff):
    """Device-side class weights from the per-picture class sums [n_img, C] int64 (``mas_class_weight``): returns
    (cum f64 [C], cls_w f32 [C], w31 int32 [C] = floor(cls_w * 2^31) bits).  No host synchronisation."""
    _need(prob_sum, "prob_sum", torch.int64)
    n_img, C = prob_sum.shape
    dev = prob_sum.device
    cum = torch.empty(C, dtype=torch.float64, device=dev)
    w = torch.empty(C, dtype=torch.float32, device=dev)
    w31 = torch.empty(C, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_class_weight(prob_sum.data_ptr(), n_img, C, int(hw), int(batch_size), int(n_batches),
                                                float(coeff), cum.data_ptr(), w.data_ptr(), w31.data_ptr(), _stream(prob_sum)),
                   "mas_class_weight")
    return cum, w, w31


def single_pass_accum(z, spx, S, invT, prob_sum=None, class_sum=None, hist=None):
    """One scan: (prob_sum [B,C] i64, class_sum [B,S,C] i64, hist [B,S,C] i32), all accumulated into."""
    _need(z, "z", torch.float32)
    _need(spx, "spx")
    B, C, H, W = z.shape
    if tuple(spx.shape) != (B, H, W):
        raise ValueError("spx shape %s does not match logits %s" % (tuple(spx.shape), tuple(z.shape)))
    dev = z.device
    if prob_sum is None:
        prob_sum = torch.zeros((B, C), dtype=torch.int64, device=dev)
    if class_sum is None:
        class_sum = torch.zeros((B, S, C), dtype=torch.int64, device=dev)
    if hist is None:
        hist = torch.zeros((B, S, C), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_single_pass_accum(z.data_ptr(), spx.data_ptr(), _id_code(spx), B, C, H, W, S, invT,
                                                     prob_sum.data_ptr(), class_sum.data_ptr(), hist.data_ptr(), _stream(z)),
                   "mas_single_pass_accum")
    return prob_sum, class_sum, hist


def single_pass_accum_lowres(zq, size, spx, S, invT, prob_sum=None, class_sum=None, hist=None, generic=False):
    """``single_pass_accum`` of ``F.interpolate(zq, size, 'bilinear', align_corners=False)`` without materialising it: ``zq``
    [B,C,h,w] quarter-resolution logits, ``spx`` [B,H,W]; same outputs, bit for bit.  ``generic`` (tests / A-B measurements): keep
    the generic tap reads at the exact x4 ratio too (a per-call flag; the results are bit-identical either way)."""
    _need(zq, "zq", torch.float32)
    _need(spx, "spx")
    B, C, h, w = zq.shape
    H, W = int(size[0]), int(size[1])
    if tuple(spx.shape) != (B, H, W):
        raise ValueError("spx shape %s does not match logits %s at size %s" % (tuple(spx.shape), tuple(zq.shape), (H, W)))
    dev = zq.device
    if prob_sum is None:
        prob_sum = torch.zeros((B, C), dtype=torch.int64, device=dev)
    if class_sum is None:
        class_sum = torch.zeros((B, S, C), dtype=torch.int64, device=dev)
    if hist is None:
        hist = torch.zeros((B, S, C), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_single_pass_accum_lowres_opt(zq.data_ptr(), h, w, spx.data_ptr(), _id_code(spx), B, C, H, W, S, invT,
                                                                prob_sum.data_ptr(), class_sum.data_ptr(), hist.data_ptr(),
                                                                _lib.LOWRES_GENERIC if generic else 0, _stream(zq)),
                   "mas_single_pass_accum_lowres_opt")
    return prob_sum, class_sum, hist


UNCERTAINTY = {'bvsb': 0, 'margin': 1, 'least_confidence': 2, 'entropy': 3}       # MAS_UNC_* of include/mulactseg_hip.h


def _measure_code(measure):
    try:
        return UNCERTAINTY[measure]
    except KeyError:
        raise ValueError("unknown uncertainty measure %r (one of %s)" % (measure, ', '.join(UNCERTAINTY)))


def _uncertainty_buffers(B, C, S, dev, prob_sum, class_sum, hist):
    if prob_sum is None:
        prob_sum = torch.zeros((B, C), dtype=torch.int64, device=dev)
    if class_sum is None:
        class_sum = torch.zeros((B, S, C), dtype=torch.int64, device=dev)
    if hist is None:
        hist = torch.zeros((B, S, C), dtype=torch.int32, device=dev)
    return prob_sum, class_sum, hist


def uncertainty_accum(z, spx, S, invT, measure, prob_sum=None, class_sum=None, hist=None):
    """``single_pass_accum`` with the per-pixel value of ``measure`` (a key of ``UNCERTAINTY``; csrc/uncertainty.h) in place of the
    BvSB margin: (prob_sum [B,C] i64, class_sum [B,S,C] i64, hist [B,S,C] i32), all accumulated into.  2 <= C <= 32."""
    code = _measure_code(measure)
    _need(z, "z", torch.float32)
    _need(spx, "spx")
    B, C, H, W = z.shape
    if tuple(spx.shape) != (B, H, W):
        raise ValueError("spx shape %s does not match logits %s" % (tuple(spx.shape), tuple(z.shape)))
    prob_sum, class_sum, hist = _uncertainty_buffers(B, C, S, z.device, prob_sum, class_sum, hist)
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().mas_uncertainty_accum(z.data_ptr(), spx.data_ptr(), _id_code(spx), B, C, H, W, S, invT, code,
                                                     prob_sum.data_ptr(), class_sum.data_ptr(), hist.data_ptr(), _stream(z)),
                   "mas_uncertainty_accum")
    return prob_sum, class_sum, hist


def uncertainty_accum_lowres(zq, size, spx, S, invT, measure, prob_sum=None, class_sum=None, hist=None):
    """``uncertainty_accum`` of ``F.interpolate(zq, size, 'bilinear', align_corners=False)`` without materialising it: ``zq``
    [B,C,h,w], ``spx`` [B,H,W]; same outputs, bit for bit.  A geometry outside the identity / an upsampling of at most x6 along the rows
    is refused ("argument out of range") before anything is launched."""
    code = _measure_code(measure)
    _need(zq, "zq", torch.float32)
    _need(spx, "spx")
    B, C, h, w = zq.shape
    H, W = int(size[0]), int(size[1])
    if tuple(spx.shape) != (B, H, W):
        raise ValueError("spx shape %s does not match logits %s at size %s" % (tuple(spx.shape), tuple(zq.shape), (H, W)))
    prob_sum, class_sum, hist = _uncertainty_buffers(B, C, S, zq.device, prob_sum, class_sum, hist)
    with torch.cuda.device(zq.device):
        _lib.check(_lib.load().mas_uncertainty_accum_lowres(zq.data_ptr(), h, w, spx.data_ptr(), _id_code(spx), B, C, H, W, S, invT, code,
                                                            prob_sum.data_ptr(), class_sum.data_ptr(), hist.data_ptr(), _stream(zq)),
                   "mas_uncertainty_accum_lowres")
    return prob_sum, class_sum, hist


def uncertainty_reference(z, spx, S, invT, measure, prob_sum=None, class_sum=None, hist=None):
    """``uncertainty_accum`` on HOST tensors: the library's plain loop over the pixels through csrc/uncertainty.h
    (``mas_uncertainty_reference``), the CPU-side statement of the arithmetic the kernel is checked against.  Needs no GPU."""
    code = _measure_code(measure)
    for t, name in ((z, "z"), (spx, "spx"), (prob_sum, "prob_sum"), (class_sum, "class_sum"), (hist, "hist")):
        if t is not None and (t.is_cuda or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous host tensor" % name)
    if z.dtype != torch.float32:
        raise TypeError("z must be float32, got %s" % z.dtype)
    B, C, H, W = z.shape
    if tuple(spx.shape) != (B, H, W):
        raise ValueError("spx shape %s does not match logits %s" % (tuple(spx.shape), tuple(z.shape)))
    prob_sum, class_sum, hist = _uncertainty_buffers(B, C, S, z.device, prob_sum, class_sum, hist)
    _lib.check(_lib.load().mas_uncertainty_reference(z.data_ptr(), spx.data_ptr(), _id_code(spx), B, C, H, W, S, invT, code,
                                                     prob_sum.data_ptr(), class_sum.data_ptr(), hist.data_ptr()),
               "mas_uncertainty_reference")
    return prob_sum, class_sum, hist


def region_finalize_weighted(class_sum, hist, w31, ban_class=-1, want_hist_i64=False):
    """Weighted mean per region from the single-pass accumulators.  ``w31``: int32 tensor [C] holding uint32 bits."""
    _need(class_sum, "class_sum", torch.int64)
    _need(hist, "hist", torch.int32)
    _need(w31, "w31", torch.int32)
    C = hist.shape[-1]
    shape = hist.shape[:-1]
    n = hist.numel() // C
    dev = hist.device
    score = torch.empty(shape, dtype=torch.float32, device=dev)
    dom = torch.empty(shape, dtype=torch.int32, device=dev)
    cnt = torch.empty(shape, dtype=torch.int32, device=dev)
    h64 = torch.empty(hist.shape, dtype=torch.int64, device=dev) if want_hist_i64 else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_region_finalize_weighted(
            class_sum.data_ptr(), hist.data_ptr(), n, C, w31.data_ptr(), ban_class, score.data_ptr(), dom.data_ptr(),
            cnt.data_ptr(), h64.data_ptr() if h64 is not None else None, _stream(hist)), "mas_region_finalize_weighted")
    return score, dom, cnt, h64


def region_reweight_(scores, dominant, ban_class=-1, cls_w=None):
    """In place: zero the regions whose dominant class is ``ban_class`` and multiply by ``cls_w[dominant]``
    (my_bvsb_banignore.py:58-61, my_bvsb_clsbal_v2_banignore.py:60-74)."""
    _need(scores, "scores", torch.float32)
    _need(dominant, "dominant", torch.int32)
    if cls_w is not None:
        _need(cls_w, "cls_w", torch.float32)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.load().mas_region_reweight(scores.data_ptr(), dominant.data_ptr(), scores.numel(), ban_class,
                                                   cls_w.data_ptr() if cls_w is not None else None, _stream(scores)),
                   "mas_region_reweight")
    return scores


def dominant_hist(dominant, C):
    """int64[C]: number of regions per dominant class."""
    _need(dominant, "dominant", torch.int32)
    counts = torch.zeros(C, dtype=torch.int64, device=dominant.device)
    with torch.cuda.device(dominant.device):
        _lib.check(_lib.load().mas_dominant_hist(dominant.data_ptr(), dominant.numel(), C, counts.data_ptr(), _stream(dominant)),
                   "mas_dominant_hist")
    return counts


# ------------------------------------------------------------------------------------------------
# Region labels of the data-generation step (csrc/labels.hip): multi-hot rows and dominant-label maps
# ------------------------------------------------------------------------------------------------
MAX_TRIM_KERNEL = 15


def trim_kernel(trim_kernel_size):
    """``None`` / 0 -> 0 (no trimming); odd 1..15 -> itself; anything else is an argument error."""
    k = int(trim_kernel_size or 0)
    if k and (k < 0 or k > MAX_TRIM_KERNEL or k % 2 == 0):
        raise ValueError("trim kernel size must be odd and in 1..%d, got %d" % (MAX_TRIM_KERNEL, k))
    return k


def _label_picture(labels, superpixel, nseg, num_classes):
    _need(labels, "labels", torch.uint8)
    _need(superpixel, "superpixel")
    code = _id_code(superpixel)
    if labels.dim() != 2 or tuple(superpixel.shape) != tuple(labels.shape):
        raise ValueError("labels and superpixel must be [H,W] of one shape, got %s and %s"
                         % (tuple(labels.shape), tuple(superpixel.shape)))
    if nseg < 1:
        raise ValueError("nseg must be positive")
    if not 1 <= num_classes < _lib.MAX_CLASSES:
        raise ValueError("num_classes + 1 must be in 2..%d, got %d" % (_lib.MAX_CLASSES, num_classes + 1))
    return code


def listed_ids(ids, nseg, device):
    """uint8 [nseg] on ``device``: 1 for the ids of the region dict's list (ids outside [0, nseg) are an argument error)."""
    a = np.asarray(ids, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() >= nseg):
        raise ValueError("listed superpixel ids must be in [0, %d)" % nseg)
    lut = np.zeros(nseg, dtype=np.uint8)
    lut[a] = 1
    return torch.from_numpy(lut).to(device)


def _raise_on_label_status(status, num_classes):
    if int(status.item()) & _lib.LABELS_BAD_VALUE:
        raise ValueError("label map holds values outside [0, %d) and 255" % num_classes)


def _label_counts(labels, superpixel, nseg, num_classes, k):
    code = _label_picture(labels, superpixel, nseg, num_classes)
    H, W = labels.shape
    dev = labels.device
    full = torch.empty((nseg, num_classes + 1), dtype=torch.int32, device=dev)
    trimmed = torch.empty_like(full) if k else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_region_label_counts(superpixel.data_ptr(), code, labels.data_ptr(), H, W, nseg, num_classes, k,
                                                       full.data_ptr(), trimmed.data_ptr() if k else None, status.data_ptr(),
                                                       _stream(labels)), "mas_region_label_counts")
    return full, trimmed, status


def region_label_counts(labels, superpixel, nseg, num_classes, trim_kernel_size=None):
    """(full, trimmed): int32 ``[nseg, num_classes + 1]`` label histograms per superpixel id (last column: label 255), over all
    pixels of the id and over those outside the dilated thick boundary (``None`` without trimming) --
    ``region_cityscapes_tensor.py:47-66``.  labels: uint8 [H,W]; superpixel: int64 / int32 / uint16 (int16) [H,W].  Reads back one
    status word (a label outside [0, C) and 255 is a ValueError)."""
    full, trimmed, status = _label_counts(labels, superpixel, nseg, num_classes, trim_kernel(trim_kernel_size))
    _raise_on_label_status(status, num_classes)
    return full, trimmed


def region_multi_hot(labels, superpixel, ids, nseg, num_classes, trim_kernel_size=None):
    """(bits uint8 ``[nseg, num_classes + 1]``, size int64 ``[nseg]``): the multi-hot rows of one picture --
    ``region_cityscapes_tensor.py:23-86``.  ``ids``: the listed superpixel ids (region dict), or a uint8 [nseg] device mask."""
    k = trim_kernel(trim_kernel_size)
    full, trimmed, status = _label_counts(labels, superpixel, nseg, num_classes, k)
    listed = ids if torch.is_tensor(ids) else listed_ids(ids, nseg, labels.device)
    _need(listed, "listed", torch.uint8)
    if listed.numel() != nseg:
        raise ValueError("listed must be uint8 [nseg]")
    bits = torch.empty((nseg, num_classes + 1), dtype=torch.uint8, device=labels.device)
    size = torch.empty(nseg, dtype=torch.int64, device=labels.device)
    with torch.cuda.device(labels.device):
        _lib.check(_lib.load().mas_region_multi_hot(full.data_ptr(), trimmed.data_ptr() if k else None, listed.data_ptr(), nseg,
                                                    num_classes, bits.data_ptr(), size.data_ptr(), _stream(labels)),
                   "mas_region_multi_hot")
    _raise_on_label_status(status, num_classes)
    return bits, size


def region_dominant(labels, superpixel, ids, nseg, num_classes, generate_ignore=False, draw=None):
    """uint8 [H,W]: the dominant-label map of one picture -- ``region_cityscapes_dominant_all.py:24-62``.  ``draw`` (the ``_sample``
    variant, ``region_cityscapes_dominant_all_sample.py``): a host callable ``full -> int32 [nseg]`` that receives the int32
    ``[nseg, num_classes + 1]`` counts as a numpy array and returns the drawn column per id (-1: none); it replaces the arg-max."""
    full, _, status = _label_counts(labels, superpixel, nseg, num_classes, 0)
    code = _id_code(superpixel)
    listed = ids if torch.is_tensor(ids) else listed_ids(ids, nseg, labels.device)
    _need(listed, "listed", torch.uint8)
    if listed.numel() != nseg:
        raise ValueError("listed must be uint8 [nseg]")
    drawn = None
    if draw is not None:
        _raise_on_label_status(status, num_classes)
        d = np.ascontiguousarray(draw(full.cpu().numpy()), dtype=np.int32)
        if d.shape != (nseg,) or d.min() < -1 or d.max() > num_classes:
            raise ValueError("draw() must return int32 [nseg] columns in -1..%d" % num_classes)
        drawn = torch.from_numpy(d).to(labels.device)
    H, W = labels.shape
    choice = torch.empty(nseg, dtype=torch.int32, device=labels.device)
    out = torch.empty_like(labels)
    gi = 1 if generate_ignore else 0
    with torch.cuda.device(labels.device):
        lib, st = _lib.load(), _stream(labels)
        _lib.check(lib.mas_region_dominant(full.data_ptr(), listed.data_ptr(), drawn.data_ptr() if drawn is not None else None, nseg,
                                           num_classes, gi, choice.data_ptr(), st), "mas_region_dominant")
        _lib.check(lib.mas_region_paint(superpixel.data_ptr(), code, labels.data_ptr(), H, W, nseg, choice.data_ptr(), gi,
                                        out.data_ptr(), st), "mas_region_paint")
    if draw is None:
        _raise_on_label_status(status, num_classes)
    return out


def spx_max_onehot(target, superpixel, nseg, num_classes=20):
    """(rows uint8 ``[nseg, num_classes]``, mask bool ``[H,W]``) of one picture -- the dominant-label stage-2 targets of
    ``trainer/eval_save_cosplbl_prop_onehotignore.py:29-33``: ``mask = target != 255``; per superpixel id the largest target value of
    its pixels (``torch_scatter.scatter_max``), 255 read as ``num_classes - 1``, one-hot.  An id with no pixel gets the row of 0 (the
    reference's table has ``max(id) + 1`` rows, this one ``nseg``: such rows carry no masked pixel and change no label).  target:
    uint8 or int64 [H,W]; superpixel: int64 / int32 / uint16 (int16) [H,W].  One pass (``csrc/labels.hip``); reads back one status
    word (a target value outside [0, num_classes) and 255 is a ValueError)."""
    _need(target, "target")
    _need(superpixel, "superpixel")
    if target.dtype not in (torch.uint8, torch.int64):
        raise TypeError("target must be uint8 or int64, got %s" % target.dtype)
    code = _id_code(superpixel)
    if target.dim() != 2 or tuple(superpixel.shape) != tuple(target.shape):
        raise ValueError("target and superpixel must be [H,W] of one shape, got %s and %s"
                         % (tuple(target.shape), tuple(superpixel.shape)))
    H, W = target.shape
    dev = target.device
    seg_max = torch.empty(nseg, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    rows = torch.empty((nseg, num_classes), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_spx_max_onehot(target.data_ptr(), _lib.MAP_U8 if target.dtype == torch.uint8 else _lib.ID_I64,
                                                  superpixel.data_ptr(), code, H, W, nseg, num_classes, seg_max.data_ptr(),
                                                  status.data_ptr(), mask.data_ptr(), rows.data_ptr(), _stream(target)),
                   "mas_spx_max_onehot")
    _raise_on_label_status(status, num_classes)
    return rows, mask.view(torch.bool)


# ------------------------------------------------------------------------------------------------
# K9: stage-2 cosine pseudo labels
# ------------------------------------------------------------------------------------------------
_STAGE2_METHODS = {'median': _lib.STAGE2_THR_MEDIAN, 'min': _lib.STAGE2_THR_MIN}
_STAGE2_THR_WS = {}


def stage2_threshold_method(method):
    """The ABI code of ``--cosprop_threshold_method``; anything but ``'median'`` / ``'min'`` is the reference's
    ``NotImplementedError`` (``trainer/eval_save_cosplbl_prop.py:253-254``)."""
    try:
        return _STAGE2_METHODS[method]
    except (KeyError, TypeError):
        raise NotImplementedError("cosprop_threshold_method must be 'median' or 'min', got %r" % (method,))


def _stage2_thresholds_aten(nn, nn_sim, n_proto, method):
    """``MAS_STAGE2_THRESHOLD=aten`` (A/B): the torch chain the kernels replaced -- a ``nonzero`` (host sync) and, for the median, two
    stable sorts by (prototype, similarity); an ``amin`` scatter for the minimum."""
    dev = nn.device
    thr = torch.ones(n_proto, dtype=torch.float32, device=dev)
    sel = (nn >= 0).nonzero().squeeze(1)
    if sel.numel():
        pid, sim = nn[sel].long(), nn_sim[sel]
        if method == 'min':
            return thr.scatter_reduce_(0, pid, sim, 'amin', include_self=False)
        order = torch.argsort(sim, stable=True)
        order = order[torch.argsort(pid[order], stable=True)]            # sorted by (prototype, similarity)
        pid_s, sim_s = pid[order], sim[order]
        cnt = torch.bincount(pid_s, minlength=n_proto)
        first = torch.cumsum(cnt, 0) - cnt
        has = cnt > 0
        thr[has] = sim_s[(first + (cnt - 1) // 2)[has]]
    return thr


def stage2_thresholds(nn, nn_sim, n_proto, method='median'):
    """float32 ``[n_proto]``: per prototype the lower median (``'median'``) or the minimum (``'min'``) of the similarities of the
    pixels assigned to it, 1.0 where there is none -- ``trainer/eval_save_cosplbl_prop.py:243-254``.  ``nn`` int32 / ``nn_sim``
    float32 ``[H*W]``: the outputs of ``mas_stage2_assign`` (``nn < 0``: the pixel takes no part).  One of the input values, picked
    by rank on the device (``csrc/stage2.hip``); ``MAS_STAGE2_THRESHOLD=aten`` runs the torch chain instead (A/B)."""
    code = stage2_threshold_method(method)
    _need(nn, "nn", torch.int32)
    _need(nn_sim, "nn_sim", torch.float32)
    if nn.numel() != nn_sim.numel() or nn.numel() == 0:
        raise ValueError("nn and nn_sim must hold one element per pixel, got %d and %d" % (nn.numel(), nn_sim.numel()))
    if os.environ.get("MAS_STAGE2_THRESHOLD", "kernel") == "aten":
        return _stage2_thresholds_aten(nn.reshape(-1), nn_sim.reshape(-1), n_proto, method)
    dev = nn.device
    with torch.cuda.device(dev):
        lib = _lib.load()
        nbytes = int(lib.mas_stage2_thresholds_scratch_bytes(n_proto, code))
        if nbytes < 0:
            _lib.check(nbytes, "mas_stage2_thresholds_scratch_bytes")
        ws = _stream_scratch(_STAGE2_THR_WS, dev, lambda: torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=dev), nbytes)
        thr = torch.empty(n_proto, dtype=torch.float32, device=dev)
        _lib.check(lib.mas_stage2_thresholds(nn.data_ptr(), nn_sim.data_ptr(), nn.numel(), n_proto, code, ws.data_ptr(), ws.numel(),
                                             thr.data_ptr(), _stream(nn)), "mas_stage2_thresholds")
    return thr


def stage2_pseudo_labels(feats, logits, targets, spmasks, superpixels, include_onehot=True, threshold_method='median', expand=True):
    """Pseudo-label maps int64 [N,H,W] (255 = none) -- trainer/eval_save_cosplbl_prop[_includeonehot].py:121-314.
    ``expand=False`` stops after the assignment (``trainer/eval_save_cosplbl.py:99-196``: no thresholds, no adjacency, no propagation):
    every selected pixel whose superpixel owns prototypes gets the class of its nearest one, everything else 255.

    feats [N,Ch,fh,fw]: the L2-normalised point features of ``feat_forward`` BEFORE the bilinear upsampling (full
    resolution is accepted too); logits [N,C,H,W]; targets u8 [N,S,C]; spmasks bool [N,H,W]; superpixels int64.
    ``threshold_method``: ``'median'`` or ``'min'`` (``--cosprop_threshold_method``, :243-254), ``NotImplementedError`` otherwise.
    The prototype list uses torch ops on the device; feature interpolation, similarities, the per-prototype
    thresholds, adjacency and propagation are HIP kernels."""
    stage2_threshold_method(threshold_method)
    _need(feats, "feats", torch.float32)
    _need(logits, "logits", torch.float32)
    _need(superpixels, "superpixels", torch.int64)
    mask = _mask_u8(spmasks)
    if targets.dtype != torch.uint8:
        targets = targets.to(torch.uint8)
    N, C, H, W = logits.shape
    Ch, fh, fw = feats.shape[1:]
    S = targets.shape[1]
    dev = logits.device
    lib = _lib.load()
    bits = target_bits(targets.contiguous())
    flags = _lib.LOSS_GROUP | (0 if include_onehot else _lib.LOSS_GROUP_ONLY_MULTI)
    out = torch.full((N, H, W), 255, dtype=torch.int64, device=dev)
    words = (S + 31) // 32
    with torch.cuda.device(dev):
        st = _stream(logits)
        for i in range(N):
            _, _, gmax = partial_loss_fwd(logits[i:i + 1], superpixels[i:i + 1], mask[i:i + 1], bits[i:i + 1], 1.0, flags)
            g = gmax[0]
            nz = (g != 0).nonzero()                              # ordered by (superpixel, class)
            n_proto = nz.shape[0]
            if n_proto == 0:
                continue
            proto_s, proto_c = nz[:, 0], nz[:, 1]
            proto_pix = (0xffffffff - (g[proto_s, proto_c] & 0xffffffff)).to(torch.int32)
            counts = torch.bincount(proto_s, minlength=S)
            p_start = torch.zeros(S + 1, dtype=torch.int32, device=dev)
            p_start[1:] = torch.cumsum(counts, 0).to(torch.int32)
            p_cls = proto_c.to(torch.int32).contiguous()
            P = torch.empty((n_proto, Ch), dtype=torch.float32, device=dev)
            f, sp, mk = feats[i], superpixels[i], mask[i]
            _lib.check(lib.mas_stage2_gather_protos(f.data_ptr(), Ch, fh, fw, H, W, proto_pix.data_ptr(), n_proto, P.data_ptr(), st),
                       "mas_stage2_gather_protos")
            nn = torch.empty(H * W, dtype=torch.int32, device=dev)
            nn_sim = torch.empty(H * W, dtype=torch.float32, device=dev)
            _lib.check(lib.mas_stage2_assign(f.data_ptr(), Ch, fh, fw, H, W, sp.data_ptr(), mk.data_ptr(), S, p_start.data_ptr(),
                                             P.data_ptr(), nn.data_ptr(), nn_sim.data_ptr(), st), "mas_stage2_assign")
            if not expand:
                _lib.check(lib.mas_stage2_assign_labels(nn.data_ptr(), p_cls.data_ptr(), H * W, out[i].data_ptr(), st),
                           "mas_stage2_assign_labels")
                continue
            thr = stage2_thresholds(nn, nn_sim, n_proto, threshold_method)
            adj = torch.zeros((S, words), dtype=torch.int32, device=dev)
            _lib.check(lib.mas_stage2_adjacency(sp.data_ptr(), H, W, S, p_start.data_ptr(), adj.data_ptr(), st), "mas_stage2_adjacency")
            _lib.check(lib.mas_stage2_propagate(f.data_ptr(), Ch, fh, fw, H, W, sp.data_ptr(), S, adj.data_ptr(), p_start.data_ptr(),
                                                p_cls.data_ptr(), P.data_ptr(), thr.data_ptr(), nn.data_ptr(), out[i].data_ptr(), st),
                       "mas_stage2_propagate")
    return out


# ------------------------------------------------------------------------------------------------
# K7: ASPP depthwise triple
# ------------------------------------------------------------------------------------------------
class _AsppDepthwise3(torch.autograd.Function):
    """(y6, y12, y18) = three dilated depthwise 3x3 convolutions of the same map, one read of x
    (models/segmentation/deeplabv3.py:174-177 x 3 branches)."""

    @staticmethod
    def forward(ctx, x, w0, w1, w2, d0, d1, d2):
        x = x.contiguous()
        w0, w1, w2 = w0.contiguous(), w1.contiguous(), w2.contiguous()
        N, C, H, W = x.shape
        ys = [torch.empty_like(x) for _ in range(3)]
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mas_aspp_dw3_fwd(x.data_ptr(), w0.data_ptr(), w1.data_ptr(), w2.data_ptr(), N, C, H, W, d0, d1, d2,
                                                    ys[0].data_ptr(), ys[1].data_ptr(), ys[2].data_ptr(), _stream(x)), "mas_aspp_dw3_fwd")
        ctx.save_for_backward(x, w0, w1, w2)
        ctx.dil = (d0, d1, d2)
        return tuple(ys)

    @staticmethod
    def backward(ctx, g0, g1, g2):
        x, w0, w1, w2 = ctx.saved_tensors
        d0, d1, d2 = ctx.dil
        N, C, H, W = x.shape
        g0, g1, g2 = g0.contiguous(), g1.contiguous(), g2.contiguous()
        lib = _lib.load()
        dx = dws = None
        with torch.cuda.device(x.device):
            st = _stream(x)
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                _lib.check(lib.mas_aspp_dw3_bwd_x(g0.data_ptr(), g1.data_ptr(), g2.data_ptr(), w0.data_ptr(), w1.data_ptr(), w2.data_ptr(),
                                                  N, C, H, W, d0, d1, d2, dx.data_ptr(), st), "mas_aspp_dw3_bwd_x")
            if any(ctx.needs_input_grad[1:4]):
                dws = [torch.empty_like(w0), torch.empty_like(w1), torch.empty_like(w2)]
                _lib.check(lib.mas_aspp_dw3_bwd_w(x.data_ptr(), g0.data_ptr(), g1.data_ptr(), g2.data_ptr(), N, C, H, W, d0, d1, d2,
                                                  dws[0].data_ptr(), dws[1].data_ptr(), dws[2].data_ptr(), st), "mas_aspp_dw3_bwd_w")
        dws = dws or [None, None, None]
        return dx, dws[0], dws[1], dws[2], None, None, None


def aspp_depthwise3(x, w0, w1, w2, dilations):
    _need(x, "x", torch.float32)
    for w in (w0, w1, w2):
        if tuple(w.shape) != (x.shape[1], 1, 3, 3):
            raise ValueError("depthwise weights must be [C,1,3,3]")
    return _AsppDepthwise3.apply(x, w0, w1, w2, int(dilations[0]), int(dilations[1]), int(dilations[2]))


class _Depthwise3x3(torch.autograd.Function):
    """y = depthwise 3x3 (stride 1, padding = dilation, no bias) of x (models/segmentation/deeplabv3.py:174-177)."""

    @staticmethod
    def forward(ctx, x, w, d):
        x, w = x.contiguous(), w.contiguous()
        N, C, H, W = x.shape
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mas_depthwise3x3_fwd(x.data_ptr(), w.data_ptr(), N, C, H, W, d, y.data_ptr(), _stream(x)),
                       "mas_depthwise3x3_fwd")
        ctx.save_for_backward(x, w)
        ctx.dil = d
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        d = ctx.dil
        N, C, H, W = x.shape
        g = g.contiguous()
        lib = _lib.load()
        dx = dw = None
        with torch.cuda.device(x.device):
            st = _stream(x)
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                _lib.check(lib.mas_depthwise3x3_bwd_x(g.data_ptr(), w.data_ptr(), N, C, H, W, d, dx.data_ptr(), st), "mas_depthwise3x3_bwd_x")
            if ctx.needs_input_grad[1]:
                dw = torch.empty_like(w)
                part = torch.empty((N, C, 9), dtype=torch.float32, device=x.device)
                _lib.check(lib.mas_depthwise3x3_bwd_w(x.data_ptr(), g.data_ptr(), N, C, H, W, d, part.data_ptr(), dw.data_ptr(), st),
                           "mas_depthwise3x3_bwd_w")
        return dx, dw, None


def depthwise3x3_supported(x, dilation):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and (16 + 2 * dilation) * (x.shape[3] + 2 * dilation) * 4 <= 64 * 1024


def depthwise3x3(x, w, dilation):
    _need(x, "x", torch.float32)
    if tuple(w.shape) != (x.shape[1], 1, 3, 3):
        raise ValueError("depthwise weight must be [C,1,3,3]")
    return _Depthwise3x3.apply(x, w, int(dilation))


class _UpsampleBilinear(torch.autograd.Function):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) with a deterministic gather backward."""

    @staticmethod
    def forward(ctx, x, Ho, Wo):
        x = x.contiguous()
        N, C, Hi, Wi = x.shape
        y = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mas_upsample_bilinear_fwd(x.data_ptr(), N * C, Hi, Wi, Ho, Wo, y.data_ptr(), _stream(x)),
                       "mas_upsample_bilinear_fwd")
        ctx.shape = (N, C, Hi, Wi, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, g):
        N, C, Hi, Wi, Ho, Wo = ctx.shape
        g = g.contiguous()
        gx = torch.empty((N, C, Hi, Wi), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().mas_upsample_bilinear_bwd(g.data_ptr(), N * C, Hi, Wi, Ho, Wo, gx.data_ptr(), _stream(g)),
                       "mas_upsample_bilinear_bwd")
        return gx, None, None


def upsample_bilinear_supported(x, size):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and int(size[1]) <= 6 * x.shape[3] and int(size[0]) >= x.shape[2]
            and int(size[1]) >= x.shape[3] and x.shape[0] * x.shape[1] <= 65535 and int(size[0]) <= 65535)


def upsample_bilinear(x, size):
    _need(x, "x", torch.float32)
    return _UpsampleBilinear.apply(x, int(size[0]), int(size[1]))


def upsample_bilinear_into(x, out):
    """Inference only: write the upsampling of x [N,C,hi,wi] into ``out`` [N,C,Ho,Wo], a view whose per-picture [C,Ho,Wo]
    blocks are contiguous (e.g. a channel slice of a concatenation buffer) -- one launch per picture, no copy afterwards."""
    _need(x, "x", torch.float32)
    N, C, Hi, Wi = x.shape
    Ho, Wo = out.shape[2], out.shape[3]
    if out.shape[0] != N or out.shape[1] != C or out.stride(3) != 1 or out.stride(2) != Wo or out.stride(1) != Ho * Wo:
        raise ValueError("out must be [N,C,Ho,Wo] with contiguous per-picture blocks")
    lib = _lib.load()
    with torch.cuda.device(x.device):
        for n in range(N):
            _lib.check(lib.mas_upsample_bilinear_fwd(x[n].data_ptr(), C, Hi, Wi, Ho, Wo, out[n].data_ptr(), _stream(x)),
                       "mas_upsample_bilinear_fwd")
    return out


def quarter_size(n):
    """The side the network emits at quarter resolution for an input side n: the stride-2 stem convolution and the stride-2
    max-pool (both padding 1, kernel 3) each give (n - 1) // 2 + 1."""
    return ((int(n) - 1) // 2) // 2 + 1


def ms_ensemble(feats_q, logits_q, scaled_sizes, flips, out_size):
    """The multi-scale + flip ensemble of the VOC stage-2 generator (trainer/eval_save_cosplbl_prop_includeonehot_voc_ms.py:56-79) in
    one launch (csrc/ms_ensemble.hip): n <= 16 sources, each the quarter-resolution ``(feat [1,Ch,hq,wq], logits [1,C,hq,wq])`` of the
    network on a picture scaled to ``scaled_sizes[k] = (Hs, Ws)`` and flipped horizontally when ``flips[k]``.  -> (features
    [1,Ch,H,W] unit-norm per pixel, logits [1,C,H,W]) at ``out_size = (H, W)``: upsampled x4 to the scaled size, flipped back, resized
    to (H, W), averaged; the features re-normalised over the channels.  The scaled-size maps never exist in memory."""
    n, dev, C, geom, H, W = _ms_sources("ms_ensemble", logits_q, scaled_sizes, flips, out_size, feats_q)
    Ch = int(feats_q[0].shape[1])
    g, fp, lp = _ms_pack(geom, feats_q=feats_q, logits_q=logits_q)
    feat = torch.empty((1, Ch, H, W), dtype=torch.float32, device=dev)
    logit = torch.empty((1, C, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_ms_ensemble(fp, lp, g, n, Ch, C, H, W, feat.data_ptr(), logit.data_ptr(), _stream(feat)),
                   "mas_ms_ensemble")
    return feat, logit


def naive_plbl_supported(logits_q, size):
    """The geometries ``mas_naive_plbl`` takes: the identity, or what ``upsample_bilinear_supported`` takes."""
    H, W = int(size[0]), int(size[1])
    if logits_q.dim() != 4:
        return False
    if (H, W) == tuple(logits_q.shape[2:]):
        return True
    h, w = int(logits_q.shape[2]), int(logits_q.shape[3])
    return h <= H and w <= W and W <= 6 * w and H <= 65535


def _naive_plbl_aten(logits_q, size, spmask, th):
    """The reference's lines (``eval_save_naiveplbl.py:52-56``) on the upsampled logits: ``F.interpolate``, ``softmax`` / ``max``,
    ``masked_fill``."""
    import torch.nn.functional as F
    H, W = int(size[0]), int(size[1])
    z = logits_q if tuple(logits_q.shape[2:]) == (H, W) else F.interpolate(logits_q, size=(H, W), mode='bilinear', align_corners=False)
    if th > 0:
        spmask = torch.softmax(z, dim=1).max(dim=1)[0] > th
    label = z.max(dim=1)[1]
    return torch.masked_fill(label, torch.logical_not(spmask), 255)


def naive_pseudo_labels(logits_q, size, spmask, th=0.0):
    """Naive top-1 pseudo labels int64 ``[N,H,W]`` (255 = none) -- ``trainer/eval_save_naiveplbl.py:46-61``.  logits_q f32
    ``[N,C,h,w]``: the network's quarter-resolution logits (``net(x, lowres=True)``), or full-resolution ones (h, w = H, W).  Label =
    the first arg-max over the C channels of the bilinear upsampling to ``size`` (bit for bit that of ``upsample_bilinear``);
    ``th <= 0``: kept where ``spmask`` (bool [N,H,W]); ``th > 0``: kept where ``1 / sum_c exp(y_c - y_max) > th`` over every pixel
    (``spmask`` unused; not bit-equal to ``torch.softmax``).  One launch (``csrc/naive_plbl.hip``): the full-resolution logits never
    exist.  CPU tensors, and ``MAS_NAIVE_PLBL=aten``, take the reference's ATen chain."""
    H, W = int(size[0]), int(size[1])
    th = float(th)
    if not logits_q.is_cuda or os.environ.get("MAS_NAIVE_PLBL", "fused") == "aten":
        return _naive_plbl_aten(logits_q, (H, W), spmask, th)
    _need(logits_q, "logits_q", torch.float32)
    if not naive_plbl_supported(logits_q, (H, W)):
        raise ValueError("naive_pseudo_labels: logits %s cannot be upsampled to %dx%d (an upsampling with W <= 6 w, or the identity)"
                         % (tuple(logits_q.shape), H, W))
    N, C, h, w = logits_q.shape
    mask = None
    if th <= 0:
        if spmask is None or tuple(spmask.shape) != (N, H, W):
            raise ValueError("spmask must be [N,H,W] = [%d,%d,%d] when th <= 0" % (N, H, W))
        mask = _mask_u8(spmask.contiguous())
    out = torch.empty((N, H, W), dtype=torch.uint8, device=logits_q.device)
    with torch.cuda.device(logits_q.device):
        _lib.check(_lib.load().mas_naive_plbl(logits_q.data_ptr(), N, C, h, w, H, W, mask.data_ptr() if mask is not None else None, th,
                                              out.data_ptr(), _stream(logits_q)), "mas_naive_plbl")
    return out.long()


def _meaniou_counts_aten(labels, targets, K, ignore_label, counts):
    """``MeanIoU(K, ignore_label)._after_step`` of the reference (``utils/miou.py:23-38``) in torch, added to ``counts`` [3K+3]."""
    keep = targets != ignore_label
    o, t = labels[keep], targets[keep]
    for i in range(K):
        counts[i] += int(torch.sum(t == i))
        counts[K + i] += int(torch.sum((t == i) & (o == t)))
        counts[2 * K + i] += int(torch.sum(o == i))
    return counts


def _candidate_plbl_aten(logits_q, size, spmask, rows, superpixels, inner, fallback, th, ce_temp):
    """The reference's lines on the upsampled logits (``upsample_bilinear`` on the GPU, ``F.interpolate`` on the CPU):
    ``top_pseudo_label_generation`` (``eval_within_multihot.py:110-146``; an id outside the rows gives 255 where the reference would
    raise) or the given map under the mask, then ``eval_save_candidateplbl_prop.py:50-59`` outside it."""
    import torch.nn.functional as F
    H, W = int(size[0]), int(size[1])
    if tuple(logits_q.shape[2:]) == (H, W):
        z = logits_q
    elif logits_q.is_cuda:
        z = upsample_bilinear(logits_q, (H, W))
    else:
        z = F.interpolate(logits_q, size=(H, W), mode='bilinear', align_corners=False)
    N, C = z.shape[:2]
    spmask = spmask.bool()
    if inner is not None:
        plbl = torch.where(spmask, inner, torch.full_like(inner, 255)).reshape(N, -1)
    else:
        S = rows.shape[1]
        plbl = torch.full((N, H * W), 255, dtype=torch.int64, device=z.device)
        outputs = z.permute(0, 2, 3, 1).reshape(N, -1, C)
        for i in range(N):
            valid = spmask[i].reshape(-1)
            if not torch.any(valid):
                continue
            ids = superpixels[i].reshape(-1)[valid]
            known = (ids >= 0) & (ids < S)
            trg_pixel = rows[i][ids.clamp(0, S - 1)]
            lab = (outputs[i][valid] * trg_pixel).max(dim=1)[1]
            plbl[i, valid.nonzero().squeeze(dim=1)] = torch.where(known, lab, torch.full_like(lab, 255))
    plbl = plbl.reshape(N, H, W)
    if fallback:
        top1, cls = torch.max(torch.softmax(z / ce_temp, dim=1), dim=1)
        keep = torch.logical_and(top1 > th, torch.logical_not(spmask))
        plbl = torch.where(keep, cls, plbl)
    return plbl


def candidate_pseudo_labels(logits_q, size, spmask, *, targets_rows=None, superpixels=None, inner=None, fallback=False, th=0.0,
                            ce_temp=1.0, targets=None, counts=None, num_classes=None, ignore_label=255):
    """Stage-2 labels without expansion, int64 ``[N,H,W]`` (255 = none) -- ``trainer/eval_save_candidateplbl.py``,
    ``eval_save_candidateplbl_prop.py`` and ``eval_save_cosplbl_naiveprop.py``.  logits_q f32 ``[N,C,h,w]``: the network's
    quarter-resolution logits (``net(x, lowres=True)``) or full-resolution ones; per pixel the C values of the bilinear upsampling to
    ``size`` (bit for bit that of ``upsample_bilinear``).  Under ``spmask`` (bool ``[N,H,W]``) exactly one of

    * ``targets_rows`` u8 ``[N,S,C]`` with ``superpixels`` int64 ``[N,H,W]``: the first arg-max of ``logit * row`` over the superpixel's
      multi-hot row (``top_pseudo_label_generation``, the quirk for all-negative candidate logits included; C <= 32);
    * ``inner`` int64 ``[N,H,W]``: labels decided elsewhere (``stage2_pseudo_labels(expand=False)``).

    Outside it 255, or with ``fallback`` the top-1 where ``1 / sum_c exp((y_c - y_max) / ce_temp) > th`` (``th >= 0``; 0 keeps every
    pixel; not bit-equal to ``torch.softmax``).  ``counts`` (int64 ``[3K+3]``, K = ``num_classes``, required with it):
    ``MeanIoU(K, ignore_label)._after_step`` of the labels against ``targets`` (int64 ``[N,H,W]``) is ADDED to it.  One launch
    (``csrc/candidate_plbl.hip``): the full-resolution logits never exist.  CPU tensors, and ``MAS_CANDIDATE_PLBL=aten``, take the
    reference's ATen chain."""
    H, W = int(size[0]), int(size[1])
    th, ce_temp, fallback = float(th), float(ce_temp), bool(fallback)
    cand = targets_rows is not None or superpixels is not None
    if cand == (inner is not None) or (cand and (targets_rows is None or superpixels is None)):
        raise ValueError("candidate_pseudo_labels takes exactly one of (targets_rows and superpixels) or inner")
    if logits_q.dim() != 4 or logits_q.dtype != torch.float32:
        raise TypeError("logits_q must be float32 [N,C,h,w], got %s %s" % (logits_q.dtype, tuple(logits_q.shape)))
    if not naive_plbl_supported(logits_q, (H, W)):
        raise ValueError("candidate_pseudo_labels: logits %s cannot be upsampled to %dx%d (an upsampling with W <= 6 w, or the identity)"
                         % (tuple(logits_q.shape), H, W))
    N, C, h, w = logits_q.shape
    if spmask is None or tuple(spmask.shape) != (N, H, W):
        raise ValueError("spmask must be [N,H,W] = [%d,%d,%d]" % (N, H, W))
    if cand:
        if C > 32:
            raise ValueError("candidate mode takes at most 32 channels (one int32 of bits per row), got %d" % C)
        if superpixels.dtype != torch.int64:
            raise TypeError("superpixels must be torch.int64, got %s" % superpixels.dtype)
        if tuple(superpixels.shape) != (N, H, W):
            raise ValueError("superpixels %s do not match [N,H,W] = [%d,%d,%d]" % (tuple(superpixels.shape), N, H, W))
        if targets_rows.dim() != 3 or targets_rows.shape[0] != N or targets_rows.shape[2] != C or targets_rows.shape[1] < 1:
            raise ValueError("targets_rows %s must be [N,S,C] = [%d,S,%d]" % (tuple(targets_rows.shape), N, C))
    else:
        if inner.dtype != torch.int64:
            raise TypeError("inner must be torch.int64, got %s" % inner.dtype)
        if tuple(inner.shape) != (N, H, W):
            raise ValueError("inner %s does not match [N,H,W] = [%d,%d,%d]" % (tuple(inner.shape), N, H, W))
        if not 1 <= C <= 255:
            raise ValueError("candidate_pseudo_labels takes 1 .. 255 channels, got %d" % C)
    if fallback and not (th >= 0.0 and ce_temp > 0.0):
        raise ValueError("the fallback needs th >= 0 and ce_temp > 0, got %r and %r" % (th, ce_temp))
    K = None if num_classes is None else int(num_classes)
    if counts is not None:
        if K is None:
            raise ValueError("num_classes is required with counts")
        if targets is None:
            raise ValueError("targets are required with counts")
        if not 1 <= K <= _lib.MAX_CLASSES:
            raise ValueError("num_classes %d must be within [1, %d]" % (K, _lib.MAX_CLASSES))
        if counts.dtype != torch.int64 or tuple(counts.shape) != (3 * K + 3,) or counts.device != logits_q.device:
            raise ValueError("counts must be int64 [3K+3] = [%d] on the logits' device" % (3 * K + 3))
    if targets is not None:
        if targets.dtype != torch.int64:
            raise TypeError("targets must be torch.int64, got %s" % targets.dtype)
        if tuple(targets.shape) != (N, H, W):
            raise ValueError("targets %s do not match [N,H,W] = [%d,%d,%d]" % (tuple(targets.shape), N, H, W))
    if not logits_q.is_cuda or os.environ.get("MAS_CANDIDATE_PLBL", "fused") == "aten":
        labels = _candidate_plbl_aten(logits_q, (H, W), spmask, targets_rows, superpixels, inner, fallback, th, ce_temp)
        if counts is not None:
            _meaniou_counts_aten(labels, targets, K, int(ignore_label), counts)
        return labels
    _need(logits_q, "logits_q", torch.float32)
    mask = _mask_u8(spmask.contiguous())
    spx = bits = None
    S = 0
    if cand:
        spx = _need(superpixels, "superpixels", torch.int64)
        rows = targets_rows if targets_rows.dtype == torch.uint8 else targets_rows.to(torch.uint8)
        bits = target_bits(rows.contiguous())
        S = int(rows.shape[1])
    else:
        _need(inner, "inner", torch.int64)
    if counts is not None:
        _need(counts, "counts", torch.int64)
        _need(targets, "targets", torch.int64)
    out = torch.empty((N, H, W), dtype=torch.uint8, device=logits_q.device)
    with torch.cuda.device(logits_q.device):
        _lib.check(_lib.load().mas_candidate_plbl(
            logits_q.data_ptr(), N, C, h, w, H, W, mask.data_ptr(), _opt(spx), _opt(bits), S, _opt(inner), int(fallback), th,
            inv_temperature(ce_temp), targets.data_ptr() if counts is not None else None, K if counts is not None else 0,
            int(ignore_label), _opt(counts), out.data_ptr(), _stream(logits_q)), "mas_candidate_plbl")
    return out.long()


def _ms_mean_aten(logits_q, sizes, flips, out_size):
    """The reference's lines (``eval_save_cosplbl_naive_voc_ms.py:59-87``) on the quarter-resolution logits: ``feat_forward``'s x4
    upsampling (``upsample_bilinear`` on the GPU, ``F.interpolate`` on the CPU), the flip back, ``F.interpolate`` to the original size,
    the sum in source order, ``/ n`` -> the mean logits [1,C,H,W]."""
    import torch.nn.functional as F
    acc = None
    for z, (Hs, Ws), fl in zip(logits_q, sizes, flips):
        if z.is_cuda:
            s = upsample_bilinear(z.contiguous(), (Hs, Ws))
        else:
            s = F.interpolate(z, size=(Hs, Ws), mode='bilinear', align_corners=False)
        if fl:
            s = s.flip(-1)
        v = F.interpolate(s, size=tuple(out_size), mode='bilinear', align_corners=False)
        acc = v if acc is None else acc + v
    return acc / len(logits_q)


def _ms_sources(name, logits_q, scaled_sizes, flips, out_size, feats_q=None):
    """The argument checks the multi-scale ops share -> (n, device, C, the [n,5] geometry table as a flat list, H, W).  ``feats_q``
    (``ms_ensemble``): a second tensor per source, ``[1,Ch,hq,wq]``, held to the same rules and to the size of its logits."""
    n = len(logits_q)
    if not 1 <= n <= _lib.MS_MAX_SOURCES:
        raise ValueError("%s takes 1 .. %d sources, got %d" % (name, _lib.MS_MAX_SOURCES, n))
    lists = [("logits_q", logits_q)] + ([] if feats_q is None else [("feats_q", feats_q)])
    if len(scaled_sizes) != n or len(flips) != n or any(len(ts) != n for _, ts in lists):
        raise ValueError("%s, scaled_sizes and flips must have one entry per source" % ", ".join(what for what, _ in lists))
    H, W = int(out_size[0]), int(out_size[1])
    if H < 1 or W < 1:
        raise ValueError("out_size must be non-empty, got %r" % (tuple(out_size),))
    dev = logits_q[0].device
    geom = []
    for k in range(n):
        for what, ts in lists:
            z = ts[k]
            if z.device != dev:
                raise ValueError("all sources must live on one device")
            if z.dtype != torch.float32:
                raise TypeError("%s[%d] must be torch.float32, got %s" % (what, k, z.dtype))
            if z.dim() != 4 or z.shape[0] != 1:
                raise ValueError("source %d: %s must be [1,C,hq,wq], got %s" % (k, what, tuple(z.shape)))
            if z.shape[1] != ts[0].shape[1]:
                raise ValueError("source %d: channel count of %s differs from source 0" % (k, what))
            if z.shape[2:] != logits_q[k].shape[2:]:
                raise ValueError("source %d: %s %s and logits_q %s differ in size" % (k, what, tuple(z.shape), tuple(logits_q[k].shape)))
        hq, wq = int(logits_q[k].shape[2]), int(logits_q[k].shape[3])
        Hs, Ws = int(scaled_sizes[k][0]), int(scaled_sizes[k][1])
        if Hs < 1 or Ws < 1:
            raise ValueError("source %d: empty scaled size %dx%d" % (k, Hs, Ws))
        if (hq, wq) != (quarter_size(Hs), quarter_size(Ws)):
            raise ValueError("source %d: quarter-resolution maps %dx%d are not what the network emits for %dx%d (%dx%d)"
                             % (k, hq, wq, Hs, Ws, quarter_size(Hs), quarter_size(Ws)))
        geom += [hq, wq, Hs, Ws, 1 if flips[k] else 0]
    return n, dev, int(logits_q[0].shape[1]), geom, H, W


def _ms_targets_counts(targets, counts, K, H, W, dev):
    """The checks ``ms_naive_labels`` and ``ms_iou_counts`` share on ``targets`` (int64, H * W elements ending in ``[H,W]``) and
    ``counts`` (int64 ``[3K+3]``), both on the logits' device; either may be None."""
    if targets is not None:
        if targets.dtype != torch.int64:
            raise TypeError("targets must be torch.int64, got %s" % targets.dtype)
        if tuple(targets.shape[-2:]) != (H, W) or targets.numel() != H * W:
            raise ValueError("targets %s do not match the picture %dx%d" % (tuple(targets.shape), H, W))
        if targets.device != dev:
            raise ValueError("targets must live on the logits' device")
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (3 * K + 3,) or counts.device != dev):
        raise ValueError("counts must be int64 [3K+3] = [%d] on the logits' device" % (3 * K + 3))


def _ms_pack(geom, **tensor_lists):
    """-> [the ``(c_int32 * 5n)`` geometry table, one ``(c_void_p * n)`` pointer array per tensor list]; the tensors must be contiguous
    f32 on the GPU."""
    out = [(ctypes.c_int32 * len(geom))(*geom)]
    for name, ts in tensor_lists.items():
        out.append((ctypes.c_void_p * len(ts))(*[_need(t, "%s[%d]" % (name, k), torch.float32).data_ptr() for k, t in enumerate(ts)]))
    return out


def ms_naive_labels(logits_q, scaled_sizes, flips, out_size, targets=None, counts=None, num_classes=None, ignore_label=255):
    """Naive arg-max pseudo labels int64 ``[1,H,W]`` of the VOC generators (``trainer/eval_save_cosplbl_naive_voc[_ms].py``) from n <= 16
    sources, each the network's quarter-resolution logits ``[1,C,hq,wq]`` (``net(x, lowres=True)``) on the picture scaled to
    ``scaled_sizes[k] = (Hs, Ws)`` and flipped horizontally when ``flips[k]``: upsampled x4 to the scaled size, flipped back, resized to
    ``out_size = (H, W)``, averaged, the first arg-max over the channels -- ``torch.max(ms_ensemble(...)[1], 1)[1]`` bit for bit.
    ``counts`` (int64 ``[3K+3]``, K = ``num_classes``, required with it): ``MeanIoU(K, ignore_label)._after_step`` of the labels against
    ``targets`` (int64 ``[1,H,W]`` or ``[H,W]``) is ADDED to it.  One launch (``csrc/ms_naive.hip``): neither the scaled-size nor the
    full-resolution logits exist.  CPU tensors, and ``MAS_MS_NAIVE=aten``, take the reference's ATen chain."""
    if counts is not None:
        if num_classes is None:
            raise ValueError("num_classes is required with counts")
        if targets is None:
            raise ValueError("targets are required with counts")
    n, dev, C, geom, H, W = _ms_sources("ms_naive_labels", logits_q, scaled_sizes, flips, out_size)
    if not 1 <= C <= 255:
        raise ValueError("ms_naive_labels takes 1 .. 255 channels, got %d" % C)
    K = None if num_classes is None else int(num_classes)
    if counts is not None and not C <= K <= _lib.MAX_CLASSES:
        raise ValueError("num_classes %d must be within [%d, %d] (the channels .. MAX_CLASSES)" % (K, C, _lib.MAX_CLASSES))
    _ms_targets_counts(targets, counts, K, H, W, dev)
    sizes = [(int(s[0]), int(s[1])) for s in scaled_sizes]
    if not logits_q[0].is_cuda or os.environ.get("MAS_MS_NAIVE", "fused") == "aten":
        labels = _ms_mean_aten(logits_q, sizes, [bool(f) for f in flips], (H, W)).max(dim=1)[1]
        if counts is not None:
            t = targets.reshape(1, H, W)
            if labels.is_cuda:
                iou_counts(labels.contiguous(), None, t.contiguous(), K, int(ignore_label), counts)
            else:
                _meaniou_counts_aten(labels, t, K, int(ignore_label), counts)
        return labels
    g, lp = _ms_pack(geom, logits_q=logits_q)
    if counts is not None:
        _need(counts, "counts", torch.int64)
        _need(targets, "targets", torch.int64)
    out = torch.empty((1, H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_ms_naive_plbl(lp, g, n, C, H, W, targets.data_ptr() if counts is not None else None,
                                                 K if counts is not None else 0, int(ignore_label), out.data_ptr(),
                                                 counts.data_ptr() if counts is not None else None, _stream(out)), "mas_ms_naive_plbl")
    return out.long()


MS_MAX_LDS = 64 * 1024      # the LDS one workgroup of csrc/ms_naive.hip may use


def ms_iou_lds_bytes(geometry, out_size):
    """The LDS one workgroup of ``mas_ms_iou_counts`` needs for the flat ``[n,5]`` geometry table ``(hq, wq, Hs, Ws, flip)`` and
    ``out_size`` -- the launch's own sizing code (``mas_ms_iou_lds_bytes``; no device is touched) -- or a negative status."""
    g, = _ms_pack([int(v) for v in geometry])
    return int(_lib.load().mas_ms_iou_lds_bytes(g, len(g) // 5, int(out_size[0]), int(out_size[1])))


def ms_iou_supported(logits_q, scaled_sizes, flips, out_size):
    """True on GPU tensors when ``ms_iou_counts`` accepts the sources: 1 .. 16 of them, each what the network emits for its scaled size,
    and a stage-2 downsample whose tile fits the LDS (factors up to 2.0 do), by the entry point's own sizing code."""
    if not all(torch.is_tensor(z) and z.is_cuda for z in logits_q):
        return False
    try:
        _, _, _, geom, H, W = _ms_sources("ms_iou_supported", logits_q, scaled_sizes, flips, out_size)
    except (TypeError, ValueError):
        return False
    return 0 <= ms_iou_lds_bytes(geom, (H, W)) <= MS_MAX_LDS


def _iou_counts_aten(m, targets, K, ignore_label, counts):
    """``MeanIoU(K)._after_step(m[:, :K].max(1)[1])`` and, with K + 1 channels, ``IoUIgnore(K)._after_step(m.max(1)[1])`` of the reference
    (``trainer/eval_naive.py:61-63``, ``utils/miou.py:23-38``, ``utils/miou_evalignore.py:20-32``) in torch, added to ``counts`` [3K+3]."""
    o_cls = m[:, :K].max(dim=1)[1]
    _meaniou_counts_aten(o_cls, targets, K, ignore_label, counts)
    if m.shape[1] > K:
        tig, oig = targets == ignore_label, m.max(dim=1)[1] == K
        counts[3 * K] += int(torch.sum(tig))
        counts[3 * K + 1] += int(torch.sum(tig & oig))
        counts[3 * K + 2] += int(torch.sum(oig))
    return o_cls


def ms_iou_counts(logits_q, scaled_sizes, flips, out_size, targets, num_classes, ignore_label, counts=None, pred=None):
    """The evaluation counters (``logits_iou_counts``: ``MeanIoU`` + ``IoUIgnore``) of the mean logits of n <= 16 scaled and flipped copies
    of one picture -- multi-scale + flip evaluation.  Sources as ``ms_naive_labels``: ``logits_q[k]`` f32 ``[1,CH,hq,wq]`` is the
    network's quarter-resolution output on the picture scaled to ``scaled_sizes[k]`` and flipped when ``flips[k]``; the mean is that of
    ``ms_ensemble`` bit for bit.  ``CH`` = K or K + 1 with K = ``num_classes``: the class arg-max runs over the first K channels, the
    "undefined" triple (only with K + 1 channels) over all of them; the first maximum wins and a NaN takes the place and keeps it
    (``torch.max``).  ``targets`` int64 ``[1,H,W]`` or ``[H,W]``; ``counts`` int64 ``[3K+3]`` is ADDED to (made when None) and
    returned; ``pred`` (optional, uint8 ``[H,W]``) receives the class arg-max.  One launch (``csrc/ms_naive.hip``): neither the
    scaled-size nor the full-resolution logits exist; a geometry ``ms_iou_supported`` declines raises.  CPU tensors, and
    ``MAS_MS_EVAL=aten``, take the ATen chain: the materialised mean logits, then ``logits_iou_counts`` (on the CPU the reference's
    ``torch.sum`` loops).  ``logits_iou_counts`` never lets a NaN win, so with NaN logits the two GPU paths differ."""
    n, dev, CH, geom, H, W = _ms_sources("ms_iou_counts", logits_q, scaled_sizes, flips, out_size)
    K = int(num_classes)
    if not 1 <= K <= _lib.MAX_CLASSES or CH not in (K, K + 1):
        raise ValueError("ms_iou_counts: %d channels are neither num_classes = %d (<= %d) nor num_classes + 1" % (CH, K, _lib.MAX_CLASSES))
    if targets is None:
        raise TypeError("targets must be torch.int64")
    _ms_targets_counts(targets, counts, K, H, W, dev)
    if counts is None:
        counts = torch.zeros(3 * K + 3, dtype=torch.int64, device=dev)
    if pred is not None and (pred.dtype != torch.uint8 or pred.numel() != H * W or pred.device != dev or not pred.is_contiguous()):
        raise ValueError("pred must be a contiguous uint8 [H,W] = [%d,%d] tensor on the logits' device" % (H, W))
    sizes = [(int(s[0]), int(s[1])) for s in scaled_sizes]
    if not logits_q[0].is_cuda or os.environ.get("MAS_MS_EVAL", "fused") == "aten":
        m = _ms_mean_aten(logits_q, sizes, [bool(f) for f in flips], (H, W))
        t = targets.reshape(1, H, W)
        if m.is_cuda:
            logits_iou_counts(m.contiguous(), t.contiguous(), K, int(ignore_label), counts)
            if pred is not None:
                pred.view(H, W).copy_(m[0, :K].max(dim=0)[1])
        else:
            o_cls = _iou_counts_aten(m, t, K, int(ignore_label), counts)
            if pred is not None:
                pred.view(H, W).copy_(o_cls[0])
        return counts
    if not 0 <= ms_iou_lds_bytes(geom, (H, W)) <= MS_MAX_LDS:
        raise ValueError("ms_iou_counts: a stage-2 downsample of these sources to %dx%d needs more LDS than one tile may use" % (H, W))
    g, lp = _ms_pack(geom, logits_q=logits_q)
    _need(targets, "targets", torch.int64)
    _need(counts, "counts", torch.int64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mas_ms_iou_counts(lp, g, n, CH, H, W, targets.data_ptr(), K, int(ignore_label), counts.data_ptr(),
                                                 pred.data_ptr() if pred is not None else None, _stream(counts)), "mas_ms_iou_counts")
    return counts


# ------------------------------------------------------------------------------------------------
# BatchNorm2d + ReLU + residual add, fused (csrc/bn.hip)
# ------------------------------------------------------------------------------------------------
_BN_COUNTERS = {}


def _bn_counters(dev, C):
    """The per-(device, stream) completion counters of the last-block form of the BatchNorm passes (one zeroed word per channel; the
    kernels leave them zeroed) under MAS_BN_LASTBLOCK=on.  Default off: None -- the statistics come from their own launch.  (Round 5
    measured the last-block form at 25.7-25.9 ms per training step against 25.6 for the three-launch form: the store-drain-publish
    tail of every workgroup costs what the 115 five-microsecond launches did.  Kept for the A/B and its bit-identity test.)"""
    if os.environ.get("MAS_BN_LASTBLOCK", "off") != "on":
        return None
    return _stream_scratch(_BN_COUNTERS, dev, lambda: torch.zeros(max(4096, C), dtype=torch.int32, device=dev), C)


class _BNActTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, num_batches_tracked, eps, momentum, relu, partials=None):
        x = x.contiguous()
        N, C, H, W = x.shape
        HW = H * W
        dev = x.device
        res = residual.contiguous() if residual is not None else None
        lib = _lib.load()
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd = torch.empty(C, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        # ReLU mask, one byte per aligned group of four outputs: the backward then reads 1/16 of the bytes of y
        mask = torch.empty(int(lib.mas_bn_mask_bytes(N, C, HW)), dtype=torch.uint8, device=dev) if relu else None
        with torch.cuda.device(dev):
            if partials is not None:
                # (sum, sum of squares) per channel and pixel set, formed in the epilogue of the convolution that produced x
                # (conv_sk(..., stats=True)): no reduction pass over x
                if partials.dtype != torch.float64 or partials.dim() != 3 or partials.shape[0] != C or partials.shape[2] != 2:
                    raise ValueError("partials must be [C, slots, 2] float64")
                _lib.check(lib.mas_bn_act_train_fwd_stats(x.data_ptr(), partials.data_ptr(), int(partials.shape[1]), _opt(weight), _opt(bias), _opt(res),
                                                          N, C, HW, float(eps), float(momentum), int(relu), _opt(running_mean), _opt(running_var),
                                                          _opt(num_batches_tracked), mean.data_ptr(), invstd.data_ptr(), y.data_ptr(), _opt(mask),
                                                          _stream(x)), "mas_bn_act_train_fwd_stats")
            else:
                ws = torch.empty(int(lib.mas_bn_workspace_bytes(N, C, HW)), dtype=torch.uint8, device=dev)
                _lib.check(lib.mas_bn_act_train_fwd(x.data_ptr(), _opt(weight), _opt(bias), _opt(res), N, C, HW, float(eps), float(momentum),
                                                    int(relu), _opt(running_mean), _opt(running_var), _opt(num_batches_tracked),
                                                    mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), y.data_ptr(), _opt(mask), _opt(_bn_counters(dev, C)),
                                                    _stream(x)),
                           "mas_bn_act_train_fwd")
        # the kernel updated the running statistics through raw pointers: bump their version counters as an in-place
        # torch op would, so caches keyed on (data_ptr, _version) -- _bn_fold -- see the change
        for buf in (running_mean, running_var, num_batches_tracked):
            if buf is not None:
                torch.autograd.graph.increment_version(buf)
        ctx.save_for_backward(x, y if mask is None else None, weight, mean, invstd, mask)
        ctx.relu = bool(relu)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, mean, invstd, mask = ctx.saved_tensors
        N, C, H, W = x.shape
        HW = H * W
        dev = x.device
        dy = dy.contiguous()
        lib = _lib.load()
        ws = torch.empty(int(lib.mas_bn_workspace_bytes(N, C, HW)), dtype=torch.uint8, device=dev)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        dg = torch.empty(C, dtype=torch.float32, device=dev) if (weight is not None and ctx.needs_input_grad[1]) else None
        db = torch.empty(C, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        with torch.cuda.device(dev):
            _lib.check(lib.mas_bn_act_train_bwd(dy.data_ptr(), x.data_ptr(), _opt(y), _opt(mask), _opt(weight), mean.data_ptr(), invstd.data_ptr(),
                                                N, C, HW, int(ctx.relu), ws.data_ptr(), dx.data_ptr(), _opt(dres), _opt(dg), _opt(db),
                                                _opt(_bn_counters(dev, C)), _stream(x)), "mas_bn_act_train_bwd")
        if ctx.has_res and dres is None and ctx.needs_input_grad[3]:
            dres = dy
        return dx, dg, db, dres, None, None, None, None, None, None, None


def bn_act_supported(bn, x, residual=None):
    """Fused path: f32 NCHW GPU tensors; training mode (batch statistics) or inference without autograd.  A frozen
    BatchNorm (eval mode with gradients flowing through it) stays on the PyTorch ops."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] <= 65535 and x.shape[1] <= 65535):
        return False
    if residual is not None and (residual.shape != x.shape or residual.dtype != torch.float32):
        return False
    if bn.training:
        return bn.momentum is not None and x.shape[0] * x.shape[2] * x.shape[3] > 1
    if not bn.track_running_stats:
        return False
    return not (torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)))


def bn_act(bn, x, relu=True, residual=None, partials=None):
    """relu?(bn(x) + residual) for a ``torch.nn.BatchNorm2d`` module ``bn`` (parameters, running statistics and
    ``num_batches_tracked`` are the module's own and are updated as PyTorch updates them).  ``partials`` (training): the
    per-channel partial sums of x that conv_train(..., stats=True) returns beside x."""
    if bn.training:
        rm, rv, nbt = (bn.running_mean, bn.running_var, bn.num_batches_tracked) if bn.track_running_stats else (None, None, None)
        return _BNActTrain.apply(x, bn.weight, bn.bias, residual, rm, rv, nbt, bn.eps, bn.momentum, relu, partials)
    x = x.contiguous()
    N, C, H, W = x.shape
    res = residual.contiguous() if residual is not None else None
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mas_bn_act_eval_fwd(x.data_ptr(), _opt(bn.weight), _opt(bn.bias), bn.running_mean.data_ptr(),
                                                   bn.running_var.data_ptr(), _opt(res), N, C, H * W, float(bn.eps), int(relu), y.data_ptr(),
                                                   _stream(x)), "mas_bn_act_eval_fwd")
    return y


# ------------------------------------------------------------------------------------------------
# the 1x1 convolution of a 1x1 map (ASPP image-pooling branch): a fixed-order [N,K] x [K,M] product (csrc/head.hip)
# ------------------------------------------------------------------------------------------------
class _DenseSmall(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x, w = x.contiguous(), w.contiguous()
        N, K = x.shape
        M = w.shape[0]
        y = torch.empty((N, M), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mas_dense_small_fwd(x.data_ptr(), w.data_ptr(), N, K, M, y.data_ptr(), _stream(x)), "mas_dense_small_fwd")
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        N, K = x.shape
        M = w.shape[0]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mas_dense_small_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), N, K, M, _opt(dx), _opt(dw), _stream(x)),
                       "mas_dense_small_bwd")
        return dx, dw


def conv1x1_on_1x1_supported(conv, x):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[2] * x.shape[3] == 1 and conv.kernel_size == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1 and conv.bias is None and x.shape[1] == conv.in_channels
            and x.shape[0] * conv.out_channels <= 1 << 20)


def conv1x1_on_1x1(conv, x):
    """conv(x) for a 1x1 convolution of a 1x1 map [N,K,1,1] -> [N,M,1,1] with autograd, fixed summation order (mas_dense_small_*)."""
    y = _DenseSmall.apply(x.flatten(1), conv.weight.flatten(1))
    return y[:, :, None, None]


# ------------------------------------------------------------------------------------------------
# K8: cosine classifier (csrc/head.hip)
# ------------------------------------------------------------------------------------------------
class _CosineHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, proxy_hat):
        feat, proxy_hat = feat.contiguous(), proxy_hat.contiguous()
        N, Ch, H, W = feat.shape
        K = proxy_hat.shape[0]
        logits = torch.empty((N, K, H, W), dtype=torch.float32, device=feat.device)
        inv = torch.empty((N, H, W), dtype=torch.float32, device=feat.device)
        with torch.cuda.device(feat.device):
            _lib.check(_lib.load().mas_cosine_head_fwd(feat.data_ptr(), proxy_hat.data_ptr(), N, Ch, K, H * W, 1e-12, logits.data_ptr(),
                                                       inv.data_ptr(), _stream(feat)), "mas_cosine_head_fwd")
        ctx.save_for_backward(feat, proxy_hat, logits, inv)
        return logits

    @staticmethod
    def backward(ctx, g):
        feat, proxy_hat, logits, inv = ctx.saved_tensors
        N, Ch, H, W = feat.shape
        K = proxy_hat.shape[0]
        g = g.contiguous()
        dfeat = dph = None
        if ctx.needs_input_grad[0]:
            dfeat = torch.empty_like(feat)
            with torch.cuda.device(feat.device):
                _lib.check(_lib.load().mas_cosine_head_bwd(feat.data_ptr(), proxy_hat.data_ptr(), logits.data_ptr(), inv.data_ptr(),
                                                           g.data_ptr(), N, Ch, K, H * W, dfeat.data_ptr(), _stream(feat)),
                           "mas_cosine_head_bwd")
        if ctx.needs_input_grad[1]:
            gs = (g * inv[:, None]).reshape(N, K, H * W)                       # small: [N,K,HW]
            dph = torch.bmm(gs, feat.reshape(N, Ch, H * W).transpose(1, 2)).sum(0)      # [K,Ch] = sum_n gs_n @ f_n^T  (hipBLASLt)
        return dfeat, dph


def cosine_head_supported(feat, proxy):
    return (feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 4 and proxy.dim() == 4 and proxy.shape[2:] == (1, 1)
            and proxy.shape[0] in (19, 20, 21) and proxy.shape[1] == feat.shape[1] and feat.shape[0] <= 65535)


def cosine_head(feat, proxy):
    """logits = conv2d(normalize(feat), normalize(proxy)) (deeplabv3.py:121-124); proxy [K,Ch,1,1] raw weights (their
    normalisation over dim 1 stays a PyTorch op on the [K,Ch] tensor, so its gradient is autograd's)."""
    phat = torch.nn.functional.normalize(proxy, dim=1).reshape(proxy.shape[0], proxy.shape[1])
    return _CosineHead.apply(feat, phat)


# ------------------------------------------------------------------------------------------------
# stem max-pool (csrc/pool.hip)
# ------------------------------------------------------------------------------------------------
class _MaxPool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        N, C, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
        arg = torch.empty((N, C, Ho, Wo), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().mas_maxpool3s2_fwd(x.data_ptr(), N * C, H, W, y.data_ptr(), arg.data_ptr(), _stream(x)), "mas_maxpool3s2_fwd")
        ctx.save_for_backward(arg)
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        g = g.contiguous()
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().mas_maxpool3s2_bwd(g.data_ptr(), arg.data_ptr(), N * C, H, W, dx.data_ptr(), _stream(g)), "mas_maxpool3s2_bwd")
        return dx


def maxpool3s2_supported(pool, x):
    def two(v):
        return (v, v) if isinstance(v, int) else tuple(v)
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] * x.shape[1] <= 65535 and x.shape[2] <= 65535
            and two(pool.kernel_size) == (3, 3) and two(pool.stride) == (2, 2) and two(pool.padding) == (1, 1)
            and two(pool.dilation) == (1, 1) and not pool.ceil_mode and not pool.return_indices)


def maxpool3s2(x):
    _need(x, "x", torch.float32)
    return _MaxPool3s2.apply(x)


# ------------------------------------------------------------------------------------------------
# small-K 1x1 convolution with the inference BatchNorm + ReLU epilogue (csrc/conv1x1.hip)
# ------------------------------------------------------------------------------------------------
def conv1x1_bn_act_supported(conv, bn, x):
    """Inference only (eval-mode BatchNorm, no autograd): 1x1 / stride 1 / no bias, at most 64 output channels -- the
    shapes where the HIP kernel beats MIOpen's GEMM path (1.6-2.2x at 256x512; tools/conv1x1_hip_probe.py)."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and not bn.training and bn.track_running_stats
            and not torch.is_grad_enabled() and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)
            and conv.groups == 1 and conv.bias is None and conv.out_channels in (32, 64) and conv.in_channels % 4 == 0
            and (x.shape[2] * x.shape[3]) % 4 == 0 and x.shape[0] <= 65535)


def _conv1x1_constants(conv, bn):
    """(transposed weight [K,M], scale [M], shift [M]): the weight cached on the conv module until it changes, the rest from _bn_fold."""
    def transposed():
        with torch.no_grad():
            return conv.weight.reshape(conv.out_channels, conv.in_channels).t().contiguous()
    return (_cached(conv, '_mas_conv1x1_cache', (conv.weight,), transposed),) + _bn_fold(bn)


def conv1x1_bn_act(conv, bn, x, relu=True, residual=None):
    """relu?(bn(conv(x)) + residual) in one kernel (inference)."""
    x = x.contiguous()
    N, K, H, W = x.shape
    M = conv.out_channels
    w_t, scale, shift = _conv1x1_constants(conv, bn)
    _, _, res, y = _fused_epilogue(None, residual, (N, M, H, W), x.device, strict=False)     # (the fold came with the weight)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mas_conv1x1_fwd(x.data_ptr(), w_t.data_ptr(), N, K, M, H * W, scale.data_ptr(), shift.data_ptr(), _opt(res),
                                               int(relu), y.data_ptr(), _stream(x)), "mas_conv1x1_fwd")
    return y


# ------------------------------------------------------------------------------------------------
# dense convolutions on the f32 matrix cores (csrc/conv_mfma.hip)
# ------------------------------------------------------------------------------------------------
def _conv_geometry(conv, x):
    """(kernel, stride, dilation, padding) of a dense square convolution this package can look at -- f32 NCHW input on the GPU with
    the convolution's input channels, no groups, no bias, the same kernel size / stride / dilation / padding along both axes -- or
    None."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.groups == 1 and conv.bias is None):
        return None
    k, s, d, pd = conv.kernel_size, conv.stride, conv.dilation, conv.padding
    if k[0] != k[1] or s[0] != s[1] or d[0] != d[1] or pd[0] != pd[1] or x.shape[1] != conv.in_channels:
        return None
    return k[0], s[0], d[0], pd[0]


def _is_1x1_or_3x3(k, s, d, pd, dilations):
    """The network's two layer forms at stride 1 / 2: 3x3 with padding = dilation in ``dilations`` (undilated at stride 2), or plain 1x1."""
    if s not in (1, 2):
        return False
    if k == 3:
        return pd == d and d in dilations and (s == 1 or d == 1)
    return k == 1 and pd == 0 and d == 1


def conv_mfma_supported(conv, x):
    """Shapes the implicit-GEMM MFMA kernel takes: 1x1 / 3x3, stride 1 or 2 (3x3 stride 2 only undilated), padding =
    dilation for 3x3, no groups, no bias, Cin % 8 (3x3) / % 16 (1x1) == 0 (any Cout: padded to 64 inside), fp32 NCHW on the GPU."""
    geom = _conv_geometry(conv, x)
    if geom is None or not _is_1x1_or_3x3(*geom, dilations=(1, 2)):
        return False
    return _lib.load().mas_conv_chunk(geom[0], conv.in_channels) > 0 and conv.in_channels * x.shape[2] * x.shape[3] < 2 ** 31


# Parameter epoch: advanced after EVERY optimizer step of the process.  The version counter of a tensor is not enough to key a
# cache of derived constants on: fused optimizers (torch.optim.AdamW(fused=True), what trainer/base.py uses on the GPU) update
# parameters in place without bumping ``_version``, so a packed weight or a folded BatchNorm would silently go stale after the
# first training step.
_PARAM_EPOCH = [0]


def _bump_param_epoch(*_args, **_kwargs):
    _PARAM_EPOCH[0] += 1


try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_step_hook
    _reg_step_hook(_bump_param_epoch)
except ImportError:                                     # pragma: no cover  (torch < 2.0)
    # Without the hook nothing tells this module that a fused optimizer stepped: packed weights and folded BatchNorm constants
    # would go stale after the first step and training would go on with wrong weights.  conv_train_plan then declines every layer
    # (the nn.Module / MIOpen path needs no derived constants) and says why, once.
    _reg_step_hook = None
    import warnings
    warnings.warn("torch.optim has no register_optimizer_step_post_hook: the package's training convolutions are disabled "
                  "(MIOpen is used); call ops.invalidate_parameter_caches() after every optimizer step to re-enable them by hand")


def invalidate_parameter_caches():
    """Call after changing parameters through raw pointers or anything else that bypasses both the version counters and
    torch.optim (every cache of packed weights / folded BatchNorm constants is rebuilt at its next use)."""
    _bump_param_epoch()


def _versions(tensors):
    return (_PARAM_EPOCH[0],) + tuple((t.data_ptr(), t._version) for t in tensors if t is not None)


def _cached(module, attr, tensors, build):
    """``build()``, kept in ``module.<attr>`` until one of ``tensors`` (parameters, running statistics) changes: its address, its
    version counter, or the process's parameter epoch."""
    key = _versions(tensors)
    cache = getattr(module, attr, None)
    if cache is None or cache[0] != key:
        cache = (key, build())
        setattr(module, attr, cache)
    return cache[1]


def _bn_tensors(bn):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var)


def _conv_packed_weight(conv):
    """The weight as mas_conv_fwd reads it -- [Cin/CK][KC/8][2][Cout][4]: k-step kk = tap * (CK/2) + cp pairs the input
    channels c = 2 cp + h (h = lane half of the MFMA), four consecutive k-steps of one (half, output channel) are
    adjacent -- cached on the module until the parameter changes."""
    def pack():
        with torch.no_grad():
            M, K, kh, kw = conv.weight.shape
            ck = _lib.load().mas_conv_chunk(kh, K)
            taps = kh * kw
            w = conv.weight.detach()
            if M % 64:                                              # output channels padded to 64 with zero rows (never stored)
                w = torch.cat([w, w.new_zeros((64 - M % 64, K, kh, kw))], dim=0)
                M = w.shape[0]
            w = w.reshape(M, K // ck, ck // 2, 2, taps)                             # [m, chunk, cp, h, tap]
            w = w.permute(1, 4, 2, 3, 0).reshape(K // ck, taps * ck // 2, 2, M)     # [chunk, kk = tap * ck/2 + cp, h, m]
            return w.reshape(K // ck, taps * ck // 8, 4, 2, M).permute(0, 1, 3, 4, 2).contiguous()      # [chunk, q, h, m, j]
    return _cached(conv, '_mas_conv_pack', (conv.weight,), pack)


def _bn_fold(bn):
    """(scale, shift) f32 [C] of an inference BatchNorm, cached on the module until a parameter or running statistic
    changes (the training kernels bump the buffers' version counters, _BNActTrain.forward)."""
    def fold():
        with torch.no_grad():
            inv = torch.rsqrt(bn.running_var.double() + bn.eps)
            g = bn.weight.double() if bn.weight is not None else torch.ones_like(inv)
            b = bn.bias.double() if bn.bias is not None else torch.zeros_like(inv)
            scale = g * inv
            shift = b - bn.running_mean.double() * scale
        return scale.float().contiguous(), shift.float().contiguous()
    return _cached(bn, '_mas_fold', _bn_tensors(bn), fold)


def _fused_epilogue(bn, residual, shape, dev, strict=True):
    """What the fused inference convolutions with output ``shape`` = (N, M, Ho, Wo) on ``dev`` share: (scale, shift, residual, y) --
    the folded BatchNorm (None, None without one), the residual made contiguous, the empty output.  ``strict``: a BatchNorm of
    another width or a residual that is not f32 ``shape`` on ``dev`` is a ValueError (the wrappers that always checked)."""
    if strict and bn is not None and bn.num_features != shape[1]:
        raise ValueError("BatchNorm has %d features, the convolution %d output channels" % (bn.num_features, shape[1]))
    scale, shift = _bn_fold(bn) if bn is not None else (None, None)
    if residual is not None:
        if strict and (tuple(residual.shape) != shape or residual.dtype != torch.float32 or residual.device != dev):
            raise ValueError("residual must be float32 %s on %s, got %s %s on %s"
                             % (shape, dev, residual.dtype, tuple(residual.shape), residual.device))
        residual = residual.contiguous()
    return scale, shift, residual, torch.empty(shape, dtype=torch.float32, device=dev)


def conv_mfma(conv, x, bn=None, relu=False, residual=None):
    """relu?(bn(conv(x)) + residual) in one kernel; ``bn`` None -> the bare convolution (then residual / relu still apply)."""
    x = x.contiguous()
    N, K, H, W = x.shape
    M = conv.out_channels
    ks, s, d = conv.kernel_size[0], conv.stride[0], conv.dilation[0]
    wt = _conv_packed_weight(conv)
    scale, shift, res, y = _fused_epilogue(bn, residual, (N, M, (H - 1) // s + 1, (W - 1) // s + 1), x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mas_conv_fwd(x.data_ptr(), wt.data_ptr(), N, K, H, W, M, ks, s, d, _opt(scale), _opt(shift), _opt(res),
                                            int(relu), y.data_ptr(), _stream(x)), "mas_conv_fwd")
    return y


# ------------------------------------------------------------------------------------------------
# the same convolutions on the bf16 matrix cores, f32 in / f32 out through exact three-term operand splits (csrc/conv_bx.hip)
# ------------------------------------------------------------------------------------------------
BX_ROLE_S2 = 2          # mas_conv_bx_pack role: the forward image of a 3x3 stride-2 convolution (nine shifted 1x1 stride-2 products)


def _train_bx():
    """MAS_TRAIN_BX as (bf16 allowed, round-4 rule): auto (default) -> (True, False): every product of a training step the split-bf16
    kernels take; r04 -> (True, True): only what round 4 gave them, for A/B runs; off -> (False, False)."""
    mode = os.environ.get("MAS_TRAIN_BX", "auto")
    return mode != "off", mode == "r04"


def _bx_s2k3():
    """MAS_BX_S2K3 (default on): may the 3x3 stride-2 convolutions run on the split-bf16 kernel?"""
    return os.environ.get("MAS_BX_S2K3", "on") != "off"


def conv_bx_supported(conv, x):
    """Shapes mas_conv_bx_fwd takes: 1x1 at stride 1 (any plane) / 2 (H even, W % 8 == 0), 3x3 stride 1 with dilation 1 / 2
    (padding = dilation) on planes at least 32 wide, 3x3 stride 2 (H even, W % 8 == 0, input channels a multiple of 32); any other
    channel counts; no groups, no bias."""
    geom = _conv_geometry(conv, x)
    if geom is None:
        return False
    k, s, d, pd = geom
    if pd != (d if k == 3 else 0) or (s == 2 and x.data_ptr() % 16):
        return False
    if s == 2 and k == 3 and not _bx_s2k3():                    # (A/B: the f32 pipe)
        return False
    return bool(_lib.load().mas_conv_bx_supported(k, s, d, conv.in_channels, conv.out_channels, x.shape[2], x.shape[3]))


def _conv_bx_weight(conv):
    """The split weight image of mas_conv_bx_pack, cached on the module until the parameter changes (inference: once per
    checkpoint load)."""
    def pack():
        lib = _lib.load()
        w = conv.weight.detach().contiguous()
        M, K, kh, _ = w.shape
        role = BX_ROLE_S2 if (kh == 3 and conv.stride[0] == 2) else 0        # (the strided 3x3: tap-major chunks of the 1x1 form)
        nbytes = lib.mas_conv_bx_packed_bytes(kh, K, M, role)
        if nbytes <= 0:
            raise ValueError("mas_conv_bx_pack does not take a %dx%d convolution with %d input channels" % (kh, kh, K))
        wp = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        with torch.cuda.device(w.device):
            _lib.check(lib.mas_conv_bx_pack(w.data_ptr(), None, M, K, kh, role, wp.data_ptr(), _stream(w)), "mas_conv_bx_pack")
        return wp
    return _cached(conv, '_mas_conv_bx_pack', (conv.weight,), pack)


def _conv_bx_folded(conv, bn):
    """(weight image with the inference BatchNorm's scale folded into its rows, shift [Cout]) for mas_conv_bx_fwd_dual, cached on the
    convolution until a parameter or running statistic changes."""
    def fold():
        scale, shift = _bn_fold(bn)
        return conv_bx_pack(conv.weight.detach(), 0, row_scale=scale), shift
    return _cached(conv, '_mas_conv_bx_folded', (conv.weight,) + _bn_tensors(bn), fold)


def conv_bx_dual_supported(conv_a, xa, conv_b, xb):
    """Two 1x1 stride-1 convolutions with the same output channels on inputs of the same plane (conv3 and a stride-1 downsample of a
    Bottleneck), both shapes the split-bf16 kernel takes."""
    for conv, x in ((conv_a, xa), (conv_b, xb)):
        if conv.kernel_size != (1, 1) or conv.stride != (1, 1) or not conv_bx_supported(conv, x):
            return False
    return conv_a.out_channels == conv_b.out_channels and xa.shape[0] == xb.shape[0] and xa.shape[2:] == xb.shape[2:]


def conv_bx_dual(conv_a, bn_a, xa, conv_b, bn_b, xb, relu=True):
    """relu?(bn_a(conv_a(xa)) + bn_b(conv_b(xb))) in ONE kernel at inference (mas_conv_bx_fwd_dual): both BatchNorm scales folded into
    the weight images, one accumulator set walks the channels of xa, then those of xb -- `out = relu(bn3(conv3(out)) + downsample(x))`
    of models/segmentation/backbone/resnet.py:143-160 without writing the identity branch to memory."""
    xa, xb = xa.contiguous(), xb.contiguous()
    N, Ka, H, W = xa.shape
    M = conv_a.out_channels
    def fold():
        # the two folded images and the sum of their shifts (three ATen launches per call if it were not kept)
        (wa, sa), (wb, sb) = _conv_bx_folded(conv_a, bn_a), _conv_bx_folded(conv_b, bn_b)
        return wa, wb, (sa.double() + sb.double()).float()
    wa, wb, shift = _cached(conv_a, '_mas_conv_bx_dual', (conv_a.weight,) + _bn_tensors(bn_a) + (conv_b.weight,) + _bn_tensors(bn_b), fold)
    y = torch.empty((N, M, H, W), dtype=torch.float32, device=xa.device)
    with torch.cuda.device(xa.device):
        _lib.check(_lib.load().mas_conv_bx_fwd_dual(xa.data_ptr(), wa.data_ptr(), Ka, xb.data_ptr(), wb.data_ptr(), xb.shape[1], N, H, W, M,
                                                    shift.data_ptr(), int(relu), y.data_ptr(), _stream(xa)), "mas_conv_bx_fwd_dual")
    return y


def conv_bx(conv, x, bn=None, relu=False, residual=None):
    """relu?(bn(conv(x)) + residual) in one kernel on the bf16 matrix cores with f32 operands and results (see conv_mfma)."""
    x = x.contiguous()
    N, K, H, W = x.shape
    M = conv.out_channels
    ks, s, d = conv.kernel_size[0], conv.stride[0], conv.dilation[0]
    wp = _conv_bx_weight(conv)
    scale, shift, res, y = _fused_epilogue(bn, residual, (N, M, (H - 1) // s + 1, (W - 1) // s + 1), x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mas_conv_bx_fwd(x.data_ptr(), wp.data_ptr(), N, K, H, W, M, ks, s, d, _opt(scale), _opt(shift), _opt(res),
                                               int(relu), y.data_ptr(), _stream(x)), "mas_conv_bx_fwd")
    return y


class Bx3:
    """An activation tensor in presplit form (mas_bx3_split / an OUT3 epilogue): ``data`` int16 [N, ceil(C/8), 3, H*W, 8] (bf16 bits),
    ``shape`` = the (N, C, H, W) of the f32 tensor it stands for."""
    __slots__ = ("data", "shape")

    def __init__(self, data, shape):
        self.data, self.shape = data, tuple(shape)


def bx3_split(x):
    """The presplit form of x [N,C,H,W] f32 as a pass of its own (csrc/conv_bx.hip:k_bx3_split)."""
    _need(x, "x", torch.float32)
    N, C, H, W = x.shape
    data = torch.empty((N, (C + 7) // 8, 3, H * W, 8), dtype=torch.int16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mas_bx3_split(x.data_ptr(), N, C, H, W, data.data_ptr(), _stream(x)), "mas_bx3_split")
    return Bx3(data, x.shape)


def conv_bx_pre(conv, x3, bn=None, relu=False, residual=None):
    """conv_bx on a presplit input (stride 1): the same products and the same bits as conv_bx(conv, x, ...) on the f32 tensor."""
    N, K, H, W = x3.shape
    M = conv.out_channels
    ks, s, d = conv.kernel_size[0], conv.stride[0], conv.dilation[0]
    if s != 1 or K != conv.in_channels:
        raise ValueError("conv_bx_pre: stride-1 convolutions on a presplit tensor of their input channels")
    wp = _conv_bx_weight(conv)
    scale, shift, res, y = _fused_epilogue(bn, residual, (N, M, H, W), x3.data.device, strict=False)
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().mas_conv_bx_fwd_pre(x3.data.data_ptr(), wp.data_ptr(), N, K, H, W, M, ks, d, _opt(scale), _opt(shift), _opt(res),
                                                   int(relu), y.data_ptr(), _stream(y)), "mas_conv_bx_fwd_pre")
    return y


def stem_conv_supported(conv, x):
    """The deep stem's first convolution (3 -> C, 3x3, stride 2, padding 1) on csrc/stem.hip: fp32 NCHW, W % 8 == 0."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and conv.in_channels == 3
            and conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.out_channels % 16 == 0 and x.shape[3] % 8 == 0
            and x.shape[0] * (conv.out_channels // 16) <= 65535)


def stem_conv(conv, x, bn=None, relu=False):
    """relu?(bn(conv(x))) for the stem's first convolution in one kernel (inference)."""
    x = x.contiguous()
    N, _, H, W = x.shape
    M = conv.out_channels
    scale, shift, _, y = _fused_epilogue(bn, None, (N, M, (H - 1) // 2 + 1, (W - 1) // 2 + 1), x.device, strict=False)
    w = conv.weight.detach().contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mas_stem_conv_fwd(x.data_ptr(), w.data_ptr(), N, H, W, M, _opt(scale), _opt(shift), int(relu), y.data_ptr(),
                                                 _stream(x)), "mas_stem_conv_fwd")
    return y


# ------------------------------------------------------------------------------------------------
# training-mode dense convolutions: forward and input gradient on the persistent stream-K kernel (csrc/conv_sk.hip), weight
# gradient on the split-K kernel (csrc/conv_wgrad.hip), all on the f32 matrix cores -- no MIOpen, no NCHW <-> NHWC copies
# ------------------------------------------------------------------------------------------------
_WGRAD_WS = {}


def _wgrad_workspace(dev, nbytes):
    """One split-K workspace per (device, stream), grown on demand (the kernels of one stream run in order, so consecutive weight
    gradients can share it; the weight gradients of a backward pass run on a side stream, _ConvTrain.backward)."""
    return _stream_scratch(_WGRAD_WS, dev, lambda: torch.empty(int(nbytes), dtype=torch.uint8, device=dev), nbytes)


def conv_wgrad(x, dy, ksize, stride, dil):
    """dW [Cout,Cin,k,k] of y = conv2d(x, W, stride, padding = dil (k = 3) / 0 (k = 1), dilation) from x [N,Cin,H,W] and
    dy [N,Cout,Ho,Wo] (mas_conv_wgrad: split-K over the pixels, fixed-order reduction)."""
    _need(x, "x", torch.float32)
    _need(dy, "dy", torch.float32)
    N, Cin, H, W = x.shape
    Cout = dy.shape[1]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if tuple(dy.shape) != (N, Cout, Ho, Wo):
        raise ValueError("dy %s does not match x %s under stride %d" % (tuple(dy.shape), tuple(x.shape), stride))
    lib = _lib.load()
    bx, r04 = _train_bx()
    if (ksize == 1 and stride == 1 and bx and Cout >= 96 and Cin >= 64
            and lib.mas_conv_wgrad_bx_supported(N, Cin, H, W, Cout)):
        # 1x1: split-bf16 kernel (csrc/conv_wgrad_bx.hip), 1.3-1.7x the f32 kernel (profiles/r04/k_bx_train_table.md); with 64 or
        # fewer output channels half of its 128 x 128 tile is padding and the f32 kernel stays ahead
        return conv_wgrad_bx(x, dy)
    if (ksize == 1 and stride == 2 and bx and not r04 and Cout >= 96 and Cin >= 64
            and lib.mas_conv_wgrad_bx_supported(N, Cin, Ho, Wo, Cout)):
        # 1x1 stride 2 (`downsample`): dW only sees the even pixels of x -- gather them once (a quarter of x, one strided copy) and the
        # product is the stride-1 one on the small plane (the f32 kernel's strided K axis ran at 29 TFLOP/s: 168 us per layer)
        return conv_wgrad_bx(x[:, :, ::2, ::2].contiguous(), dy)
    w3 = os.environ.get("MAS_WGRAD3", "auto")
    if (ksize == 3 and stride == 1 and bx and not r04 and w3 != "f32"
            and lib.mas_conv_wgrad_bx3_supported(N, Cin, H, W, Cout, dil)):
        # 3x3 stride 1: split-bf16 kernel with the X patch read through gfx950's transposing LDS read (csrc/conv_wgrad_bx3.hip)
        return conv_wgrad_bx3(x, dy, dil)
    nbytes = lib.mas_conv_wgrad_workspace_bytes(N, Cin, H, W, Cout, ksize, stride, dil)
    if nbytes == 0:
        raise ValueError("unsupported convolution geometry for mas_conv_wgrad")
    ws = _wgrad_workspace(x.device, nbytes)
    dw = torch.empty((Cout, Cin, ksize, ksize), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.mas_conv_wgrad(x.data_ptr(), dy.data_ptr(), N, Cin, H, W, Cout, ksize, stride, dil, dw.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _stream(x)), "mas_conv_wgrad")
    return dw


def _conv_wgrad_bx(x, dy, ks, dil):
    """The split-bf16 weight gradient of a stride-1 convolution: mas_conv_wgrad_bx (1x1) / mas_conv_wgrad_bx3 (3x3, which alone takes
    a dilation)."""
    _need(x, "x", torch.float32)
    _need(dy, "dy", torch.float32)
    N, Cin, H, W = x.shape
    Cout = dy.shape[1]
    if tuple(dy.shape) != (N, Cout, H, W):
        raise ValueError("dy %s does not match x %s" % (tuple(dy.shape), tuple(x.shape)))
    lib = _lib.load()
    name, geom, extra = ("mas_conv_wgrad_bx", (), "") if ks == 1 else ("mas_conv_wgrad_bx3", (dil,), ", dilation %d" % dil)
    if not getattr(lib, name + "_supported")(N, Cin, H, W, Cout, *geom):
        raise ValueError("unsupported geometry for %s: x %s%s" % (name, tuple(x.shape), extra))
    ws = _wgrad_workspace(x.device, getattr(lib, name + "_workspace_bytes")(Cin, Cout))
    dw = torch.empty((Cout, Cin, ks, ks), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(getattr(lib, name)(x.data_ptr(), dy.data_ptr(), N, Cin, H, W, Cout, *[int(d) for d in geom], dw.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream(x)), name)
    return dw


def conv_wgrad_bx(x, dy):
    """dW [Cout,Cin,1,1] of a 1x1 stride-1 convolution from x [N,Cin,H,W] and dy [N,Cout,H,W] on the bf16 matrix cores with exact
    three-term splits of both f32 operands (mas_conv_wgrad_bx: split-K over the pixels, fixed-order reduction)."""
    return _conv_wgrad_bx(x, dy, 1, None)


def conv_wgrad_bx3(x, dy, dil=1):
    """dW [Cout,Cin,3,3] of a 3x3 stride-1 convolution (padding = dilation = 1 | 2) from x [N,Cin,H,W] and dy [N,Cout,H,W] on the bf16
    matrix cores with exact three-term splits of both f32 operands (mas_conv_wgrad_bx3: the X patch staged channel-contiguous as the
    forward kernel stages it, read with ds_read_b64_tr_b16; split-K over chunks of 4 x 16 pixels, fixed-order reduction)."""
    return _conv_wgrad_bx(x, dy, 3, dil)


_SK_WS = {}


def _sk_workspace(dev):
    """(workspace, epoch) of the stream-K convolution for the current stream of `dev`: partial-tile slots + epoch flags, zero-filled
    once; launches of one stream run in order and may share it, the epoch differs from launch to launch."""
    ent = _stream_scratch(_SK_WS, dev, lambda: [torch.zeros(int(_lib.load().mas_conv_sk_workspace_bytes()), dtype=torch.uint8, device=dev), 0])
    ent[1] = ent[1] % 0xfffffff0 + 1
    return ent[0], ent[1]


def conv_sk_pack(w, stride=1, dgrad=False):
    """The weight [Cout,Cin,k,k] as mas_conv_sk reads it for one role (one small launch): dgrad False / 0 forward, True / 1 input
    gradient at stride 1, 2 + sub the parity class `sub` of the input gradient of a 3x3 stride-2 convolution."""
    _need(w, "w", torch.float32)
    Cout, Cin, ks, _ = w.shape
    lib = _lib.load()
    out = torch.empty(int(lib.mas_conv_sk_packed_elems(Cin, Cout, ks, stride, int(dgrad))), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(lib.mas_conv_sk_pack(w.data_ptr(), Cin, Cout, ks, stride, int(dgrad), out.data_ptr(), _stream(w)), "mas_conv_sk_pack")
    return out


class _PackRegistry:
    """Packed weight images of one device, re-packed together: the first use of a (weight, role) packs it alone; when a lookup
    finds a weight whose version counter or the process's parameter epoch moved (an optimizer stepped), ONE launch (mas_conv_sk_pack_multi) re-packs every
    registered image -- the optimizer updates all of them together -- instead of two small launches per convolution and step.
    Entries hold the weight WEAKLY: the active-learning loop builds a new trainer and model every round (reference train_AL.py:38),
    and a registry that kept the old weights alive would pin every dead model's convolution weights and images in HBM and re-pack
    them after every optimizer step.  An entry dies with its weight (finalizer), and dead entries never reach the job table."""

    def __init__(self, dev):
        self.dev = dev
        self.entries = {}           # key -> [weakref to the weight, image, (version, parameter epoch)]
        self.table = None           # device copy of the job records
        self.nblocks = 0
        self.njobs = 0

    @staticmethod
    def key(w, stride, dgrad):
        return (w.data_ptr(), w.untyped_storage()._cdata, tuple(w.shape), int(stride), int(dgrad))

    def _drop(self, k):
        self.entries.pop(k, None)
        self.table = None           # (its records point into freed memory)

    def get(self, w, stride, dgrad):
        import weakref
        k = self.key(w, stride, dgrad)
        e = self.entries.get(k)
        if e is not None and e[0]() is None:        # the address was recycled by a new tensor before the finalizer ran
            self._drop(k)
            e = None
        if e is None:
            img = self._pack_one(w, stride, dgrad)
            self.entries[k] = [weakref.ref(w), img, (w._version, _PARAM_EPOCH[0])]
            weakref.finalize(w, self._drop, k)
            self.table = None
            return img
        if e[2] != (w._version, _PARAM_EPOCH[0]):
            self.repack_all()
        return e[1]

    def repack_all(self):
        import ctypes
        lib = _lib.load()
        live = [(k, e, e[0]()) for k, e in list(self.entries.items())]
        for k, e, w in live:
            if w is None:
                self._drop(k)
        live = [(k, e, w) for k, e, w in live if w is not None]
        if not live:
            return
        if self.table is None:
            rec = self._job_bytes(lib)
            host = ctypes.create_string_buffer(rec * len(live))
            base = ctypes.addressof(host)
            first = 0
            for i, (k, e, w) in enumerate(live):
                n = self._fill_job(lib, base + i * rec, w, k, e[1], first)
                if n == 0:
                    raise _lib.MulActSegHipError("%s rejected the pack job %s" % (type(self).__name__, k))
                first += n
            self.table = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(self.dev)
            self.nblocks = first
            self.njobs = len(live)
        with torch.cuda.device(self.dev):
            self._multi(lib, torch.cuda.current_stream(self.dev).cuda_stream)
        for k, e, w in live:
            e[2] = (w._version, _PARAM_EPOCH[0])

    # the image format of this registry: mas_conv_sk (a subclass: mas_conv_bx)
    @staticmethod
    def _pack_one(w, stride, dgrad):
        return conv_sk_pack(w, stride, dgrad)

    @staticmethod
    def _job_bytes(lib):
        return int(lib.mas_conv_sk_pack_job_bytes())

    @staticmethod
    def _fill_job(lib, rec, w, k, img, first):
        return lib.mas_conv_sk_pack_job(rec, w.data_ptr(), w.shape[1], w.shape[0], w.shape[2], k[3], int(k[4]), img.data_ptr(), first)

    def _multi(self, lib, stream):
        _lib.check(lib.mas_conv_sk_pack_multi(self.table.data_ptr(), self.njobs, self.nblocks, stream), "mas_conv_sk_pack_multi")


def conv_bx_pack(w, role=0, row_scale=None):
    """The split-bf16 weight image of mas_conv_bx_pack for one role (0 forward, 1 input gradient at stride 1); ``row_scale`` [Cout]
    (role 0): every output channel's weights multiplied by its entry before the split (a folded BatchNorm scale)."""
    _need(w, "w", torch.float32)
    w = w.contiguous()
    if row_scale is not None:
        _need(row_scale, "row_scale", torch.float32)
        if row_scale.numel() != w.shape[0] or role != 0:
            raise ValueError("row_scale: %d entries for %d output channels (role %d)" % (row_scale.numel(), w.shape[0], role))
        row_scale = row_scale.contiguous()
    M, K, kh, _ = w.shape
    lib = _lib.load()
    nbytes = lib.mas_conv_bx_packed_bytes(kh, K, M, int(role))
    if nbytes <= 0:
        raise ValueError("mas_conv_bx_pack does not take a %dx%d weight %s" % (kh, kh, tuple(w.shape)))
    wp = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(lib.mas_conv_bx_pack(w.data_ptr(), _opt(row_scale), M, K, kh, int(role), wp.data_ptr(), _stream(w)), "mas_conv_bx_pack")
    return wp


class _BxPackRegistry(_PackRegistry):
    """The same bookkeeping for the split-bf16 images of csrc/conv_bx.hip (key: stride is always 1, `dgrad` is the role)."""

    @staticmethod
    def _pack_one(w, stride, dgrad):
        return conv_bx_pack(w, int(dgrad))

    @staticmethod
    def _job_bytes(lib):
        return int(lib.mas_conv_bx_pack_job_bytes())

    @staticmethod
    def _fill_job(lib, rec, w, k, img, first):
        return lib.mas_conv_bx_pack_job(rec, w.data_ptr(), w.shape[0], w.shape[1], w.shape[2], int(k[4]), img.data_ptr(), first)

    def _multi(self, lib, stream):
        _lib.check(lib.mas_conv_bx_pack_multi(self.table.data_ptr(), self.njobs, self.nblocks, stream), "mas_conv_bx_pack_multi")


_PACKS = {}
_BX_PACKS = {}


def bx_packed_weight(w, role=0):
    """The mas_conv_bx image of weight `w` for one role, kept up to date across optimizer steps (one re-pack launch per step for
    all registered weights: _BxPackRegistry)."""
    reg = _BX_PACKS.get(w.device)
    if reg is None:
        reg = _BX_PACKS[w.device] = _BxPackRegistry(w.device)
    return reg.get(w, 1, int(role))


_BX_WS = {}


def _bx_workspace(dev, nbytes):
    """Per-(device, stream) scratch for the partial tiles of a split-K mas_conv_bx_train launch (grown on demand, never shrunk; the
    launches of one stream run in order, so they can share it)."""
    return _stream_scratch(_BX_WS, dev, lambda: torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=dev), nbytes)


def conv_bx_train_plan(x_shape, w_shape, dil=1, dgrad=False):
    """(ksplit, tile_w, workgroups) mas_conv_bx_train would choose for this product (mas_conv_bx_train_plan)."""
    import ctypes
    Cout, Cin, ks, _ = w_shape
    K, M = (Cout, Cin) if dgrad else (Cin, Cout)
    N, _, H, W = x_shape
    out = (ctypes.c_int * 3)()
    _lib.check(_lib.load().mas_conv_bx_train_plan(N, K, H, W, M, ks, dil, out), "mas_conv_bx_train_plan")
    return int(out[0]), int(out[1]), int(out[2])


def conv_bx_s2_raw(x, w, packed=None):
    """y = conv2d(x, w, stride 2[, padding 1]) for a 1x1 or 3x3 weight on the stride-2 form of csrc/conv_bx.hip (bare product of a
    training step).  packed: the image of role 0 (1x1) / BX_ROLE_S2 (3x3)."""
    _need(x, "x", torch.float32)
    _need(w, "w", torch.float32)
    Cout, Cin, ks, _ = w.shape
    N, Cx, H, W = x.shape
    if ks not in (1, 3) or Cx != Cin:
        raise ValueError("conv_bx_s2_raw: a 1x1 or 3x3 weight on its input channels")
    y = torch.empty((N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    if packed is None:
        packed = conv_bx_pack(w, 0 if ks == 1 else BX_ROLE_S2)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mas_conv_bx_fwd(x.data_ptr(), packed.data_ptr(), N, Cin, H, W, Cout, ks, 2, 1, None, None, None, 0, y.data_ptr(),
                                               _stream(x)), "mas_conv_bx_fwd")
    return y


def conv_bx_raw(x, w, dil=1, dgrad=False, residual=None, packed=None, ksplit=0, tile_w=0, stats=False):
    """The bare stride-1 product of a training step on csrc/conv_bx.hip: dgrad False: y = conv2d(x, w, padding = dil (k 3) / 0 (k 1),
    dilation); dgrad True: x is dY [N,Cout,H,W] and the result dX [N,Cin,H,W] (+ residual: the gradient of x's other consumer).
    ksplit / tile_w: 0 = the library's work-splitting plan (mas_conv_bx_train_plan); explicit values for sweeps and tests.
    stats=True (forward, no residual): returns (y, partials) -- partials [Cout, slots, 2] float64, the BatchNorm partial sums
    (sum y, sum y^2 over disjoint pixel sets) formed in the kernel's epilogue (ksplit 1) or by the reduction pass of a split-K plan, or
    None where neither can (split K on a plane of odd size).
    Operands must be finite and within 2^-100 < |v| < 2^127 (csrc/bx_split.h): an Inf operand yields NaN where the f32 pipe would
    propagate Inf (h = Inf, m = Inf - Inf), NaN stays NaN, values below 2^-100 lose their third term (relative error <= 2^-16)."""
    _need(x, "x", torch.float32)
    _need(w, "w", torch.float32)
    Cout, Cin, ks, _ = w.shape
    N, Cx, H, W = x.shape
    K, M = (Cout, Cin) if dgrad else (Cin, Cout)
    if Cx != K:
        raise ValueError("input has %d channels, weight %s (dgrad=%s)" % (Cx, tuple(w.shape), dgrad))
    y = torch.empty((N, M, H, W), dtype=torch.float32, device=x.device)
    if residual is not None:
        _need(residual, "residual", torch.float32)
        if residual.shape != y.shape:
            raise ValueError("residual %s does not match the output %s" % (tuple(residual.shape), tuple(y.shape)))
    if packed is None:
        packed = conv_bx_pack(w, int(dgrad))
    lib = _lib.load()
    if not ksplit or not tile_w:
        plan = conv_bx_train_plan(x.shape, w.shape, dil, dgrad)
        ksplit = ksplit or plan[0]
        tile_w = tile_w or plan[1]
        cap = os.environ.get("MAS_BX_KSPLIT_DGRAD" if dgrad else "MAS_BX_KSPLIT_FWD")       # (A/B: cap the plan's K split)
        if cap:
            ksplit = max(1, min(ksplit, int(cap)))
    if ksplit > 1 and (y.numel() % 4 != 0):
        ksplit = 1                                   # (the reduction pass walks 16-byte groups)
    ws = part = None
    with torch.cuda.device(x.device):
        if ksplit > 1:
            ws = _bx_workspace(x.device, int(lib.mas_conv_bx_train_workspace_bytes(N, M, H, W, ksplit)))
        if stats and not dgrad and residual is None:
            slots = int(lib.mas_conv_bx_train_stat_slots(N, H, W, M, ks, dil, int(ksplit), int(tile_w)))
            if slots > 0:
                part = torch.empty((M, slots, 2), dtype=torch.float64, device=x.device)
        _lib.check(lib.mas_conv_bx_train(x.data_ptr(), packed.data_ptr(), N, K, H, W, M, ks, dil, _opt(residual), y.data_ptr(), int(ksplit),
                                         int(tile_w), _opt(ws), ws.numel() if ws is not None else 0, _opt(part), _stream(x)), "mas_conv_bx_train")
    return (y, part) if stats else y


def conv_bx_train_ok(x_shape, w_shape, stride, dil, dgrad):
    """Does the split-bf16 kernel take this product of a training step?  Stride 1 only.  MAS_TRAIN_BX = auto (default): every
    supported stride-1 product -- launches with fewer workgroups than the chip has slots (the 48 x 48 planes) split their K chunks
    over several workgroups and use 16 x 16 pixel tiles (mas_conv_bx_train_plan; profiles/r05/k_bx_train_table.md); r04: round 4's
    rule (1x1 everywhere, 3x3 on planes of at least 96 x 96 or with at least 320 tiles -- the others on the persistent stream-K
    kernel), for A/B runs; off: never."""
    bx, r04 = _train_bx()
    Cout, Cin, ks, _ = w_shape
    N, _, H, W = x_shape
    if bx and not r04 and stride == 2 and not dgrad and (ks == 1 or (ks == 3 and dil == 1 and _bx_s2k3())):
        # the 1x1 stride-2 `downsample` convolutions (resnet.py:215-223) and the 3x3 stride-2 conv2 of layer2.0 / layer3.0 (:140-150):
        # the stride-2 form of the forward kernel (planes with even H and W % 8 == 0 -- the 768 crop; the 769 crop's odd planes stay
        # on the stream-K kernel)
        if not (_lib.load().mas_conv_bx_supported(ks, 2, 1, Cin, Cout, H, W) and x_shape[0] > 0):
            return False
        # (the strided 3x3 has no work splitting: below 256 workgroups -- layer3.0.conv2 on the 48 x 48 planes of the training crop,
        #  144 of them with 72 chunks each -- the persistent stream-K kernel is faster: 114 against 142 us, tools/s2k3_probe.py)
        bm = 128 if Cout % 128 == 0 else 64
        wgs = (N * (H // 2) * (W // 2) + (16384 // bm) - 1) // (16384 // bm) * ((Cout + bm - 1) // bm)      # (pixel tile: 128 / 256)
        return ks == 1 or wgs >= 256
    if not bx or stride != 1:
        return False
    K, M = (Cout, Cin) if dgrad else (Cin, Cout)
    if not _lib.load().mas_conv_bx_supported(ks, 1, dil, K, M, H, W):
        return False
    if not r04 or ks == 1 or H * W >= 96 * 96:
        return True
    return N * ((H + 7) // 8) * ((W + 31) // 32) * ((M + 63) // 64) >= 320


def packed_weight(w, stride=1, dgrad=False):
    """The mas_conv_sk image of weight `w` for one role, kept up to date across optimizer steps (see _PackRegistry)."""
    reg = _PACKS.get(w.device)
    if reg is None:
        reg = _PACKS[w.device] = _PackRegistry(w.device)
    return reg.get(w, stride, dgrad)


_SK_DEFAULT_FLAGS = [0]         # wrapper default of the per-call mas_sk_opts.flags (conv_sk_set_mode: A/B runs of the LDS-DMA ring)


def sk_split_default():
    """Does a conv_sk call without explicit flags split tiles over workgroups (the stream-K hand-off)?  MAS_SK_SPLIT = auto
    (default): yes in a single-GPU process, NO under torch.distributed with more than one rank -- the hand-off assumes that the
    workgroups of a launch become resident together, which a neighbour holding CUs for seconds (an RCCL kernel of a wedged peer,
    another tenant) can break; a finisher that gives up poisons its tile and the step aborts (trainer/base.py:raise_stream_k),
    and one rank aborting while the others sit in the gradient all-reduce is a hang.  The whole-tile plan (SK_NOSPLIT) has no
    hand-off and is exact; it costs the load balance of the few layers that still run on k_conv_sk.
    on / off force either."""
    mode = os.environ.get("MAS_SK_SPLIT", "auto")
    if mode in ("on", "1"):
        return True
    if mode in ("off", "0"):
        return False
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)


def _sk_opts(flags=None, spin_limit=0, stamps=None):
    """mas_sk_opts for one call (NULL when everything is the default)."""
    import ctypes
    if flags is None:
        flags = _SK_DEFAULT_FLAGS[0] | (0 if sk_split_default() else _lib.SK_NOSPLIT)
    flags = int(flags)
    if not flags and not spin_limit and stamps is None:
        return None, flags
    o = _lib.SkOpts(flags, int(spin_limit), stamps.data_ptr() if stamps is not None else None)
    return ctypes.byref(o), flags


def conv_sk(x, w, stride=1, dil=1, dgrad=False, scale=None, shift=None, residual=None, relu=False, packed=None, stats=False,
            flags=None, spin_limit=0, stamps=None):
    """Training-mode dense convolution on the persistent stream-K MFMA kernel (mas_conv_sk), weight `w` [Cout,Cin,k,k] as PyTorch
    stores it (``packed``: its conv_sk_pack image for this role, when the caller keeps one).  dgrad=False: y = conv2d(x, w, stride, padding = dil (k 3) / 0 (k 1), dilation); dgrad=True: x is dY [N,Cout,H,W] and
    the result is dX [N,Cin,H,W] of the stride-1 convolution.  Optional epilogue y*scale[m] + shift[m] + residual, ReLU.
    ``flags`` (_lib.SK_DMA | _lib.SK_NOSPLIT), ``spin_limit``, ``stamps``: the per-call mas_sk_opts."""
    _need(x, "x", torch.float32)
    _need(w, "w", torch.float32)
    Cout, Cin, ks, _ = w.shape
    N, Cx, H, W = x.shape
    if Cx != (Cout if dgrad else Cin):
        raise ValueError("input has %d channels, weight %s (dgrad=%s)" % (Cx, tuple(w.shape), dgrad))
    M = Cin if dgrad else Cout
    Ho, Wo = (H, W) if dgrad else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    y = torch.empty((N, M, Ho, Wo), dtype=torch.float32, device=x.device)
    if residual is not None:
        _need(residual, "residual", torch.float32)
        if residual.shape != y.shape:
            raise ValueError("residual %s does not match the output %s" % (tuple(residual.shape), tuple(y.shape)))
    for t, name in ((scale, "scale"), (shift, "shift")):
        if t is not None:
            _need(t, name, torch.float32)
            if t.numel() != M:
                raise ValueError("%s must have %d entries" % (name, M))
    if packed is None:
        packed = conv_sk_pack(w, stride, dgrad)
    ws, epoch = _sk_workspace(x.device)
    lib = _lib.load()
    opts, flags = _sk_opts(flags, spin_limit, stamps)
    if stats:
        # forward without epilogue + the BatchNorm partial sums of y from the epilogue of every tile: (y, partials [Cout, slots, 2] f64)
        if dgrad or scale is not None or residual is not None or relu:
            raise ValueError("stats=True: bare forward product only")
        slots = int(lib.mas_conv_sk_stats_slots(N, Cin, H, W, Cout, ks, stride, dil, flags))
        if slots <= 0:
            raise ValueError("unsupported geometry for mas_conv_sk_stats")
        part = torch.empty((Cout, slots, 2), dtype=torch.float64, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.mas_conv_sk_stats(x.data_ptr(), packed.data_ptr(), N, Cin, H, W, Cout, ks, stride, dil, y.data_ptr(), part.data_ptr(),
                                             ws.data_ptr(), ws.numel(), epoch, opts, _stream(x)), "mas_conv_sk_stats")
        return y, part
    with torch.cuda.device(x.device):
        _lib.check(lib.mas_conv_sk(x.data_ptr(), packed.data_ptr(), N, Cin, H, W, Cout, ks, stride, dil, int(dgrad), _opt(scale), _opt(shift),
                                   _opt(residual), int(relu), y.data_ptr(), ws.data_ptr(), ws.numel(), epoch, opts, _stream(x)),
                   "mas_conv_sk")
    return y


def _dgrad_s2_operands(dy, w, H, W, ks):
    """(N, Cin, Cout) of the input gradient of a ks x ks stride-2 convolution of an H x W plane, its operands checked."""
    _need(dy, "dy", torch.float32)
    _need(w, "w", torch.float32)
    Cout, Cin, k, _ = w.shape
    N = dy.shape[0]
    if k != ks or tuple(dy.shape) != (N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise ValueError("dy %s does not belong to a %dx%d stride-2 convolution of a %dx%d plane with weight %s"
                         % (tuple(dy.shape), ks, ks, H, W, tuple(w.shape)))
    return N, Cin, Cout


def conv_sk_dgrad_s2(dy, w, H, W, packed=None, flags=None, spin_limit=0):
    """dX [N,Cin,H,W] of y = conv2d(x, w, stride 2, padding 1) for a 3x3 weight `w` [Cout,Cin,3,3] from dY [N,Cout,(H-1)//2+1,
    (W-1)//2+1]: four launches of the stream-K kernel, one per parity class of the dX pixels (mas_conv_sk_dgrad_s2) -- each a
    stride-1 product over the dY plane with 1 / 2 / 2 / 4 taps, together the exact FLOPs of the gradient (no zero insertion).
    ``packed``: the four class images (conv_sk_pack(w, 2, 2 + sub))."""
    N, Cin, Cout = _dgrad_s2_operands(dy, w, H, W, 3)
    dx = torch.empty((N, Cin, H, W), dtype=torch.float32, device=dy.device)
    lib = _lib.load()
    opts, _ = _sk_opts(flags, spin_limit)
    with torch.cuda.device(dy.device):
        for sub in range(4):
            img = packed[sub] if packed is not None else conv_sk_pack(w, 2, 2 + sub)
            ws, epoch = _sk_workspace(dy.device)
            _lib.check(lib.mas_conv_sk_dgrad_s2(dy.data_ptr(), img.data_ptr(), N, Cin, H, W, Cout, sub, None, None, None, 0, dx.data_ptr(),
                                                ws.data_ptr(), ws.numel(), epoch, opts, _stream(dy)), "mas_conv_sk_dgrad_s2")
    return dx


def conv_sk_dgrad_1x1s2(dy, w, H, W, packed=None):
    """dX [N,Cin,H,W] of y = conv2d(x, w, stride 2) for a 1x1 weight `w` [Cout,Cin,1,1] from dY [N,Cout,(H-1)//2+1,(W-1)//2+1]: the
    gradient lives on the even positions only.  ONE launch of the stream-K kernel: the stride-1 product over the dY plane with the
    strided store of the stride-2 parity classes (class 0 of mas_conv_sk_dgrad_s2 is exactly a one-tap product written to the pixels
    (2i, 2j); it takes the 1x1 weight's input-gradient image) into a zero-filled dX.  (Until round 4: the product into a temporary,
    then zeros_like + a strided ATen copy.)"""
    N, Cin, Cout = _dgrad_s2_operands(dy, w, H, W, 1)
    dx = torch.zeros((N, Cin, H, W), dtype=torch.float32, device=dy.device)
    img = packed if packed is not None else conv_sk_pack(w, 1, True)
    lib = _lib.load()
    opts, _ = _sk_opts()
    ws, epoch = _sk_workspace(dy.device)
    with torch.cuda.device(dy.device):
        _lib.check(lib.mas_conv_sk_dgrad_s2(dy.data_ptr(), img.data_ptr(), N, Cin, H, W, Cout, 0, None, None, None, 0, dx.data_ptr(),
                                            ws.data_ptr(), ws.numel(), epoch, opts, _stream(dy)), "mas_conv_sk_dgrad_s2")
    return dx


def conv_sk_set_mode(dma):
    """Default chunk staging of this wrapper's conv_sk calls (the library itself keeps no mode: the flag travels with every call in
    mas_sk_opts): False = register-staged (default), True = LDS-DMA ring; returns the previous default.  For A/B runs and tests."""
    old = bool(_SK_DEFAULT_FLAGS[0] & _lib.SK_DMA)
    _SK_DEFAULT_FLAGS[0] = (_SK_DEFAULT_FLAGS[0] & ~_lib.SK_DMA) | (_lib.SK_DMA if dma else 0)
    return old


def conv_sk_error(dev=None):
    """Non-zero when a stream-K launch on the current stream's workspace gave up waiting for another workgroup (synchronises)."""
    import ctypes
    dev = torch.device('cuda', torch.cuda.current_device()) if dev is None else dev
    ent = _SK_WS.get(_stream_key(dev))
    if ent is None:
        return 0
    torch.cuda.synchronize(dev)
    out = ctypes.c_uint(0)
    _lib.check(_lib.load().mas_conv_sk_error(ent[0].data_ptr(), ctypes.byref(out)), "mas_conv_sk_error")
    return int(out.value)


def _cuda_dev(dev):
    dev = torch.device('cuda', torch.cuda.current_device()) if dev is None else torch.device(dev)
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def _sk_error_views(dev):
    off = int(_lib.load().mas_conv_sk_workspace_bytes()) - 4096 + 512 * 4       # the word behind the 512 epoch flags
    return [ent[0][off:off + 4] for (d, _), ent in _SK_WS.items() if d == dev]


def conv_sk_error_words(dev=None):
    """The error words of every stream-K workspace of `dev` as ONE device tensor [n] int32 (gathered on the current stream, no
    synchronisation), or None when no stream-K launch has run there yet.  The words are sticky (a finisher that gives up ORs a bit
    in; nothing but conv_sk_clear_error clears it), so a caller may look at them late: the trainers ship them to the host with the
    loss of the NEXT step (trainer/active_joint_multi.py:_HostProbe) and raise StreamKGaveUp."""
    views = _sk_error_views(_cuda_dev(dev))
    return torch.cat(views).view(torch.int32) if views else None


def conv_sk_clear_error(dev=None):
    """Zero the error words of `dev` (after the caller has dealt with a reported give-up)."""
    for v in _sk_error_views(_cuda_dev(dev)):
        v.zero_()


class StreamKGaveUp(RuntimeError):
    """A stream-K convolution gave up waiting for another workgroup of its launch: the step's activations / gradients are poisoned
    (NaN).  Seen only when the GPU is shared with something that keeps CUs busy for seconds."""


_SIDE_STREAMS = {}      # device -> the side stream of MAS_WGRAD_STREAM=side


def _side_stream(dev):
    """The stream the weight gradients run on under MAS_WGRAD_STREAM=side (dW is a leaf of the backward graph; not the default:
    see _ConvTrain.backward)."""
    st = _SIDE_STREAMS.get(dev)
    if st is None:
        st = _SIDE_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return st


_BRANCH_STREAMS = {}


def branch_stream(dev, k):
    """Stream number k for an independent BRANCH of the network in a training step (the downsample path of a Bottleneck beside its
    conv1-conv2-conv3 chain, the ASPP branches, the decoder's low-level projection): most layers of the 48 x 48 / 96 x 96 planes
    launch fewer workgroups than the chip has slots, so two independent layers side by side finish sooner than one after the other.
    autograd replays every node's backward on the stream of its forward and orders the streams itself, so the backward pass of a
    branch overlaps the same way.  MAS_BRANCH_STREAMS=on; the DEFAULT IS OFF (None): the step gains 0.2 ms (23.95 -> 23.74 at the 768
    crop, same bits), but the autograd engine record_stream()s every gradient that crosses streams, and blocks freed with a recorded
    stream use cannot serve the next step's allocations while the host runs ahead of the device -- 1.7 hipMalloc calls per step in
    steady state, reserved memory 9.6 -> 16.6 GB (profiles/r06/wgrad_stream_ab.md).  A 1 % gain is not worth an allocator that
    never settles."""
    if os.environ.get("MAS_BRANCH_STREAMS", "off") != "on":
        return None
    key = (dev, int(k))
    st = _BRANCH_STREAMS.get(key)
    if st is None:
        st = _BRANCH_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


def run_on_branch(stream, fn, *tensors):
    """fn(*tensors) on `stream` (which first waits for the current stream: the inputs are ready there); the caller joins with
    join_branch(stream, outputs) before the outputs are used on the current stream."""
    cur = torch.cuda.current_stream(tensors[0].device)
    stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        out = fn(*tensors)
    # (no Tensor.record_stream -- see _ConvTrain.backward: the inputs are activations that live on until the backward pass, i.e. past
    #  join_branch, after which every free on the current stream is ordered behind the branch's reads; the outputs come from the branch
    #  stream's pool and their blocks are reused by that stream only after it has waited for the current stream again)
    return out


def join_branch(stream, *outputs):
    torch.cuda.current_stream(outputs[0].device).wait_stream(stream)


_JOIN_QUEUED = set()
_KEEP_UNTIL_JOIN = {}          # device -> [(x, dy), ...] of the weight gradients queued on the side stream in this backward pass


def _async_wgrad_ok(w):
    """The weight gradient may finish on the side stream after its autograd node has returned only if NOTHING reads it before the
    end-of-backward join: w.grad is None (AccumulateGrad then only stores the tensor; with a gradient buffer in place it adds on the
    main stream), no gradient hooks on w, and no data-parallel reducer (DistributedDataParallel copies / all-reduces a gradient the
    moment its AccumulateGrad node has run)."""
    if w.grad is not None or getattr(w, '_post_accumulate_grad_hooks', None) or getattr(w, '_backward_hooks', None):
        return False
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized())      # (any process group: a reducer hooks the AccumulateGrad nodes, not the tensors)


def _join_side(dev):
    """The main stream of `dev` waits for the weight gradients queued on the side stream."""
    _JOIN_QUEUED.discard(dev)
    torch.cuda.current_stream(dev).wait_stream(_side_stream(dev))
    _KEEP_UNTIL_JOIN.pop(dev, None)                 # (only now may the operands of the weight gradients be freed: see _ConvTrain.backward)


def _join_side_after_backward(dev):
    """Queue ONE callback per backward pass (torch.autograd's engine runs it when the pass has finished, before .backward() returns):
    the main stream waits for the side stream there."""
    if dev in _JOIN_QUEUED:
        return
    _JOIN_QUEUED.add(dev)
    torch.autograd.Variable._execution_engine.queue_callback(lambda: _join_side(dev))


def _aten_pad(ks, dil):
    return (dil, dil) if ks == 3 else (0, 0)


class _ConvTrain(torch.autograd.Function):
    """y = conv2d(x, w) with autograd.  ``own`` = (forward, input gradient, weight gradient) on this package's f32-MFMA kernels:
    forward and input gradient on the stream-K kernel k_conv_sk (it reads the weight as PyTorch stores it; the input gradient
    is the same kernel with the weight's channel axes swapped and the taps mirrored; stride 1), weight gradient on k_wgrad; a
    False entry takes MIOpen through ATen for that product.
    stats: also returns the BatchNorm partial sums of y (formed in the forward kernel's epilogue).  fork: also returns an alias of x
    for the OTHER consumer of x (the residual branch of a Bottleneck: models/segmentation/backbone/resnet.py:143-160): the gradient
    that arrives through the alias is added in the epilogue of the input-gradient kernel (its `residual` operand) instead of by a
    separate pass over both gradients (autograd's accumulation: 16 add kernels over ~1.1 GB per step)."""

    @staticmethod
    def forward(ctx, x, w, stride, dil, own, stats=False, fork=False):
        if _JOIN_QUEUED:                    # a backward pass that raised before its end-of-pass callback ran: join the side stream now
            for dev in list(_JOIN_QUEUED):
                _join_side(dev)
        x = x.contiguous()
        ks = w.shape[2]
        part = None
        with torch.no_grad():
            if own[0] and conv_bx_train_ok(x.shape, w.shape, stride, dil, False):
                # split-bf16 kernel (csrc/conv_bx.hip); the BatchNorm partial sums then come from the separate reduction pass
                if stride == 2:
                    y = conv_bx_s2_raw(x, w, packed=bx_packed_weight(w, 0 if w.shape[2] == 1 else BX_ROLE_S2))
                elif stats:
                    # (the BatchNorm partial sums from the kernel's epilogue / the split-K reduction pass)
                    y, part = conv_bx_raw(x, w, dil, packed=bx_packed_weight(w, 0), stats=True)
                else:
                    y = conv_bx_raw(x, w, dil, packed=bx_packed_weight(w, 0))
            elif own[0] and stats:
                y, part = conv_sk(x, w, stride, dil, packed=packed_weight(w, stride, False), stats=True)
            elif own[0]:
                y = conv_sk(x, w, stride, dil, packed=packed_weight(w, stride, False))
            else:
                y = torch.nn.functional.conv2d(x, w, None, stride, _aten_pad(ks, dil), dil)
        ctx.save_for_backward(x, w)
        ctx.geom = (ks, stride, dil, own)
        ctx.fork = bool(fork)
        if not stats and not fork:
            return y
        ctx.set_materialize_grads(False)            # (no zero-filled "gradient" of the partial sums in the backward)
        outs = [y]
        if stats:
            if part is not None:
                ctx.mark_non_differentiable(part)
            outs.append(part)
        if fork:
            outs.append(x.view_as(x))
        return tuple(outs)

    @staticmethod
    def backward(ctx, dy, *rest):
        x, w = ctx.saved_tensors
        ks, stride, dil, own = ctx.geom
        g_other = rest[-1] if (ctx.fork and rest) else None     # gradient of the alias = of the other consumer of x
        if dy is None:
            return g_other, None, None, None, None, None, None
        dy = dy.contiguous()
        dx = dw = None
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        side = None
        if need_dw and own[2]:
            main = torch.cuda.current_stream(x.device)
            # MAS_WGRAD_STREAM: main = one stream; side = dW on a second stream, joined behind the input gradient of the SAME layer
            # (round 3, persistent one-workgroup-per-CU kernels: 34.1 vs 32.4 ms; round 6, tile kernels: 27.2 vs 25.0 ms -- it loses
            # either way); async (the default where _async_wgrad_ok) = the second stream joined once per backward pass.
            mode = os.environ.get("MAS_WGRAD_STREAM", "async")
            if mode == "async" and not _async_wgrad_ok(w):
                mode = "main"
            if mode == "async" or (mode == "side" and need_dx):
                side = _side_stream(x.device)
                side.wait_stream(main)                      # dy (and x) are ready on the main stream
                with torch.cuda.stream(side):
                    dw = conv_wgrad(x, dy, ks, stride, dil)
                # Lifetimes across the two streams WITHOUT Tensor.record_stream: a block freed with a recorded stream use is held back
                # until an event has completed, and when the host runs ahead of the device (a step queues in 17 ms, runs in 23) those
                # held-back blocks cannot serve the next step's allocations -- the caching allocator then calls hipMalloc in steady
                # state (measured: 12-15 calls per step, reserved memory growing with the run-ahead depth, and on some boxes a 769 step
                # of 38 ms instead of 26).  Instead: x and dy are kept ALIVE until the join (a reference in _KEEP_UNTIL_JOIN), so their
                # blocks return to the main stream's pool only after the main stream has waited for the side stream; dW is allocated
                # from the side stream's pool, read by the optimizer behind the join, and its block is reused by the side stream only
                # after that stream has waited for the main stream again (the wait above, one step later).
                if mode == "async":
                    # dW is a LEAF of the backward graph: nothing downstream of this node reads it before the optimizer does.  The side
                    # stream is joined ONCE, when the whole backward pass has been queued (engine callback), so the weight gradients
                    # of all layers drain beside the chain of input gradients and BatchNorm backward passes -- most of whose launches
                    # leave CUs idle (144 workgroups of a 48 x 48 layer on 256 CUs) -- instead of being waited for layer by layer:
                    # 25.0 -> 23.8 ms per step at the 768 crop, same bits (profiles/r06/wgrad_stream_ab.md).  ("side", the per-layer
                    # join: 27.2 ms -- the join makes every layer wait for the slower of its two products.)
                    _KEEP_UNTIL_JOIN.setdefault(x.device, []).append((x, dy))
                    _join_side_after_backward(x.device)
                    side = None
            else:
                dw = conv_wgrad(x, dy, ks, stride, dil)
        if need_dx:
            if own[1] and stride == 1:
                # the gradient of x's other consumer is added in the epilogue of either kernel, where it can be
                fuse = g_other is not None and g_other.shape == x.shape and g_other.dtype == torch.float32
                if conv_bx_train_ok(dy.shape, w.shape, 1, dil, True):
                    dx = conv_bx_raw(dy, w, dil, dgrad=True, residual=g_other.contiguous() if fuse else None, packed=bx_packed_weight(w, 1))
                else:
                    dx = conv_sk(dy, w, 1, dil, dgrad=True, packed=packed_weight(w, 1, True), residual=g_other.contiguous() if fuse else None)
                if fuse:
                    g_other = None
            elif own[1] and ks == 1:
                # 1x1, stride 2: the input gradient lives on the even positions only -- the stride-1 product over the small plane,
                # stored with stride 2 into a zero-filled tensor by the kernel itself
                if stride == 2:
                    dx = conv_sk_dgrad_1x1s2(dy, w, x.shape[2], x.shape[3], packed=packed_weight(w, 1, True))
                else:
                    dx = torch.zeros_like(x)
                    dx[:, :, ::stride, ::stride] = conv_sk(dy, w, 1, 1, dgrad=True, packed=packed_weight(w, 1, True))
            elif own[1] and ks == 3 and stride == 2 and dil == 1:
                dx = conv_sk_dgrad_s2(dy, w, x.shape[2], x.shape[3], packed=[packed_weight(w, 2, 2 + sub) for sub in range(4)])
            else:
                dx = torch.ops.aten.convolution_backward(dy, x, w, None, (stride, stride), _aten_pad(ks, dil), (dil, dil), False, (0, 0), 1,
                                                         (True, False, False))[0]
        if need_dw and not own[2]:
            dw = torch.ops.aten.convolution_backward(dy, x, w, None, (stride, stride), _aten_pad(ks, dil), (dil, dil), False, (0, 0), 1,
                                                     (False, True, False))[1]
        if side is not None:
            main.wait_stream(side)                          # dW joins the main stream behind the input gradient (x, dy: alive until here)
        if g_other is not None:
            dx = g_other if dx is None else dx + g_other
        return dx, dw, None, None, None, None, None


def conv_wgrad_supported(conv, x):
    """mas_conv_wgrad takes every dense 1x1 / 3x3 convolution of the network: any channel counts and plane sizes, stride 1 / 2,
    padding = dilation (3x3) / 0 (1x1), dilation 1 / 2 / 4 at stride 1."""
    geom = _conv_geometry(conv, x)
    if geom is None or not _is_1x1_or_3x3(*geom, dilations=(1, 2, 4)):
        return False
    return max(conv.in_channels, conv.out_channels) * x.shape[2] * x.shape[3] < 2 ** 31


def conv_train_plan(conv, x):
    """(forward, input gradient, weight gradient) -> True where this package's kernel runs the product, or None when the layer
    is outside all three (then the caller keeps the nn.Module call).  MAS_TRAIN_CONV = own (default): every product the kernels
    support -- all three of every dense convolution of the network; miopen: none; auto: the weight
    gradient everywhere, forward / input gradient only on planes of >= 192 x 192 / 384 x 384 pixels (MIOpen's Tensile GEMMs are
    still ahead on the 1x1 layers of the small planes: profiles/r03/b_conv_train_table_streamk.md; ~0.4 ms per step)."""
    mode = os.environ.get("MAS_TRAIN_CONV", "own")
    if mode == "miopen" or not conv_wgrad_supported(conv, x):
        return None
    if _reg_step_hook is None and _PARAM_EPOCH[0] == 0:     # (no optimizer hook and nobody invalidates by hand: see the import above)
        return None
    hw = x.shape[2] * x.shape[3]
    fwd_ok = conv.dilation[0] in (1, 2, 4) and hw >= 64
    dgrad_ok = fwd_ok and (conv.stride[0] == 1 or conv.kernel_size[0] == 1 or conv.dilation[0] == 1)
    wgrad_ok = conv.in_channels >= 8
    if mode == "own":
        return (fwd_ok, dgrad_ok, True)
    return (fwd_ok and hw >= 192 * 192, dgrad_ok and hw >= 384 * 384, wgrad_ok)


def conv_train(conv, x, own=(True, True, True), stats=False, fork=False):
    """conv(x) with autograd on the package's kernels (see _ConvTrain).  stats=True: (y, partials) -- the BatchNorm partial sums
    of y from the epilogue of the forward kernel (None when the forward product is not on mas_conv_sk), for bn_act(partials=).
    fork=True: one more result, an alias of x to hand to the other consumer of x (see _ConvTrain)."""
    own = tuple(bool(v) for v in own)
    stats = bool(stats and own[0])
    out = _ConvTrain.apply(x, conv.weight, conv.stride[0], conv.dilation[0], own, stats, bool(fork))
    if not stats and not fork:
        return out
    out = list(out)
    if not stats:
        out.insert(1, None)
    return tuple(out) if fork else (out[0], out[1])
