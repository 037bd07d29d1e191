"""Loss modules of the reference's ``utils/loss.py`` (and the production subclasses defined inside the
reference's trainer files), backed by the HIP kernels of ``csrc/losses.hip``.

Same class names, constructor arguments and ``forward(inputs, targets, superpixels, spmasks)``
signature as the reference, so the trainer plugins read like the reference's:

=============================  =================================================================
class here                     reference definition
=============================  =================================================================
``MyCrossEntropyLoss``         ``utils/loss.py:10-21``
``JointMultiLoss``             ``utils/loss.py:44-63``  ('mean' reduction only, Appendix D)
``GroupMultiLabelCE``          ``utils/loss.py:81-141``  (drops the last target column)
``MultiChoiceCE``              ``utils/loss.py:535-588`` (drops the last target column)
``MultiChoiceCE_``             ``trainer/active_joint_multi_predignore.py:17-73``
``GroupMultiLabelCE_``         ``trainer/active_joint_multi_predignore.py:74-128``
``OnehotCEMultihotChoice``     ``trainer/active_joint_multi_predignore_lossdecomp.py:16-72``
``GroupMultiLabelCE_onlymulti````trainer/active_joint_multi_predignore_mclossablation2.py:17-79``
``RCMultiChoiceCE``            ``utils/loss.py:653-707`` (risk-consistent weighting; drops the last target column)
``OnehotCEMultihotTopone``     ``trainer/active_joint_multi_lossdecomp_topone.py:14-71``
``OnehotCEMultihotRC``         ``trainer/active_joint_multi_lossdecomp_rc.py:14-76`` -- the reference's version raises at
                               ``:54`` (``:53`` already reduced the class axis); the class here computes what
                               ``RCMultiChoiceCE`` defines, restricted to multi-hot pixels
``FusedPartialLabelLoss``      (new) the three production losses from ONE forward scan and ONE
                               backward scan -- what ``train_impl`` of the production trainer uses;
                               ``multi_hot='choice'|'rc'|'topone'`` names the multi-hot pixel term
                               (``csrc/partial_label.h``), ``group=False`` leaves the group term out
``LocalProtoCE``               ``trainer/active_onlineplbl_multi_predignore.py:14-141`` (online local-prototype pseudo
                               labels of the multi-hot superpixels + CE on them; ``csrc/online_plbl.hip``)
``LocalWProtoCE``              ``trainer/active_onlinewplbl_multi_predignore.py:15-148`` (the CE weighted by the
                               network's confidence in the label, or gated by ``--th_wplbl``; mean over non-zero terms)
``JointLocalProtoCE``          ``trainer/active_onlinewplblonly_multi_predignore.py:15-137`` (weighted; the mean of an
                               empty set is NaN, as the reference's)
``LocalsimWProtoCE``           ``trainer/active_onlinesimwplbl_multi_predignore.py:15-148`` (the CE weighted by the pixel's
                               inner product with its nearest prototype, negative ones included, or gated by ``--th_wplbl``)
``JointLocalProtoWeightingCE`` ``trainer/active_pwce_multi_predignore.py:17-155`` (no hard label: CE against the softmax of
                               the prototype similarities over the candidate classes; one-hot superpixels keep plain CE)
``TopOnePlbl``                 ``trainer/active_joint_multi_predignore_top1plbl.py:13-82`` (teacher-gated top-1 candidate term)
``MultiChoiceEnt_``            ``trainer/active_joint_multi_predignore_multient.py:12-70`` (entropy over the candidate set)
``FusedTeacherTermLoss``       (new) merged-positive CE, group term and one of the two above from ONE scan pair
                               (``csrc/teacher_terms.h``) -- what the ``top1plbl`` / ``multient`` trainers use
``WeightedGroupMultiLabelCE``  ``trainer/active_joint_multi_predignore_wgroup.py:12-82`` (group term weighted by the teacher's
                               per-(superpixel, class) maximum; ``forward(inputs, plbl_preds, targets, superpixels, spmasks)``)
``FusedWGroupLoss``            (new) merged-positive CE and the weighted group term from ONE scan pair -- what the ``wgroup``
                               trainer uses
``HierGroupMultiLabelCE``      ``utils/loss.py:143-235`` (the group term spread over the fine superpixel around every arg-pixel;
                               ``forward(inputs, targets, spmasks, superpixels, superpixel_smalls)``; ``csrc/hier_group.h``)
``AugHierGroupMultiLabelCE``   ``utils/loss.py:439-533`` (``--nocropsp``: rows of the superpixels on the crop's border cleared)
``AsyncHierGroupMultiLabelCE`` ``utils/loss.py:341-437`` (the pair table from a weak view of the picture, the sum over the strong view)
``WeightAsyncHierGroupMultiLabelCE``  ``utils/loss.py:237-339`` (the same, every pair weighted by the teacher's max / mean probability)
=============================  =================================================================

Inputs must be ROCm tensors; there is no CPU path (``_lib.MulActSegHipError`` otherwise).
"""
import torch
import torch.nn as nn

from .. import _lib, ops


def _check_superpixels(targets, num_superpixel):
    if targets.shape[1] != num_superpixel:
        raise ValueError("targets carry %d superpixels, loss was built for %d" % (targets.shape[1], num_superpixel))


def _u8(targets):
    """The multi-hot targets as the kernels read them: contiguous u8."""
    return (targets if targets.dtype == torch.uint8 else targets.to(torch.uint8)).contiguous()


def _hw(size):
    """``size`` of the ``forward_lowres`` forms as a plain (H, W); None (full-resolution logits) stays None."""
    return None if size is None else (int(size[0]), int(size[1]))


def _shared_temperature(group_temperature, multi_temperature):
    if group_temperature != multi_temperature:
        raise ValueError("the fused scan shares one softmax: group_ce_temp must equal multi_ce_temp "
                         "(both 0.1 in the reference scripts)")
    return multi_temperature


def _mean_only(reduction, why="only reduction='mean' is on the hot path"):
    if reduction != 'mean':
        raise NotImplementedError(why)


def _fused_forward(ctx, z, size, tgt, cols_used, superpixels, spmasks, invT, flags, sync, weights):
    """Shared forward of the three autograd functions below: ONE library call (prep + scan + finalize with the loss values,
    ops.partial_loss_fwd_fused); ``tgt`` is the u8 multi-hot target tensor (``cols_used`` columns count) or, with ``cols_used``
    None, ready int32 bit masks."""
    z = z.contiguous()
    spx = superpixels.contiguous()
    msk = spmasks.contiguous()
    as_bits = cols_used is None
    losses, st = ops.partial_loss_fwd_fused(z, size, spx, msk, invT, flags, targets=None if as_bits else tgt, cols_used=cols_used,
                                            bits=tgt if as_bits else None, weights=weights, reduce_acc=_all_reduce_sum if sync else None)
    ctx.save_for_backward(z, spx, msk, st.work, tgt if as_bits else st.work, weights if weights is not None else st.work)
    ctx.as_bits, ctx.has_w = as_bits, weights is not None
    ctx.geom = (st.N, st.S, st.C)
    ctx.invT, ctx.flags, ctx.size = invT, flags, size
    ctx.mark_non_differentiable(st.acc)
    return losses, st.acc


def _fused_backward(ctx, grad):
    z, spx, msk, work, bits, weights = ctx.saved_tensors
    st = ops.LossState()
    st.work, st.bits, st.flags = work, bits if ctx.as_bits else None, ctx.flags
    st.N, st.S, st.C = ctx.geom
    return ops.partial_loss_bwd_fused(z, ctx.size, spx, msk, st, grad, ctx.invT, weights=weights if ctx.has_w else None)


class _PartialLossFn(torch.autograd.Function):
    """(ce, mc, group) = f(inputs): the forward direction (accumulators, arg-pixel table, loss values) and the backward direction
    (one scan writing dz) are one library call each.  No host synchronisation in either direction.

    ``size`` None: ``inputs`` are the full-resolution logits.  ``size`` = (H, W): they are the quarter-resolution logits, and their x4
    bilinear upsampling is evaluated inside both scans -- the full-resolution logits and their gradient never exist (``csrc/losses.hip``
    LOWRES kernels).  Forward values are bit-identical to those on ``F.interpolate(inputs, size, 'bilinear')``; the gradient is an
    order-independent fixed-point sum (run-to-run identical)."""

    @staticmethod
    def forward(ctx, inputs, size, tgt, cols_used, superpixels, spmasks, invT, flags, sync):
        size = _hw(size)
        losses, acc = _fused_forward(ctx, inputs, size, tgt, cols_used, superpixels, spmasks, invT, flags, sync, None)
        return losses[0], losses[1], losses[2], acc

    @staticmethod
    def backward(ctx, g_ce, g_mc, g_group, _g_acc):
        grad_out = torch.stack([g_ce, g_mc, g_group]).to(torch.float32).contiguous()
        return _fused_backward(ctx, grad_out), None, None, None, None, None, None, None, None


class _WeightedLowResLossFn(torch.autograd.Function):
    """total, ce, mc, group = f(zq): the trainer's objective ``w_ce*ce + w_mc*mc + w_group*group`` as ONE differentiable
    output (its value is formed by the last workgroup of the group finalize, its chain rule inside the backward scan), the three
    parts as detached values for logging.  Three launches forward (prep, scan, finalize), three backward (memset, scan, fixed point ->
    float), one library call each."""

    @staticmethod
    def forward(ctx, zq, size, tgt, cols_used, superpixels, spmasks, invT, flags, sync, weights):
        losses, acc = _fused_forward(ctx, zq, (int(size[0]), int(size[1])), tgt, cols_used, superpixels, spmasks, invT, flags, sync, weights)
        parts = losses.detach()
        ctx.mark_non_differentiable(parts)
        return losses[3], parts, acc

    @staticmethod
    def backward(ctx, g_total, _g_parts, _g_acc):
        g = g_total.reshape(1).to(torch.float32).contiguous()
        return _fused_backward(ctx, g), None, None, None, None, None, None, None, None, None


def _all_reduce_sum(acc):
    """Sum the fixed-point loss sums and pixel counts over the data-parallel ranks (RCCL all-reduce of 8
    int64 words): integer addition, so the result does not depend on the number of GPUs."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)


def _run(inputs, targets, superpixels, spmasks, temp, flags, drop_last_column, sync=True, size=None):
    """CONTRACT of the drop-in modules under torch.distributed: with ``sync`` (the default of every partial-label module below,
    attribute ``sync_normalisers`` where it is configurable) the returned loss is the objective over the GLOBAL batch, identical
    on every rank; a caller that lets DistributedDataParallel average the gradients must multiply it by the world size before
    ``backward()`` (``ActiveTrainer.update`` does, guarded by ``loss_is_global``).  With ``sync=False`` the loss is the local
    objective and must NOT be scaled.

    ``sync``: under torch.distributed (world > 1) the integer sums and counts are all-reduced before the division, so
    every rank holds the SAME loss value -- the loss over the global batch.  The reference's skip-on-zero / raise-on-NaN
    decisions (``active_joint_multi.py:31-37``) are then global by construction: no rank can skip ``backward()`` while
    its peers wait in the gradient all-reduce.

    ``size`` = (H, W): ``inputs`` are the quarter-resolution logits (``_PartialLossFn``)."""
    cols = targets.shape[-1]
    return _PartialLossFn.apply(inputs, size, _u8(targets), cols - 1 if drop_last_column else cols, superpixels, spmasks,
                                ops.inv_temperature(temp), flags, sync)


class MyCrossEntropyLoss(nn.CrossEntropyLoss):
    """Cross entropy with a temperature (stage-2 training) -- reference ``utils/loss.py:10-21``.

    On the GPU (mean reduction, no class weights, no label smoothing, <= 32 channels) the value and the gradient come from the
    partial-label scans in their MAS_LOSS_TCE form: one forward scan and one backward scan over the valid pixels instead of
    ATen's div + log_softmax + nll passes over the materialised ``[N,C,H,W]`` tensor; ``forward_lowres`` takes the model's
    quarter-resolution logits (``net(images, lowres=True)``) and evaluates the x4 bilinear upsampling
    (``models/segmentation/utils.py:25``) inside the scans -- the full-resolution logits and their gradient never exist.
    Under torch.distributed the sums and the valid-pixel counts are all-reduced before the division when ``sync_normalisers``
    (the mean over the GLOBAL batch; multiply by the world size before ``backward()`` under DistributedDataParallel)."""

    def __init__(self, ignore_index, reduction='mean', temperature=1.0, sync_normalisers=False):
        super().__init__(ignore_index=ignore_index, reduction=reduction)
        self.temperature = temperature
        self.sync_normalisers = sync_normalisers

    def _fused(self, input, target):
        return (input.is_cuda and self.reduction == 'mean' and self.weight is None and getattr(self, 'label_smoothing', 0.0) == 0.0
                and input.dim() == 4 and input.shape[1] <= _lib.MAX_CLASSES and input.dtype == torch.float32
                and target.dim() == 3 and not target.is_floating_point())

    def _labels_mask(self, input, target):
        C = input.shape[1]
        labels = target.contiguous()
        # (labels outside [0, C) other than ignore_index are an error in torch; here they are left out like ignored ones)
        mask = (labels != self.ignore_index) & (labels >= 0) & (labels < C)
        dummy_bits = torch.zeros((input.shape[0], C), dtype=torch.int32, device=input.device)
        return labels, mask, dummy_bits

    def forward(self, input, target):
        if not self._fused(input, target):
            return super().forward(input / self.temperature, target)
        labels, mask, bits = self._labels_mask(input, target)
        ce, _, _, self.last_acc = _PartialLossFn.apply(input, None, bits, None, labels, mask, ops.inv_temperature(self.temperature),
                                                        _lib.LOSS_CE | _lib.LOSS_TCE, self.sync_normalisers)
        return ce

    def forward_lowres(self, quarter_logits, size, target):
        """CE of ``F.interpolate(quarter_logits, size, 'bilinear', align_corners=False) / T`` against ``target`` [N,H,W]."""
        if not self._fused(quarter_logits, target):
            up = torch.nn.functional.interpolate(quarter_logits, size=tuple(size), mode='bilinear', align_corners=False)
            return super().forward(up / self.temperature, target)
        labels, mask, bits = self._labels_mask(quarter_logits, target)
        ce, _, _, self.last_acc = _PartialLossFn.apply(quarter_logits, tuple(size), bits, None, labels, mask,
                                                        ops.inv_temperature(self.temperature), _lib.LOSS_CE | _lib.LOSS_TCE,
                                                        self.sync_normalisers)
        return ce


class MultiChoiceCE(nn.Module):
    """Merged-positive CE -- reference ``utils/loss.py:535-588`` (last target column dropped)."""
    _drop_last = True
    _flags = _lib.LOSS_CE

    def __init__(self, num_class, temperature=1.0, reduction='mean'):
        super().__init__()
        _mean_only(reduction)
        self.num_class = num_class
        self.reduction = reduction
        self.eps = 1e-8
        self.temp = temperature

    def forward(self, inputs, targets, superpixels, spmasks):
        ce, _, _, _ = _run(inputs, targets, superpixels, spmasks, self.temp, self._flags, self._drop_last)
        return ce


class MultiChoiceCE_(MultiChoiceCE):
    """All target columns (incl. "undefined") -- ``trainer/active_joint_multi_predignore.py:17-73``."""
    _drop_last = False


class OnehotCEMultihotChoice(MultiChoiceCE):
    """Returns (ce over one-hot superpixels, mc over multi-hot superpixels) --
    ``trainer/active_joint_multi_predignore_lossdecomp.py:16-72``."""
    _drop_last = False
    _flags = _lib.LOSS_CE | _lib.LOSS_DECOMP

    def forward(self, inputs, targets, superpixels, spmasks):
        ce, mc, _, _ = _run(inputs, targets, superpixels, spmasks, self.temp, self._flags, self._drop_last)
        return ce, mc


class RCMultiChoiceCE(MultiChoiceCE):
    """Risk-consistent weighting, one merged sum: every candidate's own CE weighted by the detached in-set confidence
    ``p_c / sum_Y p`` -- reference ``utils/loss.py:653-707`` (last target column dropped)."""
    _flags = _lib.LOSS_CE | _lib.LOSS_RC


class OnehotCEMultihotRC(OnehotCEMultihotChoice):
    """(ce over one-hot superpixels, risk-consistent mc over multi-hot superpixels) -- the loss
    ``trainer/active_joint_multi_lossdecomp_rc.py:14-76`` means: as written it raises at ``:54`` (a second reduction over the class
    axis ``:53`` already removed); this is ``RCMultiChoiceCE``'s term restricted to multi-hot pixels, all target columns used."""
    _flags = _lib.LOSS_CE | _lib.LOSS_DECOMP | _lib.LOSS_RC


class OnehotCEMultihotTopone(OnehotCEMultihotChoice):
    """(ce over one-hot superpixels, ``-log max_Y p`` over multi-hot superpixels) --
    ``trainer/active_joint_multi_lossdecomp_topone.py:14-71``.  On a tie the gradient goes to the lowest class index."""
    _flags = _lib.LOSS_CE | _lib.LOSS_DECOMP | _lib.LOSS_TOPONE


MULTI_HOT_FLAGS = {'choice': 0, 'rc': _lib.LOSS_RC, 'topone': _lib.LOSS_TOPONE}


class GroupMultiLabelCE(nn.Module):
    """Group / MIL loss: -log of the per-superpixel class-wise max probability --
    reference ``utils/loss.py:81-141`` (last target column dropped)."""
    _drop_last = True
    _flags = _lib.LOSS_GROUP

    def __init__(self, args, num_class, num_superpixel, temperature=1.0, reduction='mean'):
        super().__init__()
        _mean_only(reduction)
        self.args = args
        self.num_class = num_class
        self.num_superpixel = num_superpixel
        self.eps = 1e-8
        self.temp = temperature
        self.reduction = reduction

    def forward(self, inputs, targets, superpixels, spmasks):
        _check_superpixels(targets, self.num_superpixel)
        _, _, group, _ = _run(inputs, targets, superpixels, spmasks, self.temp, self._flags, self._drop_last)
        return group


class GroupMultiLabelCE_(GroupMultiLabelCE):
    """``trainer/active_joint_multi_predignore.py:74-128``."""
    _drop_last = False


class GroupMultiLabelCE_onlymulti(GroupMultiLabelCE_):
    """Only superpixels with more than one target bit --
    ``trainer/active_joint_multi_predignore_mclossablation2.py:17-79``."""
    _flags = _lib.LOSS_GROUP | _lib.LOSS_GROUP_ONLY_MULTI


class JointMultiLoss(nn.Module):
    """``utils/loss.py:44-63`` ('mean' path): returns (loss_group, loss_pos)."""

    def __init__(self, group_multi_loss, multi_pos_loss, reduction='mean'):
        super().__init__()
        _mean_only(reduction, "the reference's 'none' branch is broken (wrong arity, utils/loss.py:57-61)")
        self.group_multi_loss = group_multi_loss
        self.multi_pos_loss = multi_pos_loss
        self.reduction = reduction

    def forward(self, inputs, targets, superpixels, spmasks):
        return (self.group_multi_loss(inputs, targets, superpixels, spmasks),
                self.multi_pos_loss(inputs, targets, superpixels, spmasks))


class FusedPartialLabelLoss(nn.Module):
    """The production stage-1 objective from one forward scan and one backward scan:
    returns (group_loss, ce_loss, mc_loss) exactly as
    ``GroupMultiLabelCE_onlymulti`` + ``OnehotCEMultihotChoice`` would
    (``trainer/active_joint_multi_predignore_lossdecomp.py:102-103``), reading the logits once.

    ``multi_hot``: the term of a multi-hot pixel -- 'choice' (the reference's merged positive), 'rc' (risk-consistent weighting) or
    'topone' (top-1 candidate); the same scans with another per-pixel formula.  ``group=False``: no group term -- no
    ``[N,S,C]`` table is allocated and the group value is 0 (the objective of ``trainer/active_joint_multi_lossdecomp_rc.py``)."""

    def __init__(self, num_superpixel, group_temperature=1.0, multi_temperature=1.0, only_multi=True, decomp=True,
                 sync_normalisers=True, multi_hot='choice', group=True):
        super().__init__()
        if multi_hot not in MULTI_HOT_FLAGS:
            raise ValueError("multi_hot must be one of %s, got %r" % (', '.join(MULTI_HOT_FLAGS), multi_hot))
        self.multi_hot = multi_hot
        # under torch.distributed: all-reduce (sum, n) before the division so that the objective equals the
        # single-GPU objective over the global batch; multiply the loss by world_size before backward()
        # when gradients are then AVERAGED over ranks (DistributedDataParallel does).
        self.sync_normalisers = sync_normalisers
        self.num_superpixel = num_superpixel
        self.temp = _shared_temperature(group_temperature, multi_temperature)
        self.flags = _lib.LOSS_CE | ((_lib.LOSS_GROUP | (_lib.LOSS_GROUP_ONLY_MULTI if only_multi else 0)) if group else 0) \
            | (_lib.LOSS_DECOMP if decomp else 0) | MULTI_HOT_FLAGS[multi_hot]

    def forward(self, inputs, targets, superpixels, spmasks):
        ce, mc, group, self.last_acc = _run(inputs, targets, superpixels, spmasks, self.temp, self.flags, False,
                                            sync=self.sync_normalisers)
        return group, ce, mc

    def forward_lowres(self, quarter_logits, size, targets, superpixels, spmasks):
        """The same three losses from the model's quarter-resolution logits (``net(images, lowres=True)``): the final x4
        bilinear upsampling (``models/segmentation/utils.py:25``) happens per selected pixel inside the scans."""
        ce, mc, group, self.last_acc = _run(quarter_logits, targets, superpixels, spmasks, self.temp, self.flags, False,
                                            sync=self.sync_normalisers, size=tuple(size))
        return group, ce, mc

    def weighted_lowres(self, quarter_logits, size, targets, superpixels, spmasks, coeff, coeff_mc, coeff_gm):
        """``(coeff * ce + coeff_mc * mc) + coeff_gm * group`` (``..._lossdecomp.py:104``) as one differentiable scalar, plus the
        detached parts ``(group, ce, mc)`` for logging -- same value, bit for bit, as composing ``forward_lowres`` with torch
        arithmetic, in half the kernel launches."""
        key = (float(coeff), float(coeff_mc), float(coeff_gm), quarter_logits.device)
        if getattr(self, '_w_key', None) != key:
            self._w_key, self._w = key, torch.tensor(key[:3], dtype=torch.float32, device=quarter_logits.device)
        total, parts, self.last_acc = _WeightedLowResLossFn.apply(quarter_logits, tuple(size), _u8(targets), targets.shape[-1], superpixels, spmasks,
                                                                  ops.inv_temperature(self.temp), self.flags, self.sync_normalisers, self._w)
        return total, parts[2], parts[0], parts[1]


class LocalProtoCE(nn.Module):
    """Online local-prototype pseudo labels and the cross entropy on them -- reference
    ``trainer/active_onlineplbl_multi_predignore.py:14-141``.  For every candidate class of a selected multi-hot superpixel the pixel
    with the largest predicted probability is the class's local prototype; every pixel of the superpixel takes the class of the
    prototype whose feature is nearest to its own (``generate_plbl``); the loss is the mean CE of the training-mode logits on those
    labels, 0 when there is none.

    ``forward`` takes the reference's full-resolution tensors.  ``forward_lowres`` takes what the model computes -- quarter-resolution
    logits and features of the eval-mode forward, quarter-resolution training logits -- and evaluates the x4 bilinear upsampling
    inside the kernels: neither ``feat_forward``'s ``[N,256,H,W]`` features nor any ``[N,C,H,W]`` logits exist.  No host
    synchronisation; run-to-run identical bytes; under torch.distributed the sum and the count are all-reduced before the division
    (the loss over the global batch, see ``_run``)."""
    _mode = _lib.LCE_UNWEIGHTED
    _empty_nan = False
    _honours_weight_wo_proto = False
    _weight_sim = False             # the weight map holds prototype similarities, which may be negative (LocalsimWProtoCE)

    def __init__(self, args, num_superpixel, temperature=1.0, reduction='mean'):
        super().__init__()
        _mean_only(reduction, "only reduction='mean' exists (the reference asserts it)")
        self.args = args
        self.num_superpixel = num_superpixel
        self.temp = temperature
        self.reduction = reduction
        self.eps = 1e-8
        self.sync_normalisers = True

    def generate_plbl(self, inputs_plbl, feats_plbl, targets, superpixels, spmasks, size=None):
        """(weight f32 [N,H,W], nn_plbl u8 [N,H,W]) as the reference's ``generate_plbl`` returns them (255 = no label, weight 0).
        ``size`` None: the tensors are at the resolution of ``superpixels``; else they are quarter-resolution maps upsampled
        in-kernel to ``size``."""
        _check_superpixels(targets, self.num_superpixel)
        if size is None:
            size = superpixels.shape[-2:]
        wo_proto = self._honours_weight_wo_proto and bool(getattr(self.args, 'weight_wo_proto', False))
        with torch.no_grad():
            labels, weight = ops.online_pseudo_labels(inputs_plbl.detach().contiguous(), feats_plbl.detach().contiguous(), size,
                                                      superpixels.contiguous(), spmasks.contiguous(), targets=targets,
                                                      invT=ops.inv_temperature(self.temp), weight_wo_proto=wo_proto,
                                                      weight_sim=self._weight_sim)
        return weight, labels

    def _mode_th(self):
        return self._mode, 0.0

    def _loss(self, inputs, size, labels, weight):
        mode, th = self._mode_th()
        loss, self.last_acc = ops.label_ce_lowres(inputs, size, labels, None if mode == _lib.LCE_UNWEIGHTED else weight,
                                                  ops.inv_temperature(self.temp), mode=mode, th=th, empty_nan=self._empty_nan,
                                                  reduce_acc=_all_reduce_sum if self.sync_normalisers else None,
                                                  signed=self._weight_sim and mode == _lib.LCE_WEIGHTED)
        return loss

    def forward(self, inputs_plbl, feats_plbl, inputs, targets, superpixels, spmasks):
        weight, labels = self.generate_plbl(inputs_plbl, feats_plbl, targets, superpixels, spmasks)
        return self._loss(inputs, inputs.shape[-2:], labels, weight)

    def forward_lowres(self, zq_p, featq, zq, size, targets, superpixels, spmasks):
        """``zq_p`` [N,C,h,w] / ``featq`` [N,Ch,h,w]: logits and normalised point features of the eval-mode forward
        (``net.feat_forward_quarter``); ``zq`` [N,C,h,w]: the training-mode logits (``net(images, lowres=True)``); ``size`` = (H, W)."""
        size = _hw(size)
        weight, labels = self.generate_plbl(zq_p, featq, targets, superpixels, spmasks, size=size)
        return self._loss(zq, size, labels, weight)


class LocalWProtoCE(LocalProtoCE):
    """``LocalProtoCE`` with every pixel's CE weighted by the network's own probability of its pseudo label (``args.weight_wo_proto``:
    prototype pixels weigh 1), or, with ``args.th_wplbl``, kept only where that probability exceeds the threshold; the mean runs over
    the non-zero terms -- reference ``trainer/active_onlinewplbl_multi_predignore.py:15-148``."""
    _mode = _lib.LCE_WEIGHTED
    _honours_weight_wo_proto = True

    def _mode_th(self):
        th = getattr(self.args, 'th_wplbl', None)
        return (_lib.LCE_WEIGHTED, 0.0) if th is None else (_lib.LCE_THRESHOLD, float(th))


class JointLocalProtoCE(LocalProtoCE):
    """The weighted CE alone, as the only loss of its trainer -- reference ``trainer/active_onlinewplblonly_multi_predignore.py:15-137``:
    neither ``--th_wplbl`` nor ``--weight_wo_proto`` is read, and a batch without a non-zero term gives NaN (the mean of an empty
    tensor), which the trainer's ``update`` raises on."""
    _mode = _lib.LCE_WEIGHTED
    _empty_nan = True


class LocalsimWProtoCE(LocalWProtoCE):
    """``LocalProtoCE`` with every pixel's CE weighted by its inner product with the nearest prototype -- the similarity that chose the
    label, not the network's confidence -- or, with ``args.th_wplbl``, kept only where that similarity exceeds the threshold; the mean
    runs over the non-zero terms, 0 when there is none -- reference ``trainer/active_onlinesimwplbl_multi_predignore.py:15-148``.  A
    similarity can be negative, and the reference's ``weight * CE`` is then negative too: the sum is signed.  ``args.weight_wo_proto``
    is not read (the reference's ``generate_plbl`` never does)."""
    _honours_weight_wo_proto = False
    _weight_sim = True


class JointLocalProtoWeightingCE(nn.Module):
    """Prototype-similarity soft targets instead of hard pseudo labels -- reference ``trainer/active_pwce_multi_predignore.py:17-155``.
    Every selected pixel of a multi-hot superpixel gets a target over its candidate classes: the softmax, at temperature
    ``args.simw_temp`` (read at call time, or the ``simw_temp`` argument), of its inner products with the classes' local prototypes.
    The loss is the mean over the selected pixels of ``sum_c w_c * -log(p_c + 1e-8)``; pixels of one-hot superpixels keep plain CE.

    Replicated from the reference as it runs: both softmaxes -- the prototype pick and the training logits -- use ``args.ce_temp``; the
    ``temperature`` the class is constructed with (the trainer passes ``group_ce_temp``) is stored and ignored.  A picture without a
    selected multi-hot pixel is skipped whole, its selected one-hot pixels entering neither the sum nor the count.  An empty batch
    gives 0.  One difference: a selected pixel whose superpixel id lies outside ``[0, nseg)`` makes the reference raise; here it is
    not counted.

    ``forward`` / ``forward_lowres`` as ``LocalProtoCE``'s."""

    def __init__(self, args, num_superpixel, temperature=1.0, reduction='mean'):
        super().__init__()
        _mean_only(reduction, "only reduction='mean' exists (the reference asserts it)")
        self.args = args
        self.num_superpixel = num_superpixel
        self.ce_temp = args.ce_temp
        self.temp = temperature
        self.reduction = reduction
        self.eps = 1e-8
        self.sync_normalisers = True

    def soft_weights(self, inputs_plbl, feats_plbl, targets, superpixels, spmasks, size=None, simw_temp=None):
        """(softw f32 [N,C,H,W], defined on the candidate planes of the valid pixels; live int32 [N]; bits int32 [N,S])"""
        _check_superpixels(targets, self.num_superpixel)
        if size is None:
            size = superpixels.shape[-2:]
        tau = self.args.simw_temp if simw_temp is None else simw_temp
        with torch.no_grad():
            return ops.online_soft_weights(inputs_plbl.detach().contiguous(), feats_plbl.detach().contiguous(), size,
                                           superpixels.contiguous(), spmasks.contiguous(), targets=targets,
                                           invT=ops.inv_temperature(self.ce_temp), inv_tau=ops.inv_temperature(tau))

    def _loss(self, inputs, size, superpixels, spmasks, softw, live, bits):
        loss, self.last_acc = ops.soft_ce_lowres(inputs, size, superpixels, spmasks, bits, softw, live, ops.inv_temperature(self.ce_temp),
                                                 reduce_acc=_all_reduce_sum if self.sync_normalisers else None)
        return loss

    def forward(self, inputs_plbl, feats_plbl, inputs, targets, superpixels, spmasks, simw_temp=None):
        softw, live, bits = self.soft_weights(inputs_plbl, feats_plbl, targets, superpixels, spmasks, simw_temp=simw_temp)
        return self._loss(inputs, inputs.shape[-2:], superpixels, spmasks, softw, live, bits)

    def forward_lowres(self, zq_p, featq, zq, size, targets, superpixels, spmasks, simw_temp=None):
        size = _hw(size)
        softw, live, bits = self.soft_weights(zq_p, featq, targets, superpixels, spmasks, size=size, simw_temp=simw_temp)
        return self._loss(zq, size, superpixels, spmasks, softw, live, bits)


class _TeacherLossFn(torch.autograd.Function):
    """(ce, mc, group, x) = f(z): the scans of ``csrc/losses.hip`` with the fourth loss slot of ``csrc/teacher_terms.h`` -- one forward
    scan and one backward scan whatever the flags hold.  ``zt`` (the teacher's logits, ``None`` for the entropy) is a constant;
    ``size`` None: full-resolution tensors, else quarter-resolution ones upsampled inside the scans.  No host synchronisation."""

    @staticmethod
    def forward(ctx, z, zt, size, targets, superpixels, spmasks, invT, invT_x, plbl_th, flags, sync):
        z, spx, msk = z.contiguous(), superpixels.contiguous(), spmasks.contiguous()
        zt = None if zt is None else zt.detach().contiguous()
        bits = ops.target_bits(targets)
        losses, acc, gmax = ops.teacher_loss_fwd(z, zt, size, spx, msk, bits, invT, invT_x, plbl_th, flags,
                                                 reduce_acc=_all_reduce_sum if sync else None)
        ctx.save_for_backward(z, spx, msk, bits, acc, zt if zt is not None else acc, gmax if gmax is not None else acc)
        ctx.has = (zt is not None, gmax is not None)
        ctx.consts = (size, invT, invT_x, plbl_th, flags)
        ctx.mark_non_differentiable(acc)
        return losses[0], losses[1], losses[2], losses[3], acc

    @staticmethod
    def backward(ctx, g_ce, g_mc, g_group, g_x, _g_acc):
        z, spx, msk, bits, acc, zt, gmax = ctx.saved_tensors
        size, invT, invT_x, plbl_th, flags = ctx.consts
        grad_out = torch.stack([g_ce, g_mc, g_group, g_x]).to(torch.float32).contiguous()
        dz = ops.teacher_loss_bwd(z, zt if ctx.has[0] else None, size, spx, msk, bits, gmax if ctx.has[1] else None, acc, grad_out, invT,
                                  invT_x, plbl_th, flags)
        return (dz,) + (None,) * 10


def _teacher_run(z, zt, size, targets, superpixels, spmasks, temp, temp_x, plbl_th, flags, sync):
    return _TeacherLossFn.apply(z, zt, _hw(size), _u8(targets), superpixels, spmasks, ops.inv_temperature(temp),
                                ops.inv_temperature(temp_x), float(plbl_th), flags, sync)


class MultiChoiceEnt_(nn.Module):
    """Entropy of the softmax restricted to the candidate set, over the selected pixels of multi-hot superpixels, ``sum / (1 + n)`` --
    reference ``trainer/active_joint_multi_predignore_multient.py:12-70`` (the override that runs; the base class ``MultiChoiceEnt`` of
    ``utils/loss.py`` does not).  All target columns are used.  As in the reference a candidate whose logit is exactly ``0.0`` drops
    out of its own softmax (``csrc/teacher_terms.h``)."""
    _flags = _lib.LOSS_ENT

    def __init__(self, num_class, temperature=1.0, reduction='mean'):
        super().__init__()
        _mean_only(reduction)
        self.num_class = num_class
        self.reduction = reduction
        self.eps = 1e-8
        self.temp = temperature
        self.sync_normalisers = True

    def forward(self, inputs, targets, superpixels, spmasks):
        *_, x, self.last_acc = _teacher_run(inputs, None, None, targets, superpixels, spmasks, self.temp, self.temp, 0.0, self._flags,
                                            self.sync_normalisers)
        return x

    def forward_lowres(self, zq, size, targets, superpixels, spmasks):
        """The same value from the model's quarter-resolution logits, upsampled x4 bilinearly per selected pixel inside the scans."""
        *_, x, self.last_acc = _teacher_run(zq, None, size, targets, superpixels, spmasks, self.temp, self.temp, 0.0, self._flags,
                                            self.sync_normalisers)
        return x


class TopOnePlbl(MultiChoiceEnt_):
    """Self-training on the candidate set: ``-log max_{c in Y} p_c`` on the selected multi-hot pixels whose TEACHER (``plbl_inputs``,
    an eval-mode forward of the same weights, a constant of the gradient) is confident, ``filtering_threshold < max_{c in Y} t_c``
    (``within_filtering``: the maximum divided by the teacher's mass on the candidates); ``sum / (1 + n_counted)`` -- reference
    ``trainer/active_joint_multi_predignore_top1plbl.py:13-82``.  On a tie the gradient goes to the lowest class index."""
    _flags = _lib.LOSS_TOP1

    def __init__(self, num_class, within_filtering=False, filtering_threshold=0, temperature=1.0, reduction='mean'):
        super().__init__(num_class, temperature, reduction)
        self.plbl_th = filtering_threshold
        self.within_filtering = within_filtering

    def _f(self):
        return self._flags | (_lib.LOSS_WITHIN if self.within_filtering else 0)

    def forward(self, inputs, plbl_inputs, targets, superpixels, spmasks):
        *_, x, self.last_acc = _teacher_run(inputs, plbl_inputs, None, targets, superpixels, spmasks, self.temp, self.temp, self.plbl_th,
                                            self._f(), self.sync_normalisers)
        return x

    def forward_lowres(self, zq, zq_teacher, size, targets, superpixels, spmasks):
        """``zq`` / ``zq_teacher`` [N,C,h,w]: the training-mode and the eval-mode quarter-resolution logits; both are interpolated in
        registers with the same taps -- no ``[N,C,H,W]`` tensor of either exists."""
        *_, x, self.last_acc = _teacher_run(zq, zq_teacher, size, targets, superpixels, spmasks, self.temp, self.temp, self.plbl_th,
                                            self._f(), self.sync_normalisers)
        return x


class FusedTeacherTermLoss(nn.Module):
    """(pos, group, x) of the ``top1plbl`` / ``multient`` trainers from ONE forward scan and ONE backward scan: the merged-positive CE
    (``MultiChoiceCE_``) and the group term (``GroupMultiLabelCE_``) at their shared temperature, and ``x`` = ``TopOnePlbl``
    (``term='top1'``) or ``MultiChoiceEnt_`` (``term='ent'``) at ``term_temperature`` -- each value equal, bit for bit, to the
    stand-alone module's.  Built like ``FusedPartialLabelLoss``."""

    def __init__(self, num_superpixel, term, group_temperature=1.0, multi_temperature=1.0, term_temperature=1.0, within_filtering=False,
                 filtering_threshold=0.0, sync_normalisers=True):
        super().__init__()
        if term not in ('top1', 'ent'):
            raise ValueError("term must be 'top1' or 'ent', got %r" % (term,))
        self.num_superpixel = num_superpixel
        self.term = term
        self.temp = _shared_temperature(group_temperature, multi_temperature)
        self.term_temp = term_temperature
        self.plbl_th = filtering_threshold
        self.sync_normalisers = sync_normalisers
        self.flags = _lib.LOSS_CE | _lib.LOSS_GROUP | (_lib.LOSS_ENT if term == 'ent' else
                                                       _lib.LOSS_TOP1 | (_lib.LOSS_WITHIN if within_filtering else 0))

    def _run(self, z, zt, size, targets, superpixels, spmasks):
        _check_superpixels(targets, self.num_superpixel)
        if (zt is None) != (self.term == 'ent'):
            raise ValueError("the top1 term needs the teacher's logits, the entropy takes none")
        pos, _, group, x, self.last_acc = _teacher_run(z, zt, size, targets, superpixels, spmasks, self.temp, self.term_temp, self.plbl_th,
                                                       self.flags, self.sync_normalisers)
        return pos, group, x

    def forward(self, inputs, plbl_inputs, targets, superpixels, spmasks):
        """``plbl_inputs``: the teacher's logits (``None`` for ``term='ent'``)."""
        return self._run(inputs, plbl_inputs, None, targets, superpixels, spmasks)

    def forward_lowres(self, zq, zq_teacher, size, targets, superpixels, spmasks):
        return self._run(zq, zq_teacher, size, targets, superpixels, spmasks)


class _WGroupLossFn(torch.autograd.Function):
    """(ce, mc, group) = f(z) with the group term weighted by the teacher's table (``csrc/teacher_terms.h``, wgroup): one forward scan
    with the weighted finalize and one backward scan.  ``zt`` is a constant; ``size`` None: full-resolution tensors, else
    quarter-resolution ones upsampled inside the scans.  No host synchronisation."""

    @staticmethod
    def forward(ctx, z, zt, size, targets, superpixels, spmasks, invT, flags, sync):
        z, spx, msk = z.contiguous(), superpixels.contiguous(), spmasks.contiguous()
        zt = zt.detach().contiguous()
        bits = ops.target_bits(targets)
        losses, acc, gmax, tmax = ops.wgroup_loss_fwd(z, zt, size, spx, msk, bits, invT, flags, reduce_acc=_all_reduce_sum if sync else None)
        ctx.save_for_backward(z, zt, spx, msk, bits, acc, gmax, tmax)
        ctx.consts = (size, invT, flags)
        ctx.mark_non_differentiable(acc)
        return losses[0], losses[1], losses[2], acc

    @staticmethod
    def backward(ctx, g_ce, g_mc, g_group, _g_acc):
        z, zt, spx, msk, bits, acc, gmax, tmax = ctx.saved_tensors
        size, invT, flags = ctx.consts
        grad_out = torch.stack([g_ce, g_mc, g_group]).to(torch.float32).contiguous()
        return (ops.wgroup_loss_bwd(z, zt, size, spx, msk, bits, gmax, tmax, acc, grad_out, invT, flags),) + (None,) * 8


def _wgroup_run(z, zt, size, targets, superpixels, spmasks, temp, flags, sync):
    if zt is None:
        raise ValueError("the weighted group term needs the teacher's logits")
    return _WGroupLossFn.apply(z, zt, _hw(size), _u8(targets), superpixels, spmasks, ops.inv_temperature(temp), flags, sync)


class WeightedGroupMultiLabelCE(GroupMultiLabelCE_):
    """The group / MIL loss with every (superpixel, class) term weighted by the TEACHER's maximum probability of that class over the
    selected pixels of that superpixel (``plbl_preds``, an eval-mode forward of the same weights at the same temperature, a constant
    of the gradient): ``sum_{(s,c): P > 0} Wt[s,c] * -log(P[s,c] + eps) / (1 + n)`` -- reference
    ``trainer/active_joint_multi_predignore_wgroup.py:12-82``.  ``args.group_only_single``: only superpixels with more than one
    target bit (``args=None``: False).  All target columns are used."""

    def __init__(self, args, num_class, num_superpixel, temperature=1.0, reduction='mean'):
        super().__init__(args, num_class, num_superpixel, temperature, reduction)
        self.ignore_only_single = bool(getattr(args, 'group_only_single', False))
        self.sync_normalisers = True

    def _f(self):
        return _lib.LOSS_GROUP | _lib.LOSS_WGROUP | (_lib.LOSS_GROUP_ONLY_MULTI if self.ignore_only_single else 0)

    def _run(self, z, zt, size, targets, superpixels, spmasks):
        _check_superpixels(targets, self.num_superpixel)
        _, _, group, self.last_acc = _wgroup_run(z, zt, size, targets, superpixels, spmasks, self.temp, self._f(), self.sync_normalisers)
        return group

    def forward(self, inputs, plbl_preds, targets, superpixels, spmasks):
        return self._run(inputs, plbl_preds, None, targets, superpixels, spmasks)

    def forward_lowres(self, zq, zq_teacher, size, targets, superpixels, spmasks):
        """``zq`` / ``zq_teacher`` [N,C,h,w]: the training-mode and the eval-mode quarter-resolution logits, both interpolated in
        registers with the same taps -- no ``[N,C,H,W]`` tensor of either exists."""
        return self._run(zq, zq_teacher, size, targets, superpixels, spmasks)


class FusedWGroupLoss(nn.Module):
    """(pos, group) of the ``wgroup`` trainer from ONE forward scan and ONE backward scan: the merged-positive CE (``MultiChoiceCE_``)
    and ``WeightedGroupMultiLabelCE`` at their shared temperature -- each value equal, bit for bit, to the stand-alone module's.
    Shaped like ``FusedTeacherTermLoss``."""

    def __init__(self, num_superpixel, group_temperature=1.0, multi_temperature=1.0, group_only_single=False, sync_normalisers=True):
        super().__init__()
        self.num_superpixel = num_superpixel
        self.temp = _shared_temperature(group_temperature, multi_temperature)
        self.sync_normalisers = sync_normalisers
        self.flags = _lib.LOSS_CE | _lib.LOSS_GROUP | _lib.LOSS_WGROUP | (_lib.LOSS_GROUP_ONLY_MULTI if group_only_single else 0)

    def _run(self, z, zt, size, targets, superpixels, spmasks):
        _check_superpixels(targets, self.num_superpixel)
        pos, _, group, self.last_acc = _wgroup_run(z, zt, size, targets, superpixels, spmasks, self.temp, self.flags, self.sync_normalisers)
        return pos, group

    def forward(self, inputs, plbl_preds, targets, superpixels, spmasks):
        return self._run(inputs, plbl_preds, None, targets, superpixels, spmasks)

    def forward_lowres(self, zq, zq_teacher, size, targets, superpixels, spmasks):
        return self._run(zq, zq_teacher, size, targets, superpixels, spmasks)


class _HierGroupFn(torch.autograd.Function):
    """loss = f(z) of the hierarchical group term (``csrc/hier_group.h``): one library call forward (group scan, pair table, tile-queue
    sum), one backward.  ``size`` None: full-resolution logits, else quarter-resolution ones upsampled inside the kernels.  The
    arg-pixel choice and the pair table carry no gradient.  Returns (loss, acc i64 [2], the bits table both terms see)."""

    @staticmethod
    def forward(ctx, z, size, bits, superpixels, smalls, small_nseg, spmasks, only_single, nocropsp, sync):
        z, spx, sml, msk = z.contiguous(), superpixels.contiguous(), smalls.contiguous(), spmasks.contiguous()
        out = ops.hier_group_loss_fwd(z, size, spx, sml, small_nseg, msk, bits, only_single=only_single, nocropsp=nocropsp,
                                      reduce_acc=_all_reduce_sum if sync else None)
        ctx.save_for_backward(z, sml, msk, out['mult'], out['any'], out['acc'])
        ctx.consts = (size, small_nseg)
        bits_eff = out['bits_eff'] if nocropsp else bits.new_empty(0)          # (nothing cleared: the caller keeps its own table)
        ctx.mark_non_differentiable(out['acc'], bits_eff)
        return out['loss'][0], out['acc'], bits_eff

    @staticmethod
    def backward(ctx, g, _g_acc, _g_bits):
        z, sml, msk, mult, any_, acc = ctx.saved_tensors
        size, small_nseg = ctx.consts
        dz = ops.hier_group_loss_bwd(z, size, sml, small_nseg, msk, mult, any_, acc, g.reshape(1).to(torch.float32).contiguous())
        return (dz,) + (None,) * 9


class HierGroupMultiLabelCE(nn.Module):
    """Hierarchical group loss -- reference ``utils/loss.py:143-235``.  The group term decides one arg-pixel per (superpixel, class of
    its target row, last column dropped); here that decision is spread over the whole FINE superpixel (``superpixel_smalls``, ids in
    ``[0, args.small_nseg)``, pads carry ``small_nseg``) the arg-pixel lies in: ``sum_p sum_c M[small(p), c] * -log(p_c(p) + eps) /
    (1 + sum_p sum_c M[small(p), c])`` over the selected pixels p, with ``M`` the number of arg-pixels of class c inside the fine
    superpixel (pairs are not deduplicated: the reference gathers by index).

    ``temperature`` is accepted and has NO effect: the reference's constructor hands ``temperature=1.0`` to its base class whatever
    it is given (``:145``), so ``--group_ce_temp`` does not reach this term; the softmax runs at 1.0.  ``only_single``
    (``--group_only_single``): only superpixels with more than one target bit choose arg-pixels.  ``gumbel_scale`` other than -1 adds
    torch-sampled Gumbel noise before the arg-max in the reference and cannot be pinned: ``NotImplementedError``.
    ``reduction='none'`` returns ``(sum, 1 + n)``.  Under torch.distributed the sum and the count are all-reduced before the division
    (``sync_normalisers``, see ``_run``); the pair table is per picture and needs no exchange.  No host synchronisation; run-to-run
    identical bytes.

    After a call ``last_bits`` int32 [N,S] holds the target bits the term saw, and ``merged_positive`` evaluates the merged-positive CE
    on them (the same as ``MultiChoiceCE`` for this class; see ``AugHierGroupMultiLabelCE``)."""
    _nocropsp = False

    def __init__(self, args, num_class, num_superpixel, only_single, gumbel_scale, reduction='mean', temperature=1.0):
        super().__init__()
        if gumbel_scale != -1:
            raise NotImplementedError("gumbel_scale=%r: the reference samples torch Gumbel noise before the arg-max, which cannot be "
                                      "reproduced; only -1 (off) exists" % (gumbel_scale,))
        if reduction not in ('mean', 'none'):
            raise NotImplementedError("reduction must be 'mean' or 'none', got %r" % (reduction,))
        self.args = args
        self.num_class = num_class
        self.num_superpixel = num_superpixel
        self.num_small_superpixel = int(args.small_nseg)
        self.only_single = bool(only_single)
        self.gumbel_scale = gumbel_scale
        self.reduction = reduction
        self.eps = 1e-8
        self.temp = 1.0                 # (the reference's base-class call, whatever `temperature` says)
        self.sync_normalisers = True
        self.last_bits = None

    def _run(self, z, size, targets, spmasks, superpixels, superpixel_smalls):
        _check_superpixels(targets, self.num_superpixel)
        bits = ops.target_bits(_u8(targets), targets.shape[-1] - 1)
        size = _hw(size)
        loss, self.last_acc, cleared = _HierGroupFn.apply(z, size, bits, superpixels, superpixel_smalls, self.num_small_superpixel, spmasks,
                                                          self.only_single, self._nocropsp, self.sync_normalisers)
        self.last_bits = cleared if self._nocropsp else bits
        if self.reduction == 'mean':
            return loss
        num_valid = self.last_acc[1] + 1
        return loss * num_valid.to(torch.float32), num_valid

    def forward(self, inputs, targets, spmasks, superpixels, superpixel_smalls):
        return self._run(inputs, None, targets, spmasks, superpixels, superpixel_smalls)

    def forward_lowres(self, zq, size, targets, spmasks, superpixels, superpixel_smalls):
        """``zq`` [N,C,h,w]: the quarter-resolution logits, interpolated in registers -- no ``[N,C,H,W]`` tensor exists."""
        return self._run(zq, size, targets, spmasks, superpixels, superpixel_smalls)

    def merged_positive(self, inputs, size, superpixels, spmasks, temperature):
        """The merged-positive CE (``MultiChoiceCE``, last target column dropped) at ``temperature`` on ``last_bits``, the rows this
        term saw in its last call."""
        if self.last_bits is None:
            raise RuntimeError("merged_positive reads the bits of the last forward; call the loss first")
        size = _hw(size)
        ce, _, _, _ = _PartialLossFn.apply(inputs, size, self.last_bits, None, superpixels, spmasks, ops.inv_temperature(temperature),
                                           _lib.LOSS_CE, self.sync_normalisers)
        return ce


class AugHierGroupMultiLabelCE(HierGroupMultiLabelCE):
    """``HierGroupMultiLabelCE`` for ``--nocropsp`` -- reference ``utils/loss.py:439-533``: every superpixel id (other than ``nseg``)
    that occurs on the outermost row or column of the crop has its target row cleared before the arg-pixels are chosen.

    The reference clears the rows IN PLACE through a view of the trainer's ``labels`` (``:493-498``), and the trainer calls the
    merged-positive loss afterwards on the same tensor: under ``--nocropsp`` the cleared rows are missing from BOTH terms.  That
    effective objective is what is built here, without touching the caller's tensor: the rows are cleared in a copy of the bits table
    on the device (``last_bits``), and ``merged_positive`` gives the second term on it."""
    _nocropsp = True


class _AsyncHierFn(torch.autograd.Function):
    """loss = f(z) of the cross-view hierarchical group term on given tables (``csrc/hier_group.h``, second section): the tile-queue sum
    over the strong view forward, one backward.  The tables come from the teacher's view and carry no gradient.  Returns (loss, acc)."""

    @staticmethod
    def forward(ctx, z, size, smalls, small_nseg, spmasks, mult, any_, wgt, sync):
        z, sml, msk = z.contiguous(), smalls.contiguous(), spmasks.contiguous()
        loss, acc = ops.async_hier_loss_fwd(z, size, sml, small_nseg, msk, mult, any_, wgt, reduce_acc=_all_reduce_sum if sync else None)
        saved = (z, sml, msk, mult, any_, acc) + (() if wgt is None else (wgt,))
        ctx.save_for_backward(*saved)
        ctx.consts = (size, small_nseg)
        ctx.mark_non_differentiable(acc)
        return loss[0], acc

    @staticmethod
    def backward(ctx, g, _g_acc):
        z, sml, msk, mult, any_, acc = ctx.saved_tensors[:6]
        wgt = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
        size, small_nseg = ctx.consts
        dz = ops.async_hier_loss_bwd(z, size, sml, small_nseg, msk, mult, any_, wgt, acc, g.reshape(1).to(torch.float32).contiguous())
        return (dz,) + (None,) * 8


class AsyncHierGroupMultiLabelCE(HierGroupMultiLabelCE):
    """Cross-view hierarchical group loss -- reference ``utils/loss.py:341-437``.  Two views of one picture: on the WEAK view (the whole
    picture, seen by an eval-mode teacher) every (superpixel, class of its target row, last column dropped) chooses its arg-pixel among
    the pixels of ``spmasks_weak``, and the pair (fine superpixel of that pixel in ``spx_smalls_weak``, class) is kept; on the STRONG
    view (the student's augmented crop) every selected pixel whose fine id in ``superpixel_smalls`` holds a pair pays ``M * -log(p_c +
    eps)``, normalised by ``1 + sum M`` over those pixels.  The fine ids are the only link between the two geometries.

    ``forward(inputs, inputs_weak, targets, spmasks, spmasks_weak, superpixels, superpixels_weak, superpixel_smalls, spx_smalls_weak)``
    is the reference's signature on full-resolution logits of both views; ``forward_lowres`` takes quarter-resolution logits and the
    two sizes.  ``superpixels`` (the strong view's coarse ids) is not read by this term, as in the reference.

    ``temperature`` is accepted and has NO effect (the base constructor is handed 1.0 whatever it is given); ``only_single`` is stored
    and NOT read, as in the reference's two classes -- the parser refuses ``--group_only_single`` for their trainers rather than ignore
    it.  ``gumbel_scale`` other than -1: ``NotImplementedError``.  A pair whose summed value is exactly 0 over a non-empty fine
    superpixel is counted here and not in the reference (``size[value.nonzero()]``)."""
    _weight_reduce = None

    def _tables(self, zw, size_weak, bits, spmasks_weak, superpixels_weak, spx_smalls_weak):
        with torch.no_grad():
            return ops.async_hier_tables(zw.detach().contiguous(), size_weak, superpixels_weak.contiguous(), spx_smalls_weak.contiguous(),
                                         self.num_small_superpixel, spmasks_weak.contiguous(), bits, weight_reduce=self._weight_reduce)

    def _run(self, z, size, zw, size_weak, targets, spmasks, spmasks_weak, superpixels_weak, superpixel_smalls, spx_smalls_weak):
        _check_superpixels(targets, self.num_superpixel)
        bits = ops.target_bits(_u8(targets), targets.shape[-1] - 1)
        size = _hw(size)
        size_weak = _hw(size_weak)
        self.last_tables = tab = self._tables(zw, size_weak, bits, spmasks_weak, superpixels_weak, spx_smalls_weak)
        loss, self.last_acc = _AsyncHierFn.apply(z, size, superpixel_smalls, self.num_small_superpixel, spmasks, tab['mult'], tab['any'],
                                                 tab['wgt'], self.sync_normalisers)
        self.last_bits = bits
        if self.reduction == 'mean':
            return loss
        num_valid = self.last_acc[1] + 1
        return loss * num_valid.to(torch.float32), num_valid

    def forward(self, inputs, inputs_weak, targets, spmasks, spmasks_weak, superpixels, superpixels_weak, superpixel_smalls, spx_smalls_weak):
        return self._run(inputs, None, inputs_weak, None, targets, spmasks, spmasks_weak, superpixels_weak, superpixel_smalls, spx_smalls_weak)

    def forward_lowres(self, zq, size, zq_weak, size_weak, targets, spmasks, spmasks_weak, superpixels, superpixels_weak, superpixel_smalls,
                       spx_smalls_weak):
        """``zq`` [N,C,h,w] and ``zq_weak`` [N,C,h_o,w_o]: the quarter-resolution logits of the two views, interpolated in registers to
        ``size`` and ``size_weak`` -- no full-resolution tensor of either view exists."""
        return self._run(zq, size, zq_weak, size_weak, targets, spmasks, spmasks_weak, superpixels_weak, superpixel_smalls, spx_smalls_weak)


class WeightAsyncHierGroupMultiLabelCE(AsyncHierGroupMultiLabelCE):
    """``AsyncHierGroupMultiLabelCE`` with the teacher's confidence -- reference ``utils/loss.py:237-339``: every pair's summed value is
    multiplied by the detached ``weight_reduce`` ('max', the default, or 'mean') of the teacher's ``p_c`` over the selected weak-view
    pixels of the pair's fine superpixel, and a pair of weight exactly 0 leaves the count.  The reference's mean is an f32 sum in source
    order; here it is a fixed-point sum rounded once (``csrc/hier_group.h``)."""

    def __init__(self, args, num_class, num_superpixel, only_single, gumbel_scale, reduction='mean', temperature=1.0, weight_reduce='max'):
        super().__init__(args, num_class, num_superpixel, only_single, gumbel_scale, reduction, temperature)
        if weight_reduce not in ('max', 'mean'):
            raise ValueError("weight_reduce must be 'max' or 'mean', got %r" % (weight_reduce,))
        self.weight_reduce = self._weight_reduce = weight_reduce
