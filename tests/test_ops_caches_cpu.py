"""The derived constants ``ops`` caches on a module (``_bn_fold``, ``_conv1x1_constants``) without a GPU: kept while nothing changes,
rebuilt after an in-place update of a running statistic and after ``invalidate_parameter_caches()``, and equal to the float64 fold."""
import torch

from mulactseg_amd import ops


def _bn(seed=0):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(8).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(8, generator=g))
        bn.bias.copy_(torch.randn(8, generator=g))
        bn.running_mean.copy_(torch.randn(8, generator=g))
        bn.running_var.copy_(torch.rand(8, generator=g) + 0.1)
    return bn


def _fold64(bn):
    inv = torch.rsqrt(bn.running_var.double() + bn.eps)
    scale = bn.weight.detach().double() * inv
    shift = bn.bias.detach().double() - bn.running_mean.double() * scale
    return scale.float(), shift.float()


def _same_objects(a, b):
    return len(a) == len(b) and all(x is y for x, y in zip(a, b))


def _check_invalidation(get, bn, from_statistics):
    """get() returns the identical tensors until something they derive from changes: the entries ``from_statistics`` are rebuilt after
    an in-place update of a running statistic, every entry after the caches are invalidated by hand."""
    first = get()
    assert _same_objects(get(), first)
    bn.running_var.add_(1)
    second = get()
    assert all(second[i] is not first[i] for i in from_statistics)
    assert _same_objects(get(), second)
    ops.invalidate_parameter_caches()
    third = get()
    assert not any(x is y for x, y in zip(third, second))
    assert _same_objects(get(), third)


def test_bn_fold_is_cached_until_a_statistic_or_the_epoch_changes():
    bn = _bn()
    _check_invalidation(lambda: ops._bn_fold(bn), bn, (0, 1))


def test_bn_fold_is_the_float64_formula_cast_to_f32():
    bn = _bn(1)
    scale, shift = ops._bn_fold(bn)
    want_scale, want_shift = _fold64(bn)
    assert scale.dtype == shift.dtype == torch.float32
    assert torch.equal(scale, want_scale) and torch.equal(shift, want_shift)
    bn.running_var.add_(1)
    scale, shift = ops._bn_fold(bn)
    want_scale, want_shift = _fold64(bn)
    assert torch.equal(scale, want_scale) and torch.equal(shift, want_shift)


def test_conv1x1_constants_follow_the_same_rules_and_share_the_fold():
    bn = torch.nn.BatchNorm2d(32).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(32, generator=torch.Generator().manual_seed(2)))
        bn.running_var.copy_(torch.rand(32, generator=torch.Generator().manual_seed(3)) + 0.1)
    conv = torch.nn.Conv2d(8, 32, 1, bias=False)
    _check_invalidation(lambda: ops._conv1x1_constants(conv, bn), bn, (1, 2))        # (scale, shift; the weight did not change)
    w_t, scale, shift = ops._conv1x1_constants(conv, bn)
    fold_scale, fold_shift = ops._bn_fold(bn)
    assert torch.equal(scale, fold_scale) and torch.equal(shift, fold_shift)
    assert torch.equal(w_t, conv.weight.detach().reshape(32, 8).t())
