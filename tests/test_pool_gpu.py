"""csrc/pool.hip against torch.nn.MaxPool2d(3, 2, 1) on the CPU: values and gradients exactly (a maximum is exact; each
input receives at most four gradient terms, summed in a fixed order), odd sizes, ties, -inf, NaN, rows wider than one
workgroup, determinism."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _check_against_aten(x, g):
    """Values (NaN where ATen has NaN, equal elsewhere), gradients and run-to-run identity of ops.maxpool3s2 on ``x``."""
    from mulactseg_amd import ops
    pool = nn.MaxPool2d(3, 2, 1)
    xr = x.clone().requires_grad_(True)
    yr = pool(xr)
    go = torch.randn(yr.shape, generator=g)
    yr.backward(go)
    xd = x.cuda().requires_grad_(True)
    assert ops.maxpool3s2_supported(pool, xd)
    yd = ops.maxpool3s2(xd)
    got, want = yd.detach().cpu(), yr.detach()
    assert got.shape == want.shape
    assert torch.equal(got.isnan(), want.isnan())
    assert torch.equal(got[~want.isnan()], want[~want.isnan()])
    yd.backward(go.cuda())
    assert torch.isfinite(xr.grad).all()
    assert float((xd.grad.cpu() - xr.grad).abs().max()) <= 1e-6 * max(1.0, float(xr.grad.abs().max()))
    assert torch.equal(xd.grad.cpu() != 0, xr.grad != 0)              # the same pixels were selected
    first = xd.grad.clone()
    xd.grad = None
    ops.maxpool3s2(xd).backward(go.cuda())
    assert torch.equal(first, xd.grad)
    return xd, want


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 16, 20), (1, 4, 17, 23), (2, 2, 1, 5), (1, 8, 96, 192), (1, 1, 2, 2), (1, 3, 385, 385), (2, 2, 33, 41)])
def test_maxpool_matches_pytorch(N, C, H, W):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.randn((N, C, H, W), generator=g)
    x = (x * 2).round() / 2                       # plenty of exact ties
    x[0, 0, 0, :2] = float('-inf')
    xd, y = _check_against_aten(x, g)
    assert not y.isnan().any()
    assert not ops.maxpool3s2_supported(nn.MaxPool2d(2, 2), xd)


@pytest.mark.parametrize("N,C,H,W,Wo,fwd_groups,bwd_groups", [(1, 1, 3, 2051, 1026, 2, 5), (1, 2, 4, 2048, 1024, 1, 4)])
def test_maxpool_rows_wider_than_one_workgroup(N, C, H, W, Wo, fwd_groups, bwd_groups):
    """blockIdx.x > 0: the forward workgroup covers 4 * 256 outputs of a row, the backward one 256 column pairs."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ((W - 1) // 2 + 1, (Wo + 1023) // 1024, ((W + 1) // 2 + 255) // 256) == (Wo, fwd_groups, bwd_groups)
    g = torch.Generator().manual_seed(H * 31 + W)
    x = (torch.randn((N, C, H, W), generator=g) * 2).round() / 2
    x[0, 0, 0, :2] = float('-inf')
    _, y = _check_against_aten(x, g)
    assert y.shape[-1] == Wo


def test_maxpool_nan_rule():
    """ATen's scan, 'val > max || isnan(val)': a NaN takes the window, the last NaN of a window takes its gradient.  NaNs alone in
    their windows, two in one window, one in the first column (beside the padding), one in the element-by-element end of a 23-wide row."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g = torch.Generator().manual_seed(23)
    x = (torch.randn((1, 3, 9, 23), generator=g) * 2).round() / 2
    nan = float('nan')
    x[0, 0, 4, 10] = nan                          # alone: an even row and column, inside one window only
    x[0, 0, 7, 15] = nan                          # alone: an odd row and column, shared by four windows
    x[0, 1, 2, 4] = nan; x[0, 1, 2, 5] = nan      # two in the window of output (1, 2), which spans rows 1..3, columns 3..5
    x[0, 1, 6, 0] = nan                           # first column
    x[0, 2, 5, 20] = nan; x[0, 2, 4, 22] = nan    # the last group of a 23-wide row (columns 15..22) goes element by element
    assert 16 + 7 >= 23                           # (k_maxpool3s2_fwd: `vec` is false for the lane whose c0 = 16)
    _, y = _check_against_aten(x, g)
    assert int(y.isnan().sum()) == 1 + 4 + 2 + 1 + 2 + 1


def test_maxpool_window_of_minus_infinity():
    """A whole 3x3 window of -inf (and a corner window, 2x2 inside the plane): the value is -inf, the gradient goes to the window's first
    pixel, as in ATen."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((1, 2, 8, 12), generator=g) * 2).round() / 2
    x[0, 0, 3:6, 3:6] = float('-inf')             # output (2, 2)
    x[0, 1, 0:2, 0:2] = float('-inf')             # output (0, 0)
    x[0, 1, 5:8, 9:12] = float('-inf')            # output (3, 5): rows 5..7, columns 9..11
    xd, y = _check_against_aten(x, g)
    assert y[0, 0, 2, 2] == float('-inf') and y[0, 1, 0, 0] == float('-inf') and y[0, 1, 3, 5] == float('-inf')
    assert float(xd.grad[0, 0, 3, 3]) != 0.0 and float(xd.grad[0, 1, 0, 0]) != 0.0 and float(xd.grad[0, 1, 5, 9]) != 0.0
