"""The host half of the shared two-stage tile (csrc/ms_tile.h) without a GPU: the LDS extents that ``ms_tile_extents`` computes for
k_ms_ensemble and k_ms_naive, through ``ops.ms_iou_lds_bytes``, against bytes recorded before the sizing loop moved into the header."""
import pytest

TTA = (0.5, 0.75, 1.0, 1.25, 1.5)
LDS_BYTES = [  # (factors, flips, out_size, bytes): what the library of commit 53fe737 (the last one with the sizing loop inside
    # ms_naive.hip) returns, static counters included; each geometry at a multiple of the 8 x 32 tile and at a size that is none
    (TTA, (False, True), (375, 500), 28044), (TTA, (False, True), (376, 512), 26508),
    (TTA, (False, True), (1024, 2048), 26508), (TTA, (False, True), (1023, 2047), 28620),
    ((0.5,), (False,), (120, 160), 5580), ((0.5,), (False,), (121, 161), 5580),
    ((1.0,), (False,), (120, 160), 14124), ((1.0,), (False,), (121, 161), 15180),
    ((2.0,), (False,), (120, 160), 45452), ((2.0,), (False,), (121, 161), 45452),
    ((3.0,), (False,), (120, 160), 94636), ((3.0,), (False,), (121, 161), 94636),       # beyond 64 KB: still the byte count
    ((1.25,), (True,), (120, 160), 19596), ((1.25,), (True,), (121, 161), 21388),
    ((2.0,), (True,), (120, 160), 45452), ((2.0,), (True,), (121, 161), 45452),
]


@pytest.mark.parametrize("factors, flips, out_size, want", LDS_BYTES)
def test_the_lds_sizing_returns_the_recorded_bytes(factors, flips, out_size, want):
    from mulactseg_amd import ops
    H, W = out_size
    table = [v for fl in flips for f in factors
             for v in (ops.quarter_size(int(f * H)), ops.quarter_size(int(f * W)), int(f * H), int(f * W), int(fl))]
    assert ops.ms_iou_lds_bytes(table, (H, W)) == want
