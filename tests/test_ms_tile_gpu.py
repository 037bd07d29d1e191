"""``ops.ms_ensemble`` on the shared two-stage tile (csrc/ms_tile.h), bit for bit against the numpy restatement
(tests/ms_ensemble_restated.py), at the two geometries the cases of tests/test_ms_ensemble_gpu.py leave open: a channel block that
mixes feature and logit slots, and a stage-2 downsample by two."""
import numpy as np
import pytest

import ms_ensemble_restated as R
from test_ms_ensemble_gpu import _gpu, _run, _sources

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", [[0, 9], [4]])
def test_a_channel_block_that_straddles_features_and_logits_is_bit_exact(which):
    """Ch = 5, C = 6: channel block 0 holds five feature and three logit slots, block 1 the three logits that remain (every case of
    test_ms_ensemble_gpu.py has Ch a multiple of the block, so a block is all features or all logits and only the last one is partial)."""
    _gpu()
    H, W, Ch, C = 37, 45, 5, 6
    sizes, flips = R.tta_sizes(H, W)
    sizes, flips = [sizes[i] for i in which], [flips[i] for i in which]
    fq, lq = _sources(np.random.RandomState(37 + len(which)), sizes, Ch, C)
    got_f, got_z = _run(fq, lq, sizes, flips, (H, W))
    want_f, want_z = R.ms_ensemble(fq, lq, sizes, flips, (H, W))
    assert np.array_equal(got_z, want_z), np.abs(got_z - want_z).max()
    assert np.array_equal(got_f, want_f), np.abs(got_f - want_f).max()


def test_a_stage2_downsample_by_two_is_bit_exact():
    """Factors 1.0 and 2.0 and their flips.  By the restatement's taps a tile of the factor-2.0 sources needs at most 6 quarter rows x 64
    stage-1 columns = 384 (row, column) positions in stage A (factor 1.0: 4 x 33 = 132): more than one per thread, so both position
    slots of a thread are in use, but not more than the 2 x 256 of one load round -- this geometry does not reach the second round.
    (tests/test_ms_eval_gpu.py walks the same stage A to the largest factor the LDS admits.)"""
    _gpu()
    H, W, Ch, C = 40, 96, 8, 3
    sizes, flips = R.tta_sizes(H, W, factors=(1.0, 2.0))
    positions = []
    for Hs, Ws in sizes:
        (y0, y1, _, _), (x0, x1, _, _) = R.taps(Hs, H), R.taps(Ws, W)
        (q0, q1, _, _) = R.taps(R.quarter_size(Hs), Hs)
        positions.append(max(int((q1[y1[min(ty + 8, H) - 1]] - q0[y0[ty]] + 1) * (x1[min(tx + 32, W) - 1] - x0[tx] + 1))
                             for ty in range(0, H, 8) for tx in range(0, W, 32)))
    assert positions == [132, 384, 132, 384]
    fq, lq = _sources(np.random.RandomState(4096), sizes, Ch, C)
    got_f, got_z = _run(fq, lq, sizes, flips, (H, W))
    want_f, want_z = R.ms_ensemble(fq, lq, sizes, flips, (H, W))
    assert np.array_equal(got_z, want_z), np.abs(got_z - want_z).max()
    assert np.array_equal(got_f, want_f), np.abs(got_f - want_f).max()
