"""``--save_vis`` / ``eval_naive_vis`` on the host: the numpy restatement of csrc/render.hip on hand-worked maps with literal expected
outputs (skimage's outer boundaries, the float64 round trip of its ``img_as_float``), the parser flag, the import surface of
``--method eval_naive_vis`` and the argument checks of the two C entry points.  The kernels run in tests/test_render_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_restated as R
from mulactseg_amd.dataloader.constant import train_id_to_color, voc_id_to_color_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = np.iinfo(np.int64).max
CITY = train_id_to_color.astype(np.uint8)


def _marks(s):
    return R.outer_boundaries(np.array(s, dtype=np.int64)).astype(int).tolist()


# -- outer boundaries on hand-worked maps ---------------------------------------------------------------------------------------
def test_a_border_between_two_ids_is_marked_on_both_sides():
    s = [[1, 1, 1, 2, 2, 2]] * 5
    assert _marks(s) == [[0, 0, 1, 1, 0, 0]] * 5


def test_a_border_with_id_zero_is_marked_on_the_zero_side_only():
    s = [[5, 5, 5, 0, 0, 0]] * 5
    assert _marks(s) == [[0, 0, 0, 1, 0, 0]] * 5
    s = [[0, 0, 0, 5, 5, 5]] * 5                       # (the mirror image)
    assert _marks(s) == [[0, 0, 1, 0, 0, 0]] * 5


def test_id_zero_in_a_corner():
    s = np.full((5, 6), 7)
    s[:2, :2] = 0
    assert _marks(s) == [[0, 1, 0, 0, 0, 0],
                         [1, 1, 0, 0, 0, 0],
                         [0, 0, 0, 0, 0, 0],
                         [0, 0, 0, 0, 0, 0],
                         [0, 0, 0, 0, 0, 0]]


def test_one_pixel_wide_and_one_row_pictures():
    """The picture's edge is its own neighbour: no boundary along it."""
    assert _marks([[1], [1], [2], [2], [0]]) == [[0], [1], [1], [0], [1]]
    assert _marks([[0, 3, 3, 4, 4, 4]]) == [[1, 0, 1, 1, 0, 0]]
    assert _marks([[9]]) == [[0]] and _marks([[0]]) == [[0]]


def test_an_id_equal_to_int64_max():
    """The background's stand-in value: an id M next to id 0 is not marked (as an id v next to 0), next to another id it is."""
    s = [[3, 3, M, M, 0, 0]] * 5
    assert _marks(s) == [[0, 1, 1, 0, 1, 0]] * 5


def test_a_diagonal_neighbour_alone_marks_nothing():
    s = [[1, 1, 1, 1, 1, 1],
         [1, 1, 1, 1, 1, 1],
         [1, 1, 2, 1, 1, 1],
         [1, 1, 1, 1, 1, 1],
         [1, 1, 1, 1, 1, 1]]
    assert _marks(s) == [[0, 0, 0, 0, 0, 0],
                         [0, 0, 1, 0, 0, 0],
                         [0, 1, 1, 1, 0, 0],
                         [0, 0, 1, 0, 0, 0],
                         [0, 0, 0, 0, 0, 0]]


# -- colours ----------------------------------------------------------------------------------------------------------------------
def test_round_trip_truncates_24_byte_values():
    v = np.arange(256, dtype=np.uint8)
    formula = np.array([int(float(c) * (1.0 / 255) * 255) for c in range(256)], dtype=np.uint8)
    assert np.array_equal(R.round_trip(v), formula)
    low = [int(c) for c in v[R.round_trip(v) != v]]
    assert low == [33, 37, 41, 45, 49, 53, 57, 61, 66, 74, 82, 90, 98, 106, 114, 122, 132, 148, 164, 180, 196, 212, 228, 244]
    assert np.all(R.round_trip(low) == np.array(low) - 1)


def test_sidewalk_and_sky_lose_one_step_away_from_boundaries():
    lab = np.array([[1, 1, 10, 10, 255, 19]] * 5)
    spx = np.ones((1, 5, 6), dtype=np.int64)
    got = R.render_labels(lab[None], CITY, 20, spx)[0]
    assert got[2, 0].tolist() == [243, 35, 232]            # sidewalk (244, 35, 232)
    assert got[2, 2].tolist() == [70, 130, 179]            # sky (70, 130, 180)
    assert got[2, 4].tolist() == [255, 255, 255]           # 255 painted 20, "unselected"
    assert got[2, 5].tolist() == [0, 0, 0]                 # 19, "undefined"
    plain = R.render_labels(lab[None], CITY, 20)[0]
    assert plain[2, 0].tolist() == [244, 35, 232] and plain[2, 2].tolist() == [70, 130, 180]


def test_marked_pixels_are_yellow():
    lab = np.zeros((1, 5, 6), dtype=np.int64)
    spx = np.array([[[1, 1, 1, 2, 2, 2]] * 5], dtype=np.int64)
    got = R.render_labels(lab, CITY, 20, spx)[0]
    assert got[:, 2:4].reshape(-1, 3).tolist() == [[255, 255, 0]] * 10
    assert got[:, [0, 1, 4, 5]].reshape(-1, 3).tolist() == [[128, 64, 128]] * 20


def test_voc_colours_survive_the_round_trip():
    assert voc_id_to_color_map.shape == (22, 3)
    assert np.array_equal(R.round_trip(voc_id_to_color_map), voc_id_to_color_map)
    lab = np.arange(22).reshape(1, 2, 11)
    lab[0, 1, 10] = 255
    got = R.render_labels(lab, voc_id_to_color_map, 21, np.ones((1, 2, 11), dtype=np.int64))[0]
    assert got[1, 10].tolist() == [255, 255, 255] and got[0, 1].tolist() == [128, 0, 0] and got[1, 4].tolist() == [192, 128, 128]   # (15, person)


def test_a_label_outside_the_palette_raises_in_the_restatement():
    with pytest.raises(IndexError):
        R.render_labels(np.array([[[21]]]), CITY, 20)


def test_first_argmax_follows_torch_max():
    nan = np.float32(np.nan)
    z = np.array([[1, 3, 3, 0], [nan, 1, 2, 9], [0, nan, nan, 9], [2, 2, 1, 9]], dtype=np.float32)[:, :, None, None]   # [4,4,1,1]
    want = torch.from_numpy(z).max(dim=1)[1].numpy()
    assert np.array_equal(R.first_argmax(z), want) and want[:, 0, 0].tolist() == [1, 0, 1, 3]
    assert R.render_pred(z, CITY)[:, 0, 0].tolist() == [CITY[1].tolist(), CITY[0].tolist(), CITY[1].tolist(), CITY[0].tolist()]


# -- the parser, the import surface, the C entry points ---------------------------------------------------------------------------
@pytest.mark.parametrize("module", ["common", "common_voc"])
def test_parsers_take_save_vis(module):
    import importlib
    parser = importlib.import_module("mulactseg_amd.utils." + module).get_parser()
    assert parser.parse_args([]).save_vis is False
    assert parser.parse_args(['--save_vis']).save_vis is True


def test_eval_naive_vis_imports_under_the_reference_names():
    code = ("import mulactseg_amd, importlib\n"
            "mulactseg_amd.install_aliases()\n"
            "t = importlib.import_module('trainer.eval_naive_vis')\n"
            "n = importlib.import_module('trainer.eval_naive')\n"
            "assert issubclass(t.ActiveTrainer, n.ActiveTrainer)\n"
            "assert t.ActiveTrainer.predicts_ignore is True\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_generators_paint_with_their_dataset_palette():
    from mulactseg_amd.trainer import (eval_save_cosplbl_prop, eval_save_cosplbl_prop_includeonehot_slide,
                                       eval_save_cosplbl_prop_includeonehot_voc, eval_save_cosplbl_prop_includeonehot_voc_ms,
                                       eval_save_cosplbl_prop_onehotignore)
    for mod in (eval_save_cosplbl_prop, eval_save_cosplbl_prop_onehotignore, eval_save_cosplbl_prop_includeonehot_slide):
        assert mod.ActiveTrainer.vis_fill == 20 and mod.ActiveTrainer.vis_palette is train_id_to_color
    for mod in (eval_save_cosplbl_prop_includeonehot_voc, eval_save_cosplbl_prop_includeonehot_voc_ms):
        assert mod.ActiveTrainer.vis_fill == 21 and mod.ActiveTrainer.vis_palette is voc_id_to_color_map


def test_render_argument_errors_are_reported_without_the_gpu():
    from mulactseg_amd import _lib, ops
    lib = _lib.load()
    fake = 256                                                   # never dereferenced: every call below fails its argument checks
    I64, U8 = _lib.ID_I64, _lib.MAP_U8
    assert lib.mas_render_labels(None, I64, 1, 4, 4, fake, 21, 20, None, 0, fake, fake, None) == -1
    assert lib.mas_render_labels(fake, I64, 1, 4, 4, fake, 21, 20, None, 0, fake, None, None) == -1        # no error counter
    assert lib.mas_render_labels(fake, I64, 1, 4, 4, fake, 21, 20, None, 1, fake, fake, None) == -1        # marks without ids
    assert lib.mas_render_labels(fake, _lib.ID_I32, 1, 4, 4, fake, 21, 20, None, 0, fake, fake, None) == -4
    assert lib.mas_render_labels(fake, U8, 0, 4, 4, fake, 21, 20, None, 0, fake, fake, None) == -2
    assert lib.mas_render_labels(fake, U8, 1, 4, 4, fake, 257, 20, None, 0, fake, fake, None) == -6        # palette > 256
    assert lib.mas_render_labels(fake, U8, 1, 4, 4, fake, 21, 21, None, 0, fake, fake, None) == -6         # fill outside
    assert lib.mas_render_labels(fake, U8, 1, 4, 4, fake, 21, 20, None, 0, fake + 1, fake, None) == -5     # rgb not 4-aligned
    assert lib.mas_render_lowres_pred(None, 1, 20, 8, 8, 32, 32, fake, 21, fake, fake, None) == -1
    assert lib.mas_render_lowres_pred(fake, 1, 1, 8, 8, 32, 32, fake, 21, fake, fake, None) == -3          # no class channel
    assert lib.mas_render_lowres_pred(fake, 1, 20, 64, 64, 32, 32, fake, 21, fake, fake, None) == -2       # a downsampling
    assert lib.mas_render_lowres_pred(fake, 1, 20, 8, 8, 8, 64, fake, 21, fake, fake, None) == -2          # wider than x6
    assert lib.mas_render_lowres_pred(fake, 1, 20, 8, 8, 32, 32, fake, 18, fake, fake, None) == -6         # palette < CH - 1
    assert lib.mas_render_lowres_pred(fake, 1, 20, 8, 8, 32, 32, fake, 21, fake, fake + 2, None) == -5
    pal = torch.from_numpy(CITY)
    with pytest.raises(_lib.MulActSegHipError, match="GPU"):
        ops.render_labels(torch.zeros((1, 4, 4), dtype=torch.int64), pal, 20)
    with pytest.raises(_lib.MulActSegHipError, match="GPU"):
        ops.render_lowres_pred(torch.zeros((1, 20, 8, 8)), (32, 32), pal)
