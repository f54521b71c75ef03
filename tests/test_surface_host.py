"""Host half of the spacing-aware surface metrics (gts.metrics): the integer units of a spacing,
the exact tolerance thresholds, the range guard and the argument checks of the C entry points, and the new
flags of scripts.score_predictions.  None of it needs a GPU."""
import ctypes
import math

import numpy as np
import pytest

from tests import surface_ref


def _units(*u):
    return (ctypes.c_int64 * 3)(*u)


def test_spacing_units_examples():
    from gts.metrics import spacing_units

    assert spacing_units((1, 1, 1)) == ((1, 1, 1), 1.0)
    assert spacing_units((0.5, 0.5, 0.5)) == ((1, 1, 1), 0.5)
    assert spacing_units((0.9375, 0.9375, 5)) == ((15, 15, 80), 0.0625)
    assert spacing_units((1.0, 0.94, 3.3333)) == ((10000, 9400, 33333), 0.0001)
    assert spacing_units(np.array([1, 1, 5], dtype=np.float32)) == ((1, 1, 5), 1.0)
    assert spacing_units((100, 100, 100)) == ((100, 100, 100), 1.0)
    assert spacing_units((2, 2, 3)) == ((2, 2, 3), 1.0)
    assert spacing_units((0.0001, 0.0002, 100)) == ((1, 2, 1000000), 0.0001)
    for spacing in ((1, 1, 5), (0.9375, 0.9375, 5), (0.47, 0.47, 1.5), (1.0, 0.94, 3.3333)):
        units, scale = spacing_units(spacing)
        ref_units, g = surface_ref.units_of(spacing)
        assert units == ref_units and scale == g / 10000.0 and math.gcd(*units, 10000 // g) == 1


@pytest.mark.parametrize("spacing", [(0, 1, 1), (1, -1, 1), (1, 1, float("nan")), (1, float("inf"), 1),
                                     (1, 1, 100.0001), (1, 1, 0.00004), (1, 1), (1, 1, 1, 1)])
def test_spacing_units_refuses(spacing):
    from gts import GtsError
    from gts.metrics import spacing_units, tolerance_thresholds

    with pytest.raises(GtsError):
        spacing_units(spacing)
    with pytest.raises(GtsError):
        tolerance_thresholds((1.0,), spacing)


def test_thresholds_are_exact_integers_at_ties():
    from gts import GtsError
    from gts.metrics import tolerance_thresholds

    assert tolerance_thresholds((5.0, 2.0), (1, 1, 5)) == [25, 4]          # one 5 mm slice lies within 5.0 mm
    assert tolerance_thresholds((0.5, 1.0, 2.0, 5.0), (1, 1, 5)) == [0, 1, 4, 25]
    assert tolerance_thresholds((), (1, 1, 5)) == []
    # 0.9375 x 0.9375 x 5: g = 625 steps; one in-plane voxel is D2 = 225 = (0.9375 / 0.0625)^2
    assert tolerance_thresholds((0.9375, 0.9374, 5.0), (0.9375, 0.9375, 5)) == [225, 224, 6400]
    for spacing in ((1, 1, 5), (0.9375, 0.9375, 5), (0.47, 0.47, 1.5), (1.0, 0.94, 3.3333)):
        _, g = surface_ref.units_of(spacing)
        for tol in (0.0, 0.0001, 0.5, 1.0, 1.4142, 2.0, 5.0, 99.99):
            t = surface_ref.steps_of(tol)
            (got,) = tolerance_thresholds((tol,), spacing)
            assert got * g * g <= t * t < (got + 1) * g * g, (spacing, tol)
    assert tolerance_thresholds((1e9,), (0.0001, 0.0001, 0.0001)) == [1 << 62]      # capped above every D2
    with pytest.raises(GtsError):
        tolerance_thresholds((-0.5,), (1, 1, 1))
    with pytest.raises(GtsError):
        tolerance_thresholds((float("nan"),), (1, 1, 1))
    with pytest.raises(GtsError):
        tolerance_thresholds((1, 2, 3, 4, 5), (1, 1, 1))


def test_workspace_guard(hip_lib):
    ws = hip_lib.gts_surface_workspace
    assert ws(240, 240, 155, _units(10000, 9400, 33333)) > 0
    assert ws(240, 240, 155, _units(100000, 100000, 100000)) > 0            # 10 mm in 1e-4 mm steps, no common factor taken
    assert ws(240, 240, 155, _units(1, 1, 1)) > 240 * 240 * 155 * (1 + 12 + 48 + 48)
    for extents in ((0, 8, 8), (8, -1, 8), (8, 8, 0)):
        assert ws(*extents, _units(1, 1, 1)) == 0
    assert ws(4097, 4097, 4097, _units(99991, 99989, 99971)) == 0           # 2^31 voxels or more, and B overflows
    assert ws(1, 1, 4097, _units(1, 1, 99971)) == 0                         # B * max(N) = 2^69
    assert ws(1, 1, 4097, _units(1, 1, 1)) > 0 and ws(1, 1, 4098, _units(1, 1, 1)) == 0
    # the bound itself: B * N < 2^62 with B = u^2 (N - 1)^2
    n = 1025
    u_ok = math.isqrt(((1 << 62) - 1) // (n * (n - 1) ** 2))
    assert u_ok ** 2 * (n - 1) ** 2 * n < (1 << 62) <= (u_ok + 1) ** 2 * (n - 1) ** 2 * n and u_ok <= 1000000
    assert ws(1, 1, n, _units(1, 1, u_ok)) > 0 and ws(1, 1, n, _units(1, 1, u_ok + 1)) == 0
    for bad in ((0, 1, 1), (1, -3, 1), (1, 1, 1000001)):
        assert ws(8, 8, 8, _units(*bad)) == 0
    assert ws(8, 8, 8, None) == 0


def test_entry_point_argument_errors_do_not_need_a_gpu(hip_lib):
    one, out, big = ctypes.c_void_p(16), ctypes.c_void_p(64), 1 << 40
    unit = _units(1, 1, 5)
    thresholds = (ctypes.c_int64 * 4)(0, 1, 4, 25)

    def call(pred=one, truth=one, x=8, y=8, z=8, all_border=0, units=unit, th=thresholds, n_th=4, o=out, ws=one,
             ws_bytes=big):
        return hip_lib.gts_surface_stats_i16(pred, truth, x, y, z, all_border, units, th, n_th, o, ws, ws_bytes, None)

    assert call(pred=None) == -1 and call(truth=None) == -1 and call(o=None) == -1 and call(ws=None) == -1
    assert call(units=None) == -1 and call(th=None) == -1
    for extents in ((0, 8, 8), (8, -1, 8), (8, 8, 0), (1, 1, 4098), (2048, 2048, 600)):
        assert call(x=extents[0], y=extents[1], z=extents[2]) == -2
    assert call(x=1, y=1, z=4097, units=_units(1, 1, 99971)) == -2          # the range guard
    need = hip_lib.gts_surface_workspace(240, 240, 155, unit)
    assert call(x=240, y=240, z=155, ws_bytes=need - 1) == -2
    assert call(n_th=5) == -3 and call(n_th=-1) == -3
    assert call(all_border=2) == -3
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, 1000001)):
        assert call(units=_units(*bad)) == -3
    assert call(th=(ctypes.c_int64 * 4)(0, 1, -4, 25)) == -3                # a negative squared tolerance


def test_wrappers_refuse_on_the_host():
    import torch

    from gts import GtsError
    from gts.metrics import hd95s_mm, surface_dices

    vol = torch.zeros((4, 5, 6), dtype=torch.int16)
    with pytest.raises(GtsError, match="MI355X only"):
        hd95s_mm(vol, vol, (1, 1, 1))
    with pytest.raises(GtsError, match=r"\[X, Y, Z\]"):
        hd95s_mm(vol[0], vol[0], (1, 1, 1))
    with pytest.raises(GtsError, match="spacing"):
        surface_dices(vol, vol, (1, 0, 1), (1.0,))
    with pytest.raises(GtsError, match="tolerances"):
        surface_dices(vol, vol, (1, 1, 1), (1, 2, 3, 4, 5))


def test_score_predictions_flags():
    from scripts import score_predictions as cli

    base = ["-s", "preds", "-o", "out.csv"]
    args = cli.build_parser().parse_args(base)
    assert args.mm is False and args.nsd_tolerance == []
    assert cli.header_for(args.nsd_tolerance) == cli.HEADER
    assert cli.HEADER == ["id"] + [f"{r}_{f}" for r in ("WT", "CT", "ET")
                                   for f in ("dice", "hd95", "lw_dice", "lw_hd95", "n_scored", "n_fp", "n_fn")]
    assert cli.build_parser().parse_args(base + ["--mm"]).mm is True
    args = cli.build_parser().parse_args(base + ["--nsd_tolerance", "1", "2.5"])
    assert args.nsd_tolerance == [1.0, 2.5]
    header = cli.header_for(args.nsd_tolerance)
    assert header[:len(cli.HEADER)] == cli.HEADER
    assert header[len(cli.HEADER):] == ["WT_nsd@1", "WT_lw_nsd@1", "CT_nsd@1", "CT_lw_nsd@1", "ET_nsd@1", "ET_lw_nsd@1",
                                        "WT_nsd@2.5", "WT_lw_nsd@2.5", "CT_nsd@2.5", "CT_lw_nsd@2.5", "ET_nsd@2.5",
                                        "ET_lw_nsd@2.5"]
    with pytest.raises(SystemExit):
        cli.main(base + ["--nsd_tolerance", "1", "2", "3", "4", "5"])
