"""Host half of the device HD95 (gts.metrics): the percentile finish, the shape rule against scipy's
erosion, and the argument checks of the C entry point, none of which needs a GPU."""
import ctypes

import numpy as np
import pytest
from scipy.ndimage import binary_erosion, generate_binary_structure

from tests.hd95_ref import border_lifted as _border_lifted


def _order_stats(d2):
    from gts.metrics import percentile95_from_order_stats

    s = np.sort(d2)
    n = len(s)
    v = (n - 1) * 0.95
    lo = n - 1 if v >= n - 1 else int(np.floor(v))
    hi = n - 1 if v >= n - 1 else lo + 1
    return percentile95_from_order_stats(n, int(s[lo]), int(s[hi]))


def test_percentile_finish_is_numpys_to_the_bit():
    rng = np.random.default_rng(0)
    for n in range(1, 3001):
        d2 = rng.integers(0, 20000, size=n)
        want = np.percentile(np.sqrt(d2.astype(np.float64)), 95)
        assert _order_stats(d2) == want, n
    for n in rng.integers(3001, 400_000, size=40):
        d2 = rng.integers(0, 140_000, size=int(n))
        assert _order_stats(d2) == np.percentile(np.sqrt(d2.astype(np.float64)), 95), n


def test_percentile_finish_rejects_an_empty_multiset():
    from gts.metrics import percentile95_from_order_stats

    with pytest.raises(ValueError):
        percentile95_from_order_stats(0, 0, 0)


@pytest.mark.parametrize("shape", [(9, 7, 6), (1, 9, 7, 6), (11, 8), (9, 1, 6), (1, 1, 13), (13,), (1, 5, 1, 4)])
def test_shape_rule_gives_scipys_border(shape):
    from gts.metrics import lift_shape

    rng = np.random.default_rng(len(shape) * 100 + sum(shape))
    x, y, z, all_border = lift_shape(shape)
    assert x * y * z == int(np.prod(shape))
    assert all_border == (1 in shape)
    for density in (0.3, 0.7, 1.0):
        result = rng.random(shape) < density
        want = result ^ binary_erosion(result, structure=generate_binary_structure(result.ndim, 1), iterations=1)
        got = _border_lifted(result, x, y, z, all_border)
        assert np.array_equal(got.reshape(shape), want), (shape, density)


def test_shape_rule_refuses_four_long_axes():
    from gts import _lib
    from gts.metrics import lift_shape

    assert lift_shape(()) == (1, 1, 1, True)                     # np.atleast_1d: one voxel on a unit axis
    with pytest.raises(_lib.GtsError):
        lift_shape((2, 3, 4, 5))


def test_entry_point_argument_errors_do_not_need_a_gpu(hip_lib):
    one = ctypes.c_void_p(16)
    out = ctypes.c_void_p(64)
    big = 1 << 40

    def call(pred=one, truth=one, x=8, y=8, z=8, all_border=0, o=out, ws=one, ws_bytes=big):
        return hip_lib.gts_hd95_order_stats_i16(pred, truth, x, y, z, all_border, o, ws, ws_bytes, None)

    assert call(pred=None) == -1 and call(truth=None) == -1 and call(o=None) == -1 and call(ws=None) == -1
    for extents in ((0, 8, 8), (8, -1, 8), (8, 8, 0)):
        assert call(x=extents[0], y=extents[1], z=extents[2]) == -2
        assert hip_lib.gts_hd95_workspace(*extents) == 0
    # (X-1)^2 + (Y-1)^2 + (Z-1)^2 <= 2^24: 4097 along one axis is the longest line
    assert hip_lib.gts_hd95_workspace(1, 1, 4097) > 0 and hip_lib.gts_hd95_workspace(1, 1, 4098) == 0
    assert call(x=1, y=1, z=4098) == -2
    assert call(x=2900, y=2900, z=1) == -2                      # bound above 2^24
    assert hip_lib.gts_hd95_workspace(2048, 2048, 600) == 0     # 2^31 voxels or more
    need = hip_lib.gts_hd95_workspace(240, 240, 155)
    assert need > 240 * 240 * 155 * (1 + 12 + 24)               # bits, uint16 and int32 distances of 6 channels
    assert call(x=240, y=240, z=155, ws_bytes=need - 1) == -2
    assert call(all_border=2) == -3
