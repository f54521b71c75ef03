"""BraTS HD95 on the device (H1-H5, csrc/gts_hd95.hip).

hd95s(pred, truth) returns what model.evaluation.calculate_hd95s returns for the same volumes, to the bit:
the kernels produce the integer order statistics of the squared border distances, and the host finishes
np.percentile's linear interpolation from their square roots in float64.

Under a voxel spacing (H3w-H5w) the same borders are measured in millimetres: hd95s_mm and
surface_dices.  The spacing is taken in integer units of 1e-4 mm (spacing_units), a deviation of at most
5e-5 mm per axis from a header's float spacing; on those units the device arithmetic is exact integers, and
the results equal scipy's distance_transform_edt(sampling=units) route to the bit.
"""
import ctypes
import math

import torch

from . import _lib, _volume
from ._lib import check, current_stream, ptr

ABSENT_FROM_ONE = 300     # calculate_hd95_from_logical_array: the region is missing from one side only
ABSENT_FROM_BOTH = 0


def percentile95_from_order_stats(n, d2_lo, d2_hi):
    """np.percentile(sqrt(d2), 95) (linear method) of n sorted squared distances, from the two order
    statistics it interpolates between: d2_lo at rank floor((n - 1) * 0.95) and d2_hi at the next rank
    (both the last one when (n - 1) * 0.95 >= n - 1).  Same float64 operations as numpy's _lerp."""
    n = int(n)
    if n < 1:
        raise ValueError("percentile of an empty multiset")
    return _lerp95(n, math.sqrt(float(d2_lo)), math.sqrt(float(d2_hi)))


def _lerp95(n, a, b):
    """numpy's _lerp between the values a and b at the two ranks of the 95th percentile of n values."""
    v = (n - 1) * 0.95
    if v >= n - 1:
        return b
    g = v - math.floor(v)
    d = b - a
    return b - d * (1 - g) if g >= 0.5 else a + d * g


def lift_shape(shape):
    """(X, Y, Z, all_border) of an array shape: gts._volume.lift_shape."""
    return _volume.lift_shape(shape, "hd95s")


def hd95_order_stats(pred, truth):
    """Device int64 [3, 4]: per region (WT, CT, ET) the border count n, the squared distances at the two
    ranks np.percentile(., 95) interpolates between, and the presence bits (1 pred, 2 truth) — see
    gts_hd95_order_stats_i16 in include/gts_hip.h.  pred / truth: int16 CUDA tensors of one shape with at
    most three axes longer than 1, at least one element."""
    pred, truth = _volume.label_pair(pred, truth, "hd95s")
    x, y, z, all_border = lift_shape(pred.shape)
    lib = _lib.load()
    workspace, size = _volume.workspace(lib.gts_hd95_workspace, x, y, z, pred.device, "hd95s")
    out = torch.empty((3, 4), dtype=torch.int64, device=pred.device)
    check(lib.gts_hd95_order_stats_i16(ptr(pred), ptr(truth), x, y, z, int(all_border), ptr(out), ptr(workspace),
                                       size, current_stream()), "gts_hd95_order_stats_i16")
    return out


def hd95s(pred, truth):
    """[WT, CT, ET] HD95 of two int16 label tensors of one shape on the GPU, as Python floats: 0 for a
    region absent from both, 300 for one absent from one side.  One small device-to-host copy."""
    if pred.numel() == 0 and pred.shape == truth.shape:
        return [float(ABSENT_FROM_BOTH)] * 3       # scipy finds no object on either side
    result = []
    for n, d2_lo, d2_hi, present in hd95_order_stats(pred, truth).cpu().tolist():
        if present == 3:
            result.append(percentile95_from_order_stats(n, d2_lo, d2_hi))
        else:
            result.append(float(ABSENT_FROM_BOTH if present == 0 else ABSENT_FROM_ONE))
    return result


# ---------------------------------------------------------------- in millimetres: HD95 and surface Dice
UNITS_PER_MM = 10000          # a spacing is taken in steps of 1e-4 mm
MAX_SPACING_MM = 100
MAX_TOLERANCES = 4
STATS_INTS = 4 + 2 * MAX_TOLERANCES     # one region's row of gts_surface_stats_i16's table
_MAX_THRESHOLD = 1 << 62                # above every D2 the kernels accept (B < 2^62)


def _steps(value_mm, what):
    """value_mm in integer steps of 1e-4 mm (round half to even)."""
    value = float(value_mm)
    if not math.isfinite(value):
        raise _lib.GtsError(f"{what}: {value_mm!r} is not finite")
    return int(round(value * UNITS_PER_MM))


def _spacing_steps(spacing_mm):
    spacing = tuple(spacing_mm)
    if len(spacing) != 3:
        raise _lib.GtsError(f"spacing {spacing!r}: three values (x, y, z) in mm")
    steps = tuple(_steps(s, "spacing") for s in spacing)
    if any(u < 1 or u > MAX_SPACING_MM * UNITS_PER_MM for u in steps):
        raise _lib.GtsError(f"spacing {spacing!r}: every value must round to at least 1e-4 mm and be at most "
                            f"{MAX_SPACING_MM} mm")
    return steps


def _common_divisor(steps):
    """The greatest divisor shared by the three step counts and by 10000 (the steps in a millimetre)."""
    return math.gcd(*steps, UNITS_PER_MM)


def spacing_units(spacing_mm):
    """((ux, uy, uz), scale_mm) of a voxel spacing in mm: the spacing in steps of 1e-4 mm, u_a = round(s_a * 1e4),
    divided by g = gcd(ux, uy, uz, 10000), and scale_mm = g / 10000: a millimetre stays a whole number of
    reduced steps, so scale_mm is 1 / k.  A distance in mm is sqrt(sum_a u_a^2 (p_a - q_a)^2) * scale_mm.
    (1, 1, 1) gives ((1, 1, 1), 1.0), (0.5, 0.5, 0.5) ((1, 1, 1), 0.5), (0.9375, 0.9375, 5) ((15, 15, 80), 0.0625).
    The rounding moves a spacing by at most 5e-5 mm per axis, the deviation from a header's float spacing.  A
    spacing that is not finite, rounds to 0 or exceeds 100 mm: GtsError."""
    steps = _spacing_steps(spacing_mm)
    g = _common_divisor(steps)
    return tuple(u // g for u in steps), g / UNITS_PER_MM


def tolerance_thresholds(tolerances_mm, spacing_mm):
    """[T_k]: for each tolerance (mm, finite, >= 0, at most 4 of them) the largest integer D2 in spacing_units'
    units that lies within it, T_k = floor(t_k^2 / g^2) with t_k = round(tol * 1e4) and g the spacing's common
    divisor, in exact integers: D2 <= T_k is sqrt(D2) * scale_mm <= tolerance without a float in it."""
    tolerances = tuple(tolerances_mm)
    if len(tolerances) > MAX_TOLERANCES:
        raise _lib.GtsError(f"{len(tolerances)} tolerances (at most {MAX_TOLERANCES})")
    g = _common_divisor(_spacing_steps(spacing_mm))
    out = []
    for tol in tolerances:
        t = _steps(tol, "tolerance")
        if t < 0:
            raise _lib.GtsError(f"tolerance {tol!r} mm is negative")
        out.append(min(t * t // (g * g), _MAX_THRESHOLD))
    return out


def surface_stats(pred, truth, spacing_mm=(1, 1, 1), tolerances_mm=()):
    """Device int64 [3, 12]: per region (WT, CT, ET) n, D2 at the two ranks of the 95th percentile and the
    presence bits as hd95_order_stats gives them, D2 in spacing_units' units, then for pred and for truth the
    number of border voxels within each tolerance of the other side's border (4 slots each, unused ones 0) — see
    gts_surface_stats_i16 in include/gts_hip.h.  pred / truth: int16 CUDA volumes [X, Y, Z] of one shape."""
    units, _ = spacing_units(spacing_mm)
    thresholds = tolerance_thresholds(tolerances_mm, spacing_mm)
    pred, truth = _volume.label_pair(pred, truth, "surface_stats", three_d=True)
    x, y, z = pred.shape
    lib = _lib.load()
    c_units = (ctypes.c_int64 * 3)(*units)
    workspace, size = _volume.workspace(lambda *extents: lib.gts_surface_workspace(*extents, c_units), x, y, z,
                                        pred.device, f"surface_stats (units {units})")
    out = torch.empty((3, STATS_INTS), dtype=torch.int64, device=pred.device)
    c_thresholds = (ctypes.c_int64 * len(thresholds))(*thresholds) if thresholds else None
    all_border = int(1 in pred.shape)       # scipy's erosion of an array with a unit axis (lift_shape)
    check(lib.gts_surface_stats_i16(ptr(pred), ptr(truth), x, y, z, all_border, c_units, c_thresholds,
                                    len(thresholds), ptr(out), ptr(workspace), size, current_stream()),
          "gts_surface_stats_i16")
    return out


def hd95_mm_from_row(row, scale_mm):
    """The HD95 in mm of one region's row of surface_stats (a list of ints): the two order statistics are
    scaled to mm first, then interpolated; 0 / 300 for a region absent from both sides / from one."""
    n, d2_lo, d2_hi, present = row[:4]
    if present != 3:
        return float(ABSENT_FROM_BOTH if present == 0 else ABSENT_FROM_ONE)
    return _lerp95(n, math.sqrt(float(d2_lo)) * scale_mm, math.sqrt(float(d2_hi)) * scale_mm)


def surface_dices_from_row(row, n_tolerances):
    """[NSD per tolerance] of one region's row of surface_stats: (within_pred + within_truth) / (n_pred +
    n_truth); 1.0 for a region absent from both sides, 0.0 for one absent from one."""
    n, present = row[0], row[3]
    if present != 3:
        return [1.0 if present == 0 else 0.0] * n_tolerances
    return [(row[4 + k] + row[4 + MAX_TOLERANCES + k]) / n for k in range(n_tolerances)]


def hd95s_mm(pred, truth, spacing_mm):
    """[WT, CT, ET] HD95 in mm of two int16 label volumes [X, Y, Z] with voxel spacing spacing_mm, as Python
    floats: np.percentile(., 95) of the border-to-border distances scipy's distance_transform_edt gives with
    sampling = the spacing in 1e-4 mm steps (spacing_units' deviation).  0 and 300 for absent regions, as
    hd95s.  One small device-to-host copy."""
    _, scale = spacing_units(spacing_mm)
    return [hd95_mm_from_row(row, scale) for row in surface_stats(pred, truth, spacing_mm).cpu().tolist()]


def surface_dices(pred, truth, spacing_mm, tolerances_mm):
    """[[WT, CT, ET] per tolerance]: the normalised surface Dice at each tolerance in mm (at most 4), the
    share of both sides' border voxels (the borders of hd95s) that lie within the tolerance of the other
    side's border.  One small device-to-host copy."""
    tolerances = tuple(tolerances_mm)
    rows = surface_stats(pred, truth, spacing_mm, tolerances).cpu().tolist()
    per_region = [surface_dices_from_row(row, len(tolerances)) for row in rows]
    return [[per_region[r][k] for r in range(3)] for k in range(len(tolerances))]
