"""BraTS HD95 on the device (H1-H5, csrc/gts_hd95.hip).

hd95s(pred, truth) returns what model.evaluation.calculate_hd95s returns for the same volumes, to the bit:
the kernels produce the integer order statistics of the squared border distances, and the host finishes
np.percentile's linear interpolation from their square roots in float64.
"""
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
    v = (n - 1) * 0.95
    if v >= n - 1:
        return math.sqrt(float(d2_hi))
    g = v - math.floor(v)
    a, b = math.sqrt(float(d2_lo)), math.sqrt(float(d2_hi))
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
