"""What the wrappers of the volume kernels (the includers of csrc/gts_volume.h and gts_scan.h) share: the shape
rule, the checks on an int16 label or mask tensor and on a scan (intensity) volume, the NIfTI dtype codes, the
float32 output of a resampling call and the workspace of an entry point.  `what` is the caller's public name and
leads every message."""
import torch

from . import _lib
from ._lib import require_device
from ._operands import expect, f32, scratch

I16, F32 = 4, 16                                        # NIfTI datatype codes, csrc/gts_scan.h's kI16 and kF32
SCAN_CODES = {torch.int16: I16, torch.float32: F32}     # what a scan volume may hold


def lift_shape(shape, what):
    """(X, Y, Z, all_border) of an array shape: the axes of extent 1 dropped, the rest right-aligned in 3-D.
    A unit axis has no neighbours along it, so components are the same; it makes scipy's erosion (border_value
    0, cross footprint of the full rank) remove every voxel, so every region voxel is then border (all_border).
    More than three axes longer than 1: GtsError."""
    shape = tuple(int(s) for s in shape) or (1,)
    long_axes = [s for s in shape if s != 1]
    if len(long_axes) > 3:
        raise _lib.GtsError(f"{what}: {len(long_axes)} axes longer than 1 in {shape} (at most 3)")
    x, y, z = [1] * (3 - len(long_axes)) + long_axes
    return x, y, z, any(s == 1 for s in shape)


def label_volume(t, what, three_d=False, noun="labels"):
    """t, contiguous, after the checks every kernel needs: an int16 CUDA tensor with at least one element
    ([X, Y, Z] where three_d).  noun: what the message calls the values ("masks" for a 0/1 volume)."""
    if not isinstance(t, torch.Tensor):
        raise _lib.GtsError(f"{what} takes a torch tensor")
    if t.dtype != torch.int16:
        raise _lib.GtsError(f"{what} takes int16 {noun}")
    if three_d and t.dim() != 3:
        raise _lib.GtsError(f"{what} takes [X, Y, Z] volumes of three axes, got shape {tuple(t.shape)}")
    if t.numel() == 0:
        raise _lib.GtsError(f"{what}: empty volume")
    if not t.is_cuda:
        require_device(t)          # raises: there is no CPU route
    return t.contiguous()


def label_pair(pred, truth, what, three_d=False):
    """label_volume of both, of one shape and on one device."""
    pred, truth = label_volume(pred, what, three_d), label_volume(truth, what, three_d)
    if pred.shape != truth.shape:
        raise _lib.GtsError(f"{what}: shapes {tuple(pred.shape)} and {tuple(truth.shape)} differ")
    require_device(pred, truth)
    return pred, truth


def scan_volume(t, what):
    """(dtype code, d0, d1, d2) of a scan volume after the checks every kernel needs: a non-empty int16 or
    float32 CUDA tensor of three axes, the last one contiguous."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.numel() == 0:
        raise _lib.GtsError(f"{what} takes a non-empty [Z, Y, X] tensor")
    if t.dtype not in SCAN_CODES:
        raise _lib.GtsError(f"{what}: dtype {t.dtype} is not supported (int16 or float32)")
    require_device(t)
    return (SCAN_CODES[t.dtype],) + tuple(int(n) for n in t.shape)


def float32_out(out, shape, like):
    """The float32 tensor of `shape` a call writes: `out` when given (float32, that shape, on like's device: a
    channel slice of a scan), else a new one beside `like`."""
    if out is None:
        return torch.empty(tuple(shape), dtype=torch.float32, device=like.device)
    f32(out)
    expect(out, shape, "out")
    require_device(like, out)
    return out


def workspace(size_fn, x, y, z, device, what, limits=None):
    """(uint8 tensor, its size) for a volume, size_fn being the library's gts_*_workspace(X, Y, Z); a size of
    0 or an error code is the library's refusal.  limits: the family's limits in words, for the message."""
    size = int(size_fn(x, y, z))
    if size <= 0:
        raise _lib.GtsError(f"{what}: volume {x}x{y}x{z} is outside the kernels' limits" +
                            (f" ({limits})" if limits else ""))
    return scratch(size, device, torch.uint8), size
