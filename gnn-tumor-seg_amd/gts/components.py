"""3-D connected components on the device and the small-island clean-up built on them (C1-C5,
csrc/gts_components.hip).

component_roots(labels) gives every foreground voxel (label != 0) 1 + the smallest linear index of its
component; remove_small_components(labels, min_voxels) drops the components below a voxel count and can
relabel an implausibly small enhancing-tumour total.  Both equal what scipy.ndimage.label + np.bincount
give on the host, voxel for voxel, and run on the current stream.
"""
import torch

from . import _lesions, _lib, _volume   # _lesions imports this module in turn; both use the other at call time only
from ._lib import check, current_stream, ptr, require_device


def lift_shape(shape):
    """(X, Y, Z) of an array shape: gts._volume.lift_shape without the border flag."""
    return _volume.lift_shape(shape, "components")[:3]


def _prepare(labels, connectivity, what):
    _lesions.connectivity_arg(connectivity, what)
    labels = _volume.label_volume(labels, what)
    return labels, lift_shape(labels.shape)


def roots_unchecked(labels, extents, connectivity, what):
    """C1-C3 of a volume label_volume has passed, with (X, Y, Z) = extents."""
    lib = _lib.load()
    x, y, z = extents
    workspace, size = _volume.workspace(lib.gts_components_workspace, x, y, z, labels.device, what)
    roots = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    check(lib.gts_components_roots_i16(ptr(labels), x, y, z, connectivity, ptr(roots), ptr(workspace), size,
                                       current_stream()), "gts_components_roots_i16")
    return roots


def component_roots(labels, connectivity=26):
    """int32 tensor of labels' shape: 1 + the smallest C-order linear index of the voxel's component of
    labels != 0, 0 for background.  labels: int16 CUDA tensor, at most three axes longer than 1."""
    labels, extents = _prepare(labels, connectivity, "component_roots")
    return roots_unchecked(labels, extents, connectivity, "component_roots")


def remove_small_components(labels, min_voxels, connectivity=26, *, et_label=None, et_min_voxels=0,
                            et_replacement=None, out=None):
    """(labels_out, stats).  labels_out: labels with (a) every component of labels != 0 that has fewer than
    min_voxels voxels set to 0, then (b) when et_min_voxels > 0 and fewer than that many (but some) voxels equal
    to et_label remain, each of them set to et_replacement.  stats: device int64 [4] = components found,
    components removed, voxels removed, ET voxels relabelled.  `out` may be labels itself (in place)."""
    src, (x, y, z) = _prepare(labels, connectivity, "remove_small_components")
    lib = _lib.load()
    workspace, size = _volume.workspace(lib.gts_components_workspace, x, y, z, src.device, "remove_small_components")
    et_min_voxels = int(et_min_voxels)
    if et_min_voxels > 0 and (et_label is None or et_replacement is None):
        raise _lib.GtsError("remove_small_components: et_min_voxels needs et_label and et_replacement")
    if et_label is None or et_replacement is None:
        et_label, et_replacement, et_min_voxels = 0, 0, 0
    for value in (et_label, et_replacement):
        if not -32768 <= int(value) <= 32767:
            raise _lib.GtsError(f"remove_small_components: label {value} is not an int16")
    if out is None:
        out = torch.empty_like(src)
    elif out.dtype != torch.int16 or out.shape != labels.shape or not out.is_cuda or not out.is_contiguous():
        raise _lib.GtsError("remove_small_components: out must be a contiguous int16 CUDA tensor of labels' shape")
    require_device(src, out)
    stats = torch.empty(4, dtype=torch.int64, device=src.device)
    check(lib.gts_components_filter_i16(ptr(src), x, y, z, connectivity, int(min_voxels), int(et_label), et_min_voxels,
                                        int(et_replacement), ptr(out), ptr(stats), ptr(workspace), size,
                                        current_stream()), "gts_components_filter_i16")
    return out, stats
