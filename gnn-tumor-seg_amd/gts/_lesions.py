"""What the per-lesion features share (gts.lesionwise, gts.measure, gts.mesh; the device half is csrc/gts_lesions.h):
the argument checks, the region mask, the front end from (labels, region, spacing, connectivity) to the roots every
table pass starts from, and the copy of a table's head to the host.  A new per-lesion feature builds a RegionLesions
and runs its own stages on it.  `what` is the caller's public name and leads every message."""
import ctypes

import numpy as np
import torch

from . import _lib, _volume, components, metrics
from ._lib import check, current_stream, ptr

REGIONS = ("WT", "CT", "ET")
FIRST_COPY_BYTES = 1 << 16   # the table of a real prediction fits here; a longer one takes a second copy


def region_index(region, what):
    if region in REGIONS:
        return REGIONS.index(region)
    if isinstance(region, int) and not isinstance(region, bool) and 0 <= region < 3:
        return region
    raise _lib.GtsError(f"{what}: region {region!r} (one of {REGIONS} or 0..2)")


def connectivity_arg(connectivity, what):
    if isinstance(connectivity, bool) or connectivity not in (6, 26):
        raise _lib.GtsError(f"{what}: connectivity {connectivity!r} (6 or 26)")
    return int(connectivity)


def grid_arg(grid_blocks, what):
    if isinstance(grid_blocks, bool) or not isinstance(grid_blocks, int) or not 0 <= grid_blocks < 2 ** 31:
        raise _lib.GtsError(f"{what}: grid_blocks {grid_blocks!r} (0 for the library's choice, or 1 .. 2^31 - 1)")
    return grid_blocks


def region_mask(lib, labels, region, dilation, workspace, size):
    """L1: the region's mask of a checked label volume, dilated `dilation` times, as int16 0 / 1."""
    x, y, z = labels.shape
    out = torch.empty_like(labels)
    check(lib.gts_lesionwise_dilate_i16(ptr(labels), x, y, z, region, dilation, ptr(out), ptr(workspace), size,
                                        current_stream()), "gts_lesionwise_dilate_i16")
    return out


class RegionLesions:
    """The lesions of one (labels, region, spacing, connectivity) before any table: the checked arguments and `roots`,
    C1-C3 over the region's mask.  limits: the caller's limits in words, for its refusal.  mark: called with a
    stage's name once the stage is enqueued, here "region mask" and "components"; the caller's stages go on with it."""

    def __init__(self, labels, region, spacing_mm, connectivity, what, limits, mark=None):
        self.mark = mark or (lambda stage: None)
        self.region, self.connectivity = region_index(region, what), connectivity_arg(connectivity, what)
        self.units, self.scale_mm = metrics.spacing_units(spacing_mm)
        self.labels = labels = _volume.label_volume(labels, what, three_d=True)
        self.lib = lib = _lib.load()
        self.shape = x, y, z = tuple(labels.shape)
        self.c_units = (ctypes.c_int64 * 3)(*self.units)
        if lib.gts_measure_check(x, y, z, self.c_units) != 0:
            raise _lib.GtsError(f"{what}: volume {x}x{y}x{z} at units {self.units} is outside the kernels' limits "
                                f"({limits})")
        scratch, size = _volume.workspace(lib.gts_lesionwise_workspace, x, y, z, labels.device, what)
        mask = region_mask(lib, labels, self.region, 0, scratch, size)
        self.mark("region mask")
        self.roots = components.roots_unchecked(mask, self.shape, self.connectivity, what)
        self.mark("components")


def table_head(table, total_of):
    """The words of a device table that are in use, on the host: the first FIRST_COPY_BYTES, then the remainder when
    total_of(head), the words in use by the head's counts, says there are more."""
    head = table[:min(table.numel(), FIRST_COPY_BYTES // table.element_size())].cpu().numpy()
    total = total_of(head)
    if total > head.size:
        head = np.concatenate([head, table[head.size:total].cpu().numpy()])
    return head[:total]
