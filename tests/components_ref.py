"""Host reference of gts.components: scipy.ndimage.label and a restatement of the two filter rules."""
import numpy as np
from scipy import ndimage


def _structure(connectivity):
    return ndimage.generate_binary_structure(3, {6: 1, 26: 3}[connectivity])


def lift(labels):
    """The volume as 3-D: unit axes dropped, the rest right-aligned (gts.components.lift_shape)."""
    labels = np.asarray(labels)
    long_axes = [s for s in labels.shape if s != 1]
    assert len(long_axes) <= 3
    return labels.reshape([1] * (3 - len(long_axes)) + long_axes)


def ref_labels(labels, connectivity):
    """(scipy's component numbers 1..k in raster order of first voxel, k), in labels' own shape."""
    lab, k = ndimage.label(lift(labels) != 0, _structure(connectivity))
    return lab.reshape(np.shape(labels)), k


def ref_roots(labels, connectivity):
    """int32: 1 + the smallest C-order linear index of the voxel's component, 0 for background."""
    lab, k = ref_labels(labels, connectivity)
    flat = lab.ravel()
    first = np.full(k + 1, -1, dtype=np.int64)
    idx = np.flatnonzero(flat)
    first[flat[idx][::-1]] = idx[::-1]                    # the smallest index of each number is written last
    return (first[flat] + 1).astype(np.int32).reshape(lab.shape)


def ref_filter(labels, min_voxels, connectivity, et_label=None, et_min_voxels=0, et_replacement=None):
    """(filtered labels, [components found, components removed, voxels removed, ET voxels relabelled])."""
    labels = np.asarray(labels)
    lab, k = ref_labels(labels, connectivity)
    sizes = np.bincount(lab.ravel(), minlength=k + 1)
    small = sizes < min_voxels
    small[0] = False
    out = np.where(small[lab], 0, labels).astype(labels.dtype)               # rule (a)
    relabelled = 0
    if et_label is not None and et_min_voxels > 0:
        et = (out == et_label) & (out != 0)
        if 0 < et.sum() < et_min_voxels:                                     # rule (b)
            out[et] = et_replacement
            relabelled = int(et.sum())
    return out, [k, int(small.sum()), int(sizes[small].sum()), relabelled]


def check_roots(roots, labels, connectivity):
    """The device roots against scipy, exactly: background 0, root - 1 the smallest linear index of its
    component, and the ranks of the roots equal to scipy's numbering voxel for voxel."""
    roots, labels = np.asarray(roots), np.asarray(labels)
    assert roots.dtype == np.int32 and roots.shape == labels.shape
    lab, k = ref_labels(labels, connectivity)
    assert np.array_equal(roots == 0, labels == 0)
    values, ranks = np.unique(roots[roots > 0], return_inverse=True)
    assert len(values) == k
    assert np.array_equal(ranks.ravel() + 1, lab[roots > 0])
    assert np.array_equal(roots, ref_roots(labels, connectivity))
    return k
