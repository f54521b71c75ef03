"""numpy restatement of gts.conform (F1): what the plan and the kernel must give, written straight from the
formulas and independent of the package's tables.

Arrays are [X, Y, Z] or [C, X, Y, Z] (the channel axis in front), as a NIfTI file's voxels index.  An
orientation is (perm, signs, spacing): input axis j runs along world axis perm[j] in direction signs[j] at
spacing[j] mm.  The pipeline's frame has its axes along world x, y, z with signs (-, -, +): L, P, S.
"""
import itertools

import numpy as np

TARGET_SIGNS = (-1, -1, 1)
ORIENTATIONS = tuple((p, s) for p in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3))


def make_affine(perm, signs, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    a = np.eye(4)
    a[:3, :3] = 0.0
    for j in range(3):
        a[perm[j], j] = signs[j] * spacing[j]
    a[:3, 3] = origin
    return a


def flips_of(perm, signs):
    return tuple(signs[j] != TARGET_SIGNS[perm[j]] for j in range(3))


def source_of(perm):
    return tuple(perm.index(w) for w in range(3))


def reorient(a, perm, signs):
    """The array in the pipeline's frame, spacing untouched: np.transpose of np.flip."""
    lead = a.ndim - 3
    flipped = [lead + j for j, f in enumerate(flips_of(perm, signs)) if f]
    a = np.flip(a, axis=flipped) if flipped else a
    return np.ascontiguousarray(np.transpose(a, list(range(lead)) + [lead + j for j in source_of(perm)]))


def unreorient(a, perm, signs):
    lead = a.ndim - 3
    a = np.transpose(a, list(range(lead)) + [lead + w for w in perm])
    flipped = [lead + j for j, f in enumerate(flips_of(perm, signs)) if f]
    return np.ascontiguousarray(np.flip(a, axis=flipped) if flipped else a)


def axis_samples(n, s, reverse):
    """(i0, i1, t) for every output index of an axis of length n at spacing s, by the issue's formulas."""
    n_out = int(np.floor((n - 1) * np.float64(s))) + 1
    i0, i1, t = [], [], []
    for i in range(n_out):
        u = np.float64(i) / np.float64(s)
        r0 = min(int(np.floor(u)), n - 1)
        r1 = min(r0 + 1, n - 1)
        t.append(u - r0)
        i0.append(n - 1 - r0 if reverse else r0)
        i1.append(n - 1 - r1 if reverse else r1)
    return np.array(i0), np.array(i1), np.array(t, dtype=np.float64)


def _per_input_axis(shape, perm, signs, spacing):
    """For input axis j: (i0, i1, t) over conformed axis perm[j], each reshaped to broadcast along it."""
    flips = flips_of(perm, signs)
    out = []
    for j in range(3):
        i0, i1, t = axis_samples(shape[j], spacing[j], flips[j])
        view = [1, 1, 1]
        view[perm[j]] = len(i0)
        out.append((i0.reshape(view), i1.reshape(view), t.reshape(view)))
    return out


def conform_trilinear(a, perm, signs, spacing):
    """(float64 result, largest neighbour magnitude per voxel): lerp along input x, then y, then z, a + (b - a) t."""
    if a.ndim == 4:
        parts = [conform_trilinear(c, perm, signs, spacing) for c in a]
        return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    (x0, x1, tx), (y0, y1, ty), (z0, z1, tz) = _per_input_axis(a.shape, perm, signs, spacing)
    v = a.astype(np.float64)
    corner = {(i, j, k): v[(x0, x1)[i], (y0, y1)[j], (z0, z1)[k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)}
    vmax = np.max(np.stack([np.abs(c) for c in corner.values()]), axis=0)
    along_x = {(j, k): corner[0, j, k] + (corner[1, j, k] - corner[0, j, k]) * tx for j in (0, 1) for k in (0, 1)}
    along_y = {k: along_x[0, k] + (along_x[1, k] - along_x[0, k]) * ty for k in (0, 1)}
    return along_y[0] + (along_y[1] - along_y[0]) * tz, vmax


def conform_nearest(a, perm, signs, spacing):
    """t < 0.5 takes the first index, anything else (a tie included) the second."""
    if a.ndim == 4:
        return np.stack([conform_nearest(c, perm, signs, spacing) for c in a])
    pick = [np.where(t < 0.5, i0, i1) for i0, i1, t in _per_input_axis(a.shape, perm, signs, spacing)]
    return np.ascontiguousarray(a[pick[0], pick[1], pick[2]])


def conformed_shape(shape, perm, spacing):
    src = source_of(perm)
    return tuple(int(np.floor((shape[j] - 1) * np.float64(spacing[j]))) + 1 for j in src)


def unconform_nearest(c, shape, perm, signs, spacing):
    """Conformed labels c back onto the scan's grid of `shape`: input index a reads conformed index
    min(floor(r s + 0.5), n_out - 1), r = a or n - 1 - a when the axis is reversed."""
    if c.ndim == 4:
        return np.stack([unconform_nearest(ch, shape, perm, signs, spacing) for ch in c])
    flips = flips_of(perm, signs)
    idx = []
    for j in range(3):
        n, n_out = shape[j], c.shape[perm[j]]
        r = np.arange(n, dtype=np.float64)
        if flips[j]:
            r = n - 1 - r
        view = [1, 1, 1]
        view[j] = n
        idx.append(np.minimum(np.floor(r * np.float64(spacing[j]) + 0.5), n_out - 1).astype(np.int64).reshape(view))
    by_world = [idx[source_of(perm)[w]] for w in range(3)]
    return np.ascontiguousarray(c[by_world[0], by_world[1], by_world[2]])


def ulp32(x):
    """The float32 unit in the last place at the magnitude of float64 x (2^-149 at and below the subnormals)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))
