"""numpy restatement of the co-registration definitions (R1, R2, the mutual information and the compass search of
DESIGN.md 4v), written from the definitions and independent of gts.register.

Arrays are [X, Y, Z], as a NIfTI file's voxels index (the device holds them [Z, Y, X]).  A transform is a 3 x 4
float64 matrix T that takes an output (or fixed) voxel index (x, y, z) to index coordinates of the moving volume.
Every product and sum is one float64 numpy operation in the order the definition writes it.
"""
import numpy as np

MIN_STEP = 0.0625


def _coordinates(T, shape, stride=1):
    T = np.asarray(T, dtype=np.float64).reshape(3, 4)
    x, y, z = np.meshgrid(*[np.arange(0, n, stride, dtype=np.float64) for n in shape], indexing="ij")
    return [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]


def _lerp(a, b, t):
    return np.where(t == 0.0, a, a + (b - a) * t)


def sample(vol, T, shape, stride=1):
    """(inside [..] bool, value [..] float64, 0 where outside) at the points T sends the strided indices of a grid of
    `shape` to."""
    u, v, w = _coordinates(T, shape, stride)
    X, Y, Z = vol.shape
    with np.errstate(invalid="ignore"):
        inside = (u >= 0) & (u <= X - 1) & (v >= 0) & (v <= Y - 1) & (w >= 0) & (w <= Z - 1)
    u, v, w = (np.where(inside, c, 0.0) for c in (u, v, w))
    idx = []
    for c, n in ((u, X), (v, Y), (w, Z)):
        i0 = np.minimum(np.floor(c), n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        idx.append((i0.astype(np.int64), i1.astype(np.int64), c - i0))
    (x0, x1, tx), (y0, y1, ty), (z0, z1, tz) = idx
    f = vol.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        along_x = {(j, k): _lerp(f[x0, (y0, y1)[j], (z0, z1)[k]], f[x1, (y0, y1)[j], (z0, z1)[k]], tx)
                   for j in (0, 1) for k in (0, 1)}
        along_y = {k: _lerp(along_x[0, k], along_x[1, k], ty) for k in (0, 1)}
        value = _lerp(along_y[0], along_y[1], tz)
    return inside, np.where(inside, value, 0.0)


def affine_resample(vol, T, out_shape):
    """R1: float32 [OX, OY, OZ]."""
    _, value = sample(vol, T, out_shape)
    with np.errstate(over="ignore"):
        return value.astype(np.float32)


def bin_of(v, lo, scale, bins):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((v - np.float64(lo)) * np.float64(scale))
        b = np.where(q >= 1.0, np.where(q < bins - 1, q, bins - 1), 0.0)
    b = np.where(np.isfinite(v), b, 0.0)
    return b.astype(np.int64)


def joint_histogram(fixed, moving, matrices, stride, bins, ranges):
    """R2: int64 [K, bins^2 + 1]."""
    lo_f, scale_f, lo_m, scale_m = ranges
    matrices = np.asarray(matrices, dtype=np.float64).reshape(-1, 3, 4)
    bf = bin_of(fixed[::stride, ::stride, ::stride], lo_f, scale_f, bins)
    out = np.zeros((len(matrices), bins * bins + 1), dtype=np.int64)
    for k, T in enumerate(matrices):
        inside, m = sample(moving, T, fixed.shape, stride)
        cell = np.where(inside, bf * bins + bin_of(m, lo_m, scale_m, bins), bins * bins)
        out[k] = np.bincount(cell.ravel(), minlength=bins * bins + 1)
    return out


def strided_samples(shape, stride):
    return int(np.prod([(n + stride - 1) // stride for n in shape]))


def bin_ranges(fixed, moving, bins):
    out = []
    for v in (fixed, moving):
        v = np.asarray(v)
        finite = v[np.isfinite(v)] if v.dtype.kind == "f" else v.ravel()
        lo, hi = float(finite.min()), float(finite.max())
        out += [lo, float(bins) / (hi - lo) if hi > lo else 0.0]
    return tuple(out)


def mutual_information(counts):
    counts = np.asarray(counts, dtype=np.int64)
    bins = int(round(np.sqrt(counts.size - 1)))
    table = counts[:-1].reshape(bins, bins)
    n = int(table.sum())
    if n == 0:
        return 0.0
    row, col = table.sum(axis=1), table.sum(axis=0)
    total = 0.0
    for i in range(bins):
        filled = np.flatnonzero(table[i])
        if filled.size == 0:
            continue
        p = table[i, filled] / np.float64(n)
        terms = p * np.log(p / ((row[i] / np.float64(n)) * (col[filled] / np.float64(n))))
        for t in terms.tolist():
            total += t
    return total


def search(fixed, moving, base_transform, levels, bins, max_rotate=15.0):
    """The compass search on the host: (params float64 [6], score, launches, outside fraction)."""
    ranges = bin_ranges(fixed, moving, bins)
    launches = 0

    def score_many(param_list, stride):
        nonlocal launches
        launches += 1
        counts = joint_histogram(fixed, moving, [base_transform(q) for q in param_list], stride, bins, ranges)
        return [mutual_information(c) for c in counts], [c[-1] / np.float64(max(int(c.sum()), 1)) for c in counts]

    p = np.zeros(6)
    current = outside = 0.0
    for stride in levels:
        (current,), (outside,) = score_many([p], stride)
        step = float(stride)
        while step >= MIN_STEP:
            probes = []
            for k in range(6):
                for sign in (1.0, -1.0):
                    q = p.copy()
                    q[k] = q[k] + sign * step
                    if k >= 3:
                        q[k] = min(max(q[k], -max_rotate), max_rotate)
                    probes.append(q)
            scores, outsides = score_many(probes, stride)
            best = 0
            for k in range(1, 12):                   # the first maximum
                if scores[k] > scores[best]:
                    best = k
            if scores[best] > current:
                p, current, outside = probes[best], scores[best], outsides[best]
            else:
                step *= 0.5
    return p, float(current), launches, float(outside)
