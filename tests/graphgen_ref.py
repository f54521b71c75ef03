"""Numpy restatement of skimage <= 0.18 SLIC as DESIGN.md "Graph generation" states it: the
oracle the HIP SLIC (gts.graphgen) must match label for label.  Test-side only.

regular_grid, the SLIC rounds from a given smoothed + scaled volume, and the connectivity
enforcement pass (a direct Python loop in skimage's raster/BFS order).  Also the seeded test
volumes the fixtures are computed on.
"""
import hashlib
from collections import namedtuple

import numpy as np


# regular_grid follows skimage.util.regular_grid (scikit-image, BSD-3-Clause licence,
# Copyright (C) 2019, the scikit-image team; redistribution with this notice is permitted).
def regular_grid(ar_shape, n_points):
    ar_shape = np.asanyarray(ar_shape)
    ndim = len(ar_shape)
    unsort_dim_idxs = np.argsort(np.argsort(ar_shape))
    sorted_dims = np.sort(ar_shape)
    space_size = float(np.prod(ar_shape))
    if space_size <= n_points:
        return (slice(None),) * ndim
    stepsizes = (space_size / n_points) ** (1.0 / ndim) * np.ones(ndim)
    if (sorted_dims < stepsizes).any():
        for dim in range(ndim):
            stepsizes[dim] = sorted_dims[dim]
            space_size = float(np.prod(sorted_dims[dim + 1:]))
            stepsizes[dim + 1:] = ((space_size / n_points) ** (1.0 / (ndim - dim - 1)))
            if (sorted_dims >= stepsizes).all():
                break
    starts = (stepsizes // 2).astype(int)
    stepsizes = np.round(stepsizes).astype(int)
    slices = [slice(start, None, step) for start, step in zip(starts, stepsizes)]
    return tuple(slices[i] for i in unsort_dim_idxs)


def _steps(slices):
    return [int(s.step if s.step is not None else 1) for s in slices]


def slic_rounds_ref(scaled, n_segments, max_iter=10, emptied=None):
    """Labels (int64, before connectivity) of max_iter SLIC rounds over `scaled` [D,H,W,C].
    `emptied`, a list, receives the number of emptied segments (NaN centres) after each update."""
    if scaled.ndim == 3:
        scaled = scaled[..., None]
    d, h, w, c = scaled.shape
    slices = regular_grid((d, h, w), n_segments)
    steps = _steps(slices)
    zz, yy, xx = np.mgrid[:d, :h, :w]
    coords = np.stack([zz[slices].ravel(), yy[slices].ravel(), xx[slices].ravel()], axis=1).astype(np.float64)
    n_c = coords.shape[0]
    seg = np.zeros((n_c, 3 + c))
    seg[:, :3] = coords
    sw = 1.0 / (float(max(steps)) ** 2)
    wz, wy, wx = _steps(regular_grid((d, h, w), n_c))
    labels = np.full((d, h, w), -1, dtype=np.int64)
    for it in range(max_iter):
        dist_img = np.full((d, h, w), np.finfo(np.float64).max)
        for k in range(n_c):
            cz, cy, cx = seg[k, :3]
            if np.isnan(cz):
                continue
            z0, z1 = int(max(cz - 2 * wz, 0)), int(min(cz + 2 * wz + 1, d))
            y0, y1 = int(max(cy - 2 * wy, 0)), int(min(cy + 2 * wy + 1, h))
            x0, x1 = int(max(cx - 2 * wx, 0)), int(min(cx + 2 * wx + 1, w))
            if z1 <= z0 or y1 <= y0 or x1 <= x0:
                continue
            dz = ((cz - np.arange(z0, z1)) ** 2)[:, None, None]
            dy = ((cy - np.arange(y0, y1)) ** 2)[None, :, None]
            dx = ((cx - np.arange(x0, x1)) ** 2)[None, None, :]
            dist = ((dz + dy) + dx) * sw
            win = scaled[z0:z1, y0:y1, x0:x1]
            col = np.zeros(dist.shape)
            for ch in range(c):
                col = col + (win[..., ch] - seg[k, 3 + ch]) ** 2
            dist = dist + col
            sub = dist_img[z0:z1, y0:y1, x0:x1]
            better = dist < sub
            sub[better] = dist[better]
            labels[z0:z1, y0:y1, x0:x1][better] = k
        if it == 0:
            assert (labels >= 0).all(), "a voxel lies in no window in the first round"
        if it == max_iter - 1:
            break
        lab = labels.ravel()
        counts = np.bincount(lab, minlength=n_c).astype(np.float64)
        sums = [np.bincount(lab, weights=a.ravel().astype(np.float64), minlength=n_c) for a in (zz, yy, xx)]
        sums += [np.bincount(lab, weights=scaled[..., ch].ravel(), minlength=n_c) for ch in range(c)]
        with np.errstate(invalid="ignore", divide="ignore"):
            seg = np.stack(sums, axis=1) / counts[:, None]
        if emptied is not None:
            emptied.append(int(np.isnan(seg[:, 0]).sum()))
    return labels


def connectivity_ref(segments, min_size, max_size):
    """skimage _enforce_label_connectivity_cython (start_label 0), literally."""
    d, h, w = segments.shape
    ddx = (1, -1, 0, 0, 0, 0)
    ddy = (0, 0, 1, -1, 0, 0)
    ddz = (0, 0, 0, 0, 1, -1)
    seg = segments.tolist()
    out = np.full((d, h, w), -1, dtype=np.int64).tolist()
    coord = [None] * max(max_size, 1)
    current = 0
    for z in range(d):
        for y in range(h):
            for x in range(w):
                if out[z][y][x] >= 0:
                    continue
                adjacent = 0
                label = seg[z][y][x]
                out[z][y][x] = current
                size = 1
                visited = 0
                coord[0] = (z, y, x)
                while visited < size < max_size:
                    cz, cy, cx = coord[visited]
                    for i in range(6):
                        zz, yy, xx = cz + ddz[i], cy + ddy[i], cx + ddx[i]
                        if 0 <= xx < w and 0 <= yy < h and 0 <= zz < d:
                            if seg[zz][yy][xx] == label and out[zz][yy][xx] == -1:
                                out[zz][yy][xx] = current
                                coord[size] = (zz, yy, xx)
                                size += 1
                                if size >= max_size:
                                    break
                            elif out[zz][yy][xx] >= 0 and out[zz][yy][xx] != current:
                                adjacent = out[zz][yy][xx]
                    visited += 1
                if size < min_size:
                    for i in range(size):
                        a, b, cc = coord[i]
                        out[a][b][cc] = adjacent
                else:
                    current += 1
    return np.array(out, dtype=np.int64)


def connectivity_sizes(shape3, n_segments):
    segment_size = float(np.prod(shape3)) / n_segments
    return int(0.5 * segment_size), int(3 * segment_size)


# ---- seeded volumes ------------------------------------------------------------------------------

Case = namedtuple("Case", "name shape channels n_segments compactness seed constant_box")

CASES = (
    Case("c4", (40, 48, 36), 4, 300, 0.5, 11, None),
    Case("c1", (32, 36, 28), 0, 200, 0.5, 12, None),     # channels 0 = a 3-D single-channel volume
    Case("flat", (36, 40, 32), 4, 400, 0.5, 13, (slice(0, 36), slice(0, 22), slice(0, 32))),
    # piecewise-constant planes, colour-dominated (compactness 0.05): segments straddling a boundary
    # take a mixed colour and lose every voxel to their neighbours — 4 segments are emptied
    Case("empty", (30, 32, 28), 2, 200, 0.05, 2, "planes"),
)


def _planes_volume(case):
    """Two channels of constant regions cut by an oblique plane and stripes along x, the second with
    a little noise; labels follow the regions."""
    rng = np.random.default_rng(case.seed)
    d, h, w = case.shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    a = np.where(0.7 * z + 0.4 * y + 0.2 * x > 22, 0.9, 0.25).astype(np.float32)
    a[x % 9 < 2] = 0.6
    b = a * 0.5 + 0.1 * rng.random((d, h, w)).astype(np.float32)
    labels = np.select([a == np.float32(0.9), a == np.float32(0.6)], [1, 3], 0).astype(np.int16)
    return np.stack([a, b], -1), labels


def make_volume(case):
    """float32 intensities (a noisy ellipsoid on a zero background with a brighter blob) and
    int16 labels in {0, 1, 2, 3}.  Deterministic in the seed (numpy PCG64)."""
    if case.constant_box == "planes":
        return _planes_volume(case)
    rng = np.random.default_rng(case.seed)
    d, h, w = case.shape
    z, y, x = np.meshgrid(np.linspace(-1, 1, d), np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    brain = (z / 0.85) ** 2 + (y / 0.9) ** 2 + (x / 0.8) ** 2 < 1.0
    blob = (z - 0.2) ** 2 + (y + 0.1) ** 2 + (x - 0.15) ** 2 < 0.12
    n_ch = max(case.channels, 1)
    img = np.zeros((d, h, w, n_ch), dtype=np.float32)
    for ch in range(n_ch):
        base = 0.4 + 0.1 * ch + 0.2 * np.sin(3 * z + ch) * np.cos(2 * y)
        v = base + 0.08 * rng.standard_normal((d, h, w)) + 0.5 * blob
        img[..., ch] = np.where(brain, v, 0.0).astype(np.float32)
    if case.constant_box is not None:
        img[case.constant_box] = 0.25
    labels = np.zeros((d, h, w), dtype=np.int16)
    labels[blob] = 1
    labels[blob & (rng.random((d, h, w)) < 0.3)] = 2
    labels[blob & (z > 0.3)] = 3
    if case.channels == 0:
        img = img[..., 0]
    return img, labels


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()
