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


def assign_ref(scaled, centres, window, spatial_weight, labels):
    """One SLIC assignment: the labels after every centre k = 0, 1, ... (NaN centres skipped) has
    claimed, with strict '<', the voxels of its window it is nearer to than every earlier centre.
    A voxel inside no window keeps its label from `labels`, which is left unchanged."""
    if scaled.ndim == 3:
        scaled = scaled[..., None]
    d, h, w, c = scaled.shape
    wz, wy, wx = window
    labels = np.array(labels, dtype=np.int64)
    dist_img = np.full((d, h, w), np.finfo(np.float64).max)
    for k in range(len(centres)):
        cz, cy, cx = centres[k, :3]
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
        dist = ((dz + dy) + dx) * spatial_weight
        win = scaled[z0:z1, y0:y1, x0:x1]
        col = np.zeros(dist.shape)
        for ch in range(c):
            col = col + (win[..., ch] - centres[k, 3 + ch]) ** 2
        dist = dist + col
        sub = dist_img[z0:z1, y0:y1, x0:x1]
        better = dist < sub
        sub[better] = dist[better]
        labels[z0:z1, y0:y1, x0:x1][better] = k
    return labels


def update_ref(scaled, labels, n_centres):
    """One SLIC centre update: [n_centres, 3 + C] means of (z, y, x, colours) per label, every sum
    in raster order (np.bincount adds its weights in index order); a label that owns nothing gets
    a 0/0 = NaN row.  Labels outside [0, n_centres) belong to nobody."""
    if scaled.ndim == 3:
        scaled = scaled[..., None]
    d, h, w, c = scaled.shape
    zz, yy, xx = np.mgrid[:d, :h, :w]
    lab = np.asarray(labels).ravel()
    own = (lab >= 0) & (lab < n_centres)
    lab = lab[own]
    counts = np.bincount(lab, minlength=n_centres).astype(np.float64)
    sums = [np.bincount(lab, weights=a.ravel()[own].astype(np.float64), minlength=n_centres) for a in (zz, yy, xx)]
    sums += [np.bincount(lab, weights=scaled[..., ch].ravel()[own], minlength=n_centres) for ch in range(c)]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack(sums, axis=1) / counts[:, None]


def slic_rounds_ref(scaled, n_segments, max_iter=10, emptied=None, at_update=None):
    """Labels (int64, before connectivity) of max_iter SLIC rounds over `scaled` [D,H,W,C].
    `emptied`, a list, receives the number of emptied segments (NaN centres) after each update;
    `at_update`, a list, a copy of the labels each update reads."""
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
    window = _steps(regular_grid((d, h, w), n_c))
    labels = np.full((d, h, w), -1, dtype=np.int64)
    for it in range(max_iter):
        labels = assign_ref(scaled, seg, window, sw, labels)
        if it == 0:
            assert (labels >= 0).all(), "a voxel lies in no window in the first round"
        if it == max_iter - 1:
            break
        if at_update is not None:
            at_update.append(labels.copy())
        seg = update_ref(scaled, labels, n_c)
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


# ---- stage references: statistics, discard, kNN candidates, face adjacency -------

QUANTILES = (0.1, 0.25, 0.5, 0.75, 0.9)


def _segments(partition, n_sv):
    """(order, starts, ends): order[starts[k]:ends[k]] are the raster indices of label k, ascending."""
    part = np.asarray(partition).ravel()
    order = np.argsort(part, kind="stable")
    ks = np.arange(n_sv)
    return order, np.searchsorted(part[order], ks, "left"), np.searchsorted(part[order], ks, "right")


def _stats_inputs(partition, img_f32, vox_labels):
    img = np.asarray(img_f32)
    assert img.dtype == np.float32, "the statistics contract is float32 intensities"
    shape = np.asarray(partition).shape
    flat = img.reshape(int(np.prod(shape)), -1)
    coords = np.stack(np.unravel_index(np.arange(flat.shape[0]), shape), axis=1).astype(np.int64)
    vl = None if vox_labels is None else np.asarray(vox_labels).ravel()
    return flat, coords, vl


def stats_ref(partition, img_f32, vox_labels, n_sv):
    """(feats [n_sv, 5C] fp64, centroids [n_sv, 3] fp64, labels [n_sv] int32): per segment and
    channel np.quantile of the float32 values, the most frequent voxel label (the smallest among
    equally frequent ones; 0 without voxel labels) and integer coordinate sums / count.  A label
    no voxel carries gets feats -1, a NaN centroid and label -1."""
    flat, coords, vl = _stats_inputs(partition, img_f32, vox_labels)
    c = flat.shape[1]
    order, starts, ends = _segments(partition, n_sv)
    feats = np.full((n_sv, 5 * c), -1.0)
    cents = np.full((n_sv, 3), np.nan)
    labs = np.full(n_sv, -1, dtype=np.int32)
    for k in range(n_sv):
        idx = order[starts[k]:ends[k]]
        if len(idx) == 0:
            continue
        for ch in range(c):
            feats[k, 5 * ch:5 * ch + 5] = np.quantile(flat[idx, ch], QUANTILES)
        if vl is None:
            labs[k] = 0
        else:
            vals, counts = np.unique(vl[idx], return_counts=True)
            labs[k] = vals[counts.argmax()]
        cents[k] = coords[idx].sum(axis=0) / len(idx)
    return feats, cents, labs


def stats_ref_grouped(partition, img_f32, vox_labels, n_sv):
    """stats_ref without a Python loop over segments: segments of equal size are stacked and given
    to one np.quantile(axis=1); the mode comes from one np.unique over (segment, label) pairs."""
    flat, coords, vl = _stats_inputs(partition, img_f32, vox_labels)
    c = flat.shape[1]
    order, starts, ends = _segments(partition, n_sv)
    sizes = ends - starts
    feats = np.full((n_sv, 5 * c), -1.0)
    cents = np.full((n_sv, 3), np.nan)
    labs = np.where(sizes > 0, 0, -1).astype(np.int32)
    for n in np.unique(sizes[sizes > 0]):
        ks = np.flatnonzero(sizes == n)
        idx = order[starts[ks][:, None] + np.arange(n)[None, :]]
        for ch in range(c):
            feats[ks, 5 * ch:5 * ch + 5] = np.quantile(flat[idx, ch], QUANTILES, axis=1).T
        cents[ks] = coords[idx].sum(axis=1) / n
    if vl is not None:
        part = np.asarray(partition).ravel().astype(np.int64)
        own = (part >= 0) & (part < n_sv)
        pairs, counts = np.unique(part[own] * 65536 + (vl[own].astype(np.int64) + 32768), return_counts=True)
        seg, lab = pairs >> 16, (pairs & 65535) - 32768
        o = np.lexsort((lab, -counts, seg))                  # per segment: most frequent first, then smallest
        first = np.r_[True, seg[o][1:] != seg[o][:-1]]
        labs[seg[o][first]] = lab[o][first]
    return feats, cents, labs


def discard_ref(partition, feats, centroids, labels):
    """Drop the supervoxels whose feature 4 lies below min(feature 4) + 0.01 (strict '<', fp64),
    number the kept ones in order: (int16 partition with -1, node feats, centroids, labels)."""
    feats = np.asarray(feats, dtype=np.float64)
    keep = ~(feats[:, 4] < feats[:, 4].min() + 0.01)
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int16)
    part = np.asarray(partition)
    known = (part >= 0) & (part < len(keep))
    new_part = np.where(known, remap[np.where(known, part, 0)], -1).astype(np.int16)
    return new_part, feats[keep], np.asarray(centroids)[keep], np.asarray(labels)[keep]


def knn_candidates_ref(pos, k, order=None):
    """cand[i, t] = the t-th j > i in the stable argsort of row i of cdist(pos, pos); -1 past the end.
    `order` replaces that argsort (the sensitivity checks pass an unstable one)."""
    from scipy.spatial.distance import cdist

    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    if order is None:
        order = np.argsort(cdist(pos, pos), axis=1, kind="stable")
    cand = np.full((n, k), -1, dtype=np.int32)
    for i in range(n):
        js = order[i][order[i] > i][:k]
        cand[i, :len(js)] = js
    return cand


def touching_ref(partition_i16, n):
    """Sorted (row, col) pairs of the face adjacency among nodes 0..n-1: the label pairs across the
    three axis shifts in both orientations, a self-loop on every node; labels < 0 or >= n are nobody."""
    part = np.asarray(partition_i16).astype(np.int64)
    pairs = [np.stack([np.arange(n), np.arange(n)], axis=1)]
    for axis in range(3):
        a = part[tuple(slice(None, -1) if ax == axis else slice(None) for ax in range(3))].ravel()
        b = part[tuple(slice(1, None) if ax == axis else slice(None) for ax in range(3))].ravel()
        nodes = (a >= 0) & (a < n) & (b >= 0) & (b < n) & (a != b)
        pairs += [np.stack([a[nodes], b[nodes]], axis=1), np.stack([b[nodes], a[nodes]], axis=1)]
    return [tuple(p) for p in np.unique(np.concatenate(pairs), axis=0).tolist()]


# ---- edge-shape inputs shared by the host and the GPU edge tests -----------------------------------

WIDE_SLIC = {   # name -> (shape, n_segments, channels, compactness): step >= 16 along x
    "300x3-c1": ((4, 6, 300), 3, 1, 0.05),
    "300x3-c2": ((4, 6, 300), 3, 2, 0.5),
    "400x2-c8": ((3, 5, 400), 2, 8, 0.5),
    "260x4-c3": ((6, 8, 260), 4, 3, 0.05),
}


def striped_volume(name):
    """float64 [D,H,W,C]: stripes of period 14 along x under uniform noise, seeded by the case."""
    shape, _, c, _ = WIDE_SLIC[name]
    rng = np.random.default_rng(sorted(WIDE_SLIC).index(name) + 40)
    x = np.arange(shape[2])
    return 0.2 * rng.random(shape + (c,)) + ((x // 7) % 2)[None, None, :, None]


def x_runs(mask):
    """Number of maximal runs of consecutive x a 3-D mask occupies (projected on the x axis)."""
    occ = mask.any(axis=(0, 1)).astype(np.int8)
    return int((np.diff(np.r_[0, occ]) == 1).sum())


STATS_SIZES = (1, 2, 3, 5, 255, 256, 257, 4095, 4096, 4097, 9000)
STATS_ABSENT = 5            # a label in the middle that no voxel carries; so is the last, n_sv - 1


def stats_edge_case():
    """(partition int32, img float32 [.., 3], labels int16, n_sv): segments of exactly STATS_SIZES
    scattered over a 28x28x29 volume, labels STATS_ABSENT and n_sv - 1 absent, the spare voxels
    labelled -1 and n_sv.  Channel 0 holds four distinct values; channel 1 puts the lower quarter of
    each segment near 1e-1 and the rest near 1e7, so the 0.25 quantile interpolates across a float32
    subtraction that rounds; voxel labels are negative and positive with exact mode ties."""
    rng = np.random.default_rng(77)
    shape = (28, 28, 29)
    n_vox = int(np.prod(shape))
    n_sv = len(STATS_SIZES) + 2
    names = [k for k in range(n_sv - 1) if k != STATS_ABSENT]
    perm = rng.permutation(n_vox)
    part = np.where(np.arange(n_vox) % 2 == 0, -1, n_sv).astype(np.int32)
    img = np.empty((n_vox, 3), dtype=np.float32)
    img[:, 0] = rng.integers(0, 4, n_vox) / np.float32(4)
    img[:, 1] = (1e7 + 1e7 * rng.random(n_vox)).astype(np.float32)
    img[:, 2] = rng.standard_normal(n_vox).astype(np.float32)
    lab = rng.choice(np.array([-3, -1, 0, 2, 7], dtype=np.int16), n_vox)
    at = 0
    for k, n in zip(names, STATS_SIZES):
        idx = perm[at:at + n]
        at += n
        part[idx] = k
        small = int(np.floor((n - 1) * 0.25)) + 1
        img[idx[:small], 1] = (0.1 + 0.1 * rng.random(small)).astype(np.float32)
        if n == 2:
            lab[idx] = [2, -3]                               # tie: -3
        if n == 256:
            lab[idx[:128]], lab[idx[128:]] = 7, -1           # tie: -1
    return part.reshape(shape), img.reshape(shape + (3,)), lab.reshape(shape), n_sv


def quantile_float64_diff(values, q):
    """np.quantile's linear rule with hi - lo formed in float64: NOT the contract (numpy subtracts in
    the data's float32); the sensitivity check shows the two differ on stats_edge_case."""
    a = np.sort(np.asarray(values)).astype(np.float64)
    out = []
    for qq in q:
        vi = (len(a) - 1) * qq
        p = int(np.floor(vi))
        t = vi - p
        hi = a[min(p + 1, len(a) - 1)]
        out.append(hi - (hi - a[p]) * (1.0 - t) if t >= 0.5 else a[p] + (hi - a[p]) * t)
    return np.array(out)


def lattice_positions(n, seed=0):
    """n distinct points of a half-integer cubic lattice in a shuffled order: every squared distance
    is exact in fp64 and most rows have many exactly equal distances."""
    rng = np.random.default_rng(1000 + seed + n)
    m = int(np.ceil(n ** (1.0 / 3.0))) + 1
    cells = rng.choice(m ** 3, size=n, replace=False)
    return np.stack(np.unravel_index(cells, (m, m, m)), axis=1) / 2.0


def blocky_partition(shape, block, n, seed):
    """int16 partition of random cubes labelled -1 .. n + 2: -1 and the labels >= n are nobody."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(-1, n + 3, size=tuple(-(-s // block) for s in shape))
    part = np.kron(coarse, np.ones((block,) * 3, dtype=np.int64))[:shape[0], :shape[1], :shape[2]].astype(np.int16)
    part[0, 0, 0], part[-1, -1, -1] = -1, n                   # both kinds of nobody, whatever the draw
    return part
