"""numpy / scipy reference of the brain extraction, written from the definition and independent of
gts/brainmask.py: the GPU tests hold S1-S6 and brain_mask to it integer for integer and voxel for voxel."""
import math

import numpy as np
from scipy import ndimage

BINS = 4096


def squared_radius(radius):
    return int(math.floor(float(radius) * float(radius)))


def ball(r2):
    """bool [2 r + 1] * 3, r = floor(sqrt(r2)): the offsets o with |o|^2 <= r2."""
    r = math.isqrt(int(r2))
    o = np.arange(-r, r + 1)
    return (o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) <= int(r2)


def positive(v):
    f = np.asarray(v).astype(np.float64)
    return np.isfinite(f) & (f > 0)


def brain_range(v):
    """(n, hi as float64); ValueError when no voxel is finite and > 0."""
    p = positive(v)
    n = int(p.sum())
    if n == 0:
        raise ValueError("no positive voxel")
    return n, np.float64(np.asarray(v)[p].max())


def histogram(v, hi):
    p = positive(v)
    f = np.asarray(v)[p].astype(np.float64)
    bins = np.minimum(BINS - 1, np.floor(f / np.float64(hi) * 4096.0).astype(np.int64))
    return np.bincount(bins, minlength=BINS).astype(np.int64)


def threshold_from_counts(counts, hi, fraction):
    """The definition as a plain loop over the bins."""
    n = int(sum(int(c) for c in counts))
    need2, need98 = math.ceil(0.02 * n), math.ceil(0.98 * n)
    b2 = b98 = None
    cum = 0
    for b in range(BINS):
        cum += int(counts[b])
        if b2 is None and cum >= need2:
            b2 = b
        if b98 is None and cum >= need98:
            b98 = b
    t = (np.float64(b2) + np.float64(fraction) * np.float64(b98 - b2)) * np.float64(hi) / np.float64(4096.0)
    return float(t), b2, b98


def erode(mask, r2, border_value=0):
    return ndimage.binary_erosion(np.asarray(mask) != 0, structure=ball(r2), border_value=border_value)


def dilate(mask, r2):
    return ndimage.binary_dilation(np.asarray(mask) != 0, structure=ball(r2))


def morph_brute(mask, r2, target, outside):
    """bool: the squared distance to the nearest position equal to `target` is <= r2, positions outside the volume
    counting as target iff outside.  Brute force: one shifted copy of the padded volume per offset of the ball.
    Offsets longer than an extent along its axis are left out: they only reach positions outside, and a position
    outside at the same other two coordinates lies nearer."""
    hit = (np.asarray(mask) != 0) == bool(target)
    r = math.isqrt(int(r2))
    pad = [min(r, n) for n in hit.shape]
    padded = np.pad(hit, [(p, p) for p in pad], constant_values=bool(outside))
    out = np.zeros(hit.shape, dtype=bool)
    X, Y, Z = hit.shape
    for dx in range(-pad[0], pad[0] + 1):
        for dy in range(-pad[1], pad[1] + 1):
            for dz in range(-pad[2], pad[2] + 1):
                if dx * dx + dy * dy + dz * dz <= r2:
                    out |= padded[pad[0] + dx:pad[0] + dx + X, pad[1] + dy:pad[1] + dy + Y, pad[2] + dz:pad[2] + dz + Z]
    return out


def largest_component(mask, connectivity=6):
    """(keep bool, components, largest, second); a tie goes to the component whose first voxel in C order comes first
    (ndimage.label numbers the components in that order).  ValueError for an empty mask."""
    lab, count = ndimage.label(np.asarray(mask) != 0,
                               structure=ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    if count == 0:
        raise ValueError("empty mask")
    sizes = np.bincount(lab.reshape(-1))[1:]
    winner = int(np.argmax(sizes))              # the first maximum
    rest = np.delete(sizes, winner)
    return lab == winner + 1, int(count), int(sizes[winner]), int(rest.max()) if rest.size else 0


def fill_holes(mask):
    return ndimage.binary_fill_holes(np.asarray(mask) != 0)


def brain_mask(v, radius=3.0, close=2.0, fraction=0.1, connectivity=6):
    """(mask bool, report with the integers of gts.brainmask.brain_mask's report)."""
    v = np.asarray(v)
    r2e, r2c = squared_radius(radius), squared_radius(close)
    n, hi = brain_range(v)
    t, _, _ = threshold_from_counts(histogram(v, hi), hi, fraction)
    m0 = positive(v) & (v.astype(np.float64) >= t)
    e = erode(m0, r2e, 0)
    keep, components, largest, second = largest_component(e, connectivity)
    d = dilate(keep, r2e)
    c = erode(dilate(d, r2c), r2c, 1) if r2c > 0 else d
    b = fill_holes(c)
    report = {"threshold": t, "hi": float(hi), "positive_voxels": n, "threshold_voxels": int(m0.sum()),
              "eroded_voxels": int(e.sum()), "components": components, "largest": largest, "second": second,
              "mask_voxels": int(b.sum())}
    return b, report


def apply_mask(scan, mask):
    scan = np.asarray(scan)
    return np.where(np.asarray(mask) != 0, scan, np.zeros((), dtype=scan.dtype)).astype(scan.dtype)


def dice(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return 2.0 * float((a & b).sum()) / float(a.sum() + b.sum())


_PHANTOM = {}


def phantom_case(shape, seed):
    """(t1 volume int16 [X, Y, Z], truth bool, reference mask and report at the defaults) of the head phantom, computed
    once per process and shared: nobody writes to them."""
    key = (tuple(shape), int(seed))
    if key not in _PHANTOM:
        from gts import synth_mri

        img, _, truth = synth_mri.make_head_sample(seed, shape)
        t1 = np.ascontiguousarray(img[..., 1].astype(np.int16))
        mask, report = brain_mask(t1)
        for a in (t1, truth, mask):
            a.setflags(write=False)
        _PHANTOM[key] = (t1, truth, mask, report)
    return _PHANTOM[key]
