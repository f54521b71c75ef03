"""The per-lesion intensity and texture tables of gts.texture in scipy and numpy, written straight
from the definitions and independent of the package: lesions from scipy's label, levels from the float64 expression,
the histogram from bincount, the GLCM from shifted-array comparison per direction (no lists, no chunks, no folding),
and every float feature in exact rational arithmetic (fractions.Fraction over the integer counts; math.fsum where a
logarithm is needed) beside the sum of the absolute values of its terms.  Also the cases the host and the GPU tests
share, so the host test can check that this reference stays cheap on every one of them."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

from tests import measure_ref

MAX_LEVELS = 128
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]   # the first non-zero one is +1
HIST_KEYS = ("min", "max", "range", "levels", "mean_level", "variance", "skewness", "kurtosis", "median_level",
             "p10_level", "p90_level", "mode_level", "entropy", "uniformity", "mean_intensity_approx")
GLCM_KEYS = ("joint_maximum", "joint_average", "joint_variance", "joint_entropy", "difference_average",
             "difference_variance", "difference_entropy", "sum_average", "sum_variance", "sum_entropy",
             "angular_second_moment", "contrast", "dissimilarity", "inverse_difference", "inverse_difference_moment",
             "correlation", "autocorrelation", "cluster_tendency", "cluster_shade", "cluster_prominence",
             "information_correlation_1", "information_correlation_2")


class Refused(Exception):
    pass


def grey_levels(values, lo, hi, bins=32, bin_width=None):
    """(levels of float64 `values`, number of levels) of a lesion whose range is [lo, hi]."""
    v, lo, hi = np.asarray(values, dtype=np.float64), np.float64(lo), np.float64(hi)
    if bin_width is not None:
        w = np.float64(bin_width)
        return (np.floor(v / w) - np.floor(lo / w)).astype(np.int64), int(np.floor(hi / w) - np.floor(lo / w)) + 1
    if hi == lo:
        return np.zeros(v.shape, dtype=np.int64), 1
    n = np.float64(bins)
    return np.minimum(bins - 1, np.floor((v - lo) * n / (hi - lo))).astype(np.int64), int(bins)


def lesion_texture(labels, image, region, connectivity=26, bins=32, bin_width=None, min_lesion_voxels=1):
    """The integer tables of gts.texture.lesion_texture for numpy volumes: root, n, lo, hi, levels [L], hist [L, G],
    glcm [L, 13, G, G] (int64, symmetric), G the largest `levels`.  A non-finite value inside a selected lesion, or
    more than MAX_LEVELS levels, raises Refused (its args: the root)."""
    labels, image = np.asarray(labels), np.asarray(image)
    mask = measure_ref.region_mask(labels, region)
    structure = ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1)
    lab, count = ndimage.label(mask, structure=structure)
    sizes = np.bincount(lab.ravel(), minlength=count + 1)
    chosen = [k for k in range(1, count + 1) if sizes[k] >= min_lesion_voxels]     # ascending root, as scipy labels
    row_of = np.full(count + 1, -1, dtype=np.int64)
    row_of[chosen] = np.arange(len(chosen))
    level = np.zeros(labels.shape, dtype=np.int64)
    out = dict(root=[], n=[], lo=[], hi=[], levels=[])
    for k in chosen:
        where = lab == k
        values = image[where]
        root = 1 + int(np.flatnonzero(where.ravel())[0])
        if not np.all(np.isfinite(values)):
            raise Refused(root)
        lo, hi = values.min(), values.max()
        g, n_levels = grey_levels(values, lo, hi, bins, bin_width)
        if n_levels > MAX_LEVELS:
            raise Refused(root)
        level[where] = g
        for key, value in zip(("root", "n", "lo", "hi", "levels"), (root, int(where.sum()), lo, hi, n_levels)):
            out[key].append(value)
    L, G = len(chosen), max(out["levels"], default=1)
    hist = np.zeros((L, G), dtype=np.int64)
    glcm = np.zeros((L, len(DIRECTIONS), G, G), dtype=np.int64)
    np.add.at(hist, (row_of[lab[row_of[lab] >= 0]], level[row_of[lab] >= 0]), 1)
    for d, delta in enumerate(DIRECTIONS):
        here = tuple(slice(max(0, -s), labels.shape[a] - max(0, s)) for a, s in enumerate(delta))
        there = tuple(slice(max(0, s), labels.shape[a] - max(0, -s)) for a, s in enumerate(delta))
        pair = (lab[here] == lab[there]) & (row_of[lab[here]] >= 0)      # the same lesion, and a selected one
        rows, i, j = row_of[lab[here][pair]], level[here][pair], level[there][pair]
        np.add.at(glcm, (rows, d, i, j), 1)                              # q = p + delta
        np.add.at(glcm, (rows, d, j, i), 1)                              # q = p - delta
    return dict(root=np.array(out["root"], dtype=np.int64), n=np.array(out["n"], dtype=np.int64),
                lo=np.array(out["lo"], dtype=image.dtype), hi=np.array(out["hi"], dtype=image.dtype),
                levels=np.array(out["levels"], dtype=np.int64), hist=hist, glcm=glcm, bins=bins, bin_width=bin_width)


# ------------------------------------------------------------------ the float features, exactly
def _entropy(probabilities):
    """(-sum p log2 p by fsum over the rounded terms, the sum of their absolute values)."""
    terms = [-(p * math.log2(p)) for p in probabilities if p > 0.0]
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


def _rooted(value, root_of, power):
    """value / root_of ** power for a Fraction pair, 0.0 when both vanish."""
    if root_of == 0:
        return 0.0
    return float(value) / math.pow(float(root_of), power)


def histogram_features(table, k):
    """{key: (value, sum of |terms|)} of the histogram family of lesion k; levels are numbered from 1."""
    n_levels, n = int(table["levels"][k]), int(table["n"][k])
    counts = [int(c) for c in table["hist"][k][:n_levels]]
    lo, hi = Fraction(float(table["lo"][k])), Fraction(float(table["hi"][k]))
    p = [Fraction(c, n) for c in counts]
    level = range(1, n_levels + 1)
    mean = sum(i * q for i, q in zip(level, p))
    moment = {r: sum((i - mean) ** r * q for i, q in zip(level, p)) for r in (2, 3, 4)}
    abs3 = sum(abs(i - mean) ** 3 * q for i, q in zip(level, p))
    cumulative = np.cumsum(counts)

    def reach(num, den):                                   # the smallest level whose cumulative count reaches num/den
        return 1 + int(np.flatnonzero(cumulative * den >= n * num)[0])

    if table["bin_width"] is not None:
        w = Fraction(float(table["bin_width"]))
        centre = (math.floor(lo / w) + mean - Fraction(1, 2)) * w
        centre_abs = (abs(math.floor(lo / w)) + mean + Fraction(1, 2)) * w
    else:
        centre = lo + (mean - Fraction(1, 2)) * (hi - lo) / table["bins"] if hi != lo else lo
        centre_abs = abs(lo) + (mean + Fraction(1, 2)) * (hi - lo) / table["bins"]
    entropy = _entropy([float(q) for q in p])
    kurt = moment[4] / moment[2] ** 2 if moment[2] else Fraction(3)
    out = dict(min=(lo, abs(lo)), max=(hi, abs(hi)), range=(hi - lo, abs(hi) + abs(lo)), levels=(n_levels, n_levels),
               mean_level=(mean, mean), variance=(moment[2], moment[2]),
               skewness=(_rooted(moment[3], moment[2], 1.5), _rooted(abs3, moment[2], 1.5)),
               kurtosis=(kurt - 3, kurt + 3), median_level=(reach(1, 2),) * 2, p10_level=(reach(1, 10),) * 2,
               p90_level=(reach(9, 10),) * 2, mode_level=(1 + int(np.argmax(counts)),) * 2, entropy=entropy,
               uniformity=(sum(q * q for q in p),) * 2, mean_intensity_approx=(centre, centre_abs))
    return out


def _direction_features(matrix):
    """{key: (value, sum of |terms|)} of one direction's symmetric count matrix with at least one pair."""
    G = matrix.shape[0]
    total = int(matrix.sum())
    p = {(i + 1, j + 1): Fraction(int(matrix[i, j]), total) for i in range(G) for j in range(G) if matrix[i, j]}
    px = {}
    diff, plus = {}, {}
    for (i, j), q in p.items():
        px[i] = px.get(i, 0) + q
        diff[abs(i - j)] = diff.get(abs(i - j), 0) + q
        plus[i + j] = plus.get(i + j, 0) + q
    mu = sum(i * q for i, q in px.items())
    var = sum((i - mu) ** 2 * q for i, q in px.items())
    d_mean = sum(k * q for k, q in diff.items())
    s_mean = sum(k * q for k, q in plus.items())
    auto = sum(i * j * q for (i, j), q in p.items())
    hxy = _entropy([float(q) for q in p.values()])
    hx = _entropy([float(q) for q in px.values()])
    hxy1 = _entropy_cross(p, px)
    hxy2 = _entropy_cross({(i, j): a * b for i, a in px.items() for j, b in px.items()}, px)
    imc1 = ((hxy[0] - hxy1[0]) / hx[0], (hxy[1] + hxy1[1]) / hx[0]) if hx[0] > 0.0 else (0.0, 0.0)
    gap = hxy2[0] - hxy[0]
    imc2 = math.sqrt(1.0 - math.exp(-2.0 * gap)) if gap > 0.0 else 0.0
    out = dict(joint_maximum=(max(p.values()),) * 2, joint_average=(mu, mu), joint_variance=(var, var),
               joint_entropy=hxy, difference_average=(d_mean, d_mean),
               difference_variance=(sum((k - d_mean) ** 2 * q for k, q in diff.items()),) * 2,
               difference_entropy=_entropy([float(q) for q in diff.values()]), sum_average=(s_mean, s_mean),
               sum_variance=(sum((k - s_mean) ** 2 * q for k, q in plus.items()),) * 2,
               sum_entropy=_entropy([float(q) for q in plus.values()]),
               angular_second_moment=(sum(q * q for q in p.values()),) * 2,
               contrast=(sum(k * k * q for k, q in diff.items()),) * 2, dissimilarity=(d_mean, d_mean),
               inverse_difference=(sum(q / (1 + k) for k, q in diff.items()),) * 2,
               inverse_difference_moment=(sum(q / (1 + k * k) for k, q in diff.items()),) * 2,
               correlation=((auto - mu * mu) / var, (auto + mu * mu) / var) if var else (Fraction(1), Fraction(1)),
               autocorrelation=(auto, auto),
               cluster_tendency=(sum((k - 2 * mu) ** 2 * q for k, q in plus.items()),) * 2,
               cluster_shade=(sum((k - 2 * mu) ** 3 * q for k, q in plus.items()),
                              sum(abs(k - 2 * mu) ** 3 * q for k, q in plus.items())),
               cluster_prominence=(sum((k - 2 * mu) ** 4 * q for k, q in plus.items()),) * 2,
               information_correlation_1=imc1, information_correlation_2=(imc2, imc2))
    return out


def _entropy_cross(weights, px):
    """(-sum w(i, j) log2(px(i) px(j)), the sum of |terms|), the logarithm of the rounded product."""
    terms = [-(float(w) * math.log2(float(px[i]) * float(px[j]))) for (i, j), w in weights.items() if w]
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


def glcm_features(table, k):
    """{key: (value, sum of |terms|)}: each feature per direction on the normalised matrix, averaged over the
    directions that hold at least one pair; None when no direction does."""
    n_levels = int(table["levels"][k])
    per = [_direction_features(m[:n_levels, :n_levels]) for m in table["glcm"][k] if m.any()]
    if not per:
        return None
    return {key: tuple(sum(f[key][s] for f in per) / len(per) for s in (0, 1)) for key in GLCM_KEYS}


# ------------------------------------------------------------------ the cases the tests share
BOX = (2, 3, 5)


def box_cases():
    """{name: (labels, image)}: a constant-intensity 2 x 3 x 5 box at a corner, on a face, in the interior and filling
    its volume, and a 3 x 3 x 1 volume with a unit axis."""
    block = np.ones(BOX, dtype=bool)
    cases = {}
    for where, vol in measure_ref.placements(block).items():
        cases[f"box-{where}"] = (vol, np.full(vol.shape, 7, dtype=np.int16))
    cases["box-whole"] = (measure_ref.embed(block, BOX, (0, 0, 0)), np.full(BOX, -3, dtype=np.int16))
    cases["unit-axis"] = (np.full((3, 3, 1), 3, dtype=np.int16), np.full((3, 3, 1), 2.5, dtype=np.float32))
    return cases


def ramp_case(extent=(6, 4, 3)):
    """Intensity = the x index over a box one voxel inside its volume; bins = the x extent."""
    vol = np.zeros(tuple(e + 2 for e in extent), dtype=np.int16)
    vol[1:-1, 1:-1, 1:-1] = 1
    image = np.broadcast_to(np.arange(extent[0] + 2, dtype=np.int16)[:, None, None] - 1, vol.shape).copy()
    return vol, image, extent


def checkerboard_case(extent=(4, 5, 3)):
    vol = np.full(extent, 2, dtype=np.int16)
    return vol, (np.indices(extent).sum(axis=0) % 2).astype(np.float32), extent


def touching_case():
    """Two boxes that touch along an edge and two that touch at a corner only, of different intensities."""
    vol = np.zeros((6, 6, 6), dtype=np.int16)
    image = np.zeros(vol.shape, dtype=np.int16)
    vol[0:2, 0:2, 0:3], image[0:2, 0:2, 0:3] = 1, 10
    vol[2:4, 2:4, 0:3], image[2:4, 2:4, 0:3] = 1, 20        # an edge along z with the first
    vol[4:6, 4:6, 3:6], image[4:6, 4:6, 3:6] = 1, 35        # a corner with the second
    image[1, 1, 2], image[2, 2, 2], image[4, 4, 3] = 12, 27, 31
    return vol, image


def chunk_case(voxels, chunk, seed=0):
    """One lesion of exactly `voxels` voxels (a filled prefix of a 17-row volume in C order) with random values."""
    side = 17
    depth = -(-voxels // (side * side))
    flat = np.zeros(side * side * depth, dtype=np.int16)
    flat[:voxels] = 3
    rng = np.random.default_rng([seed, voxels, chunk])
    return flat.reshape(depth, side, side), rng.integers(-500, 500, (depth, side, side)).astype(np.int16)


def random_image(shape, dtype, seed):
    rng = np.random.default_rng([seed] + list(shape))
    if dtype == np.int16:
        return rng.integers(-300, 1200, shape).astype(np.int16)
    return (rng.normal(0.0, 40.0, shape) + 0.25 * rng.integers(-8, 8, shape)).astype(np.float32)


def selection_cases():
    """[(name, labels, image)]: measure_ref's random volumes, int16 and float32 images alternating."""
    cases = []
    for k, (shape, p) in enumerate(itertools.product(measure_ref.RANDOM_SHAPES, measure_ref.RANDOM_P)):
        dtype = (np.int16, np.float32)[k % 2]
        cases.append((f"random-{'x'.join(map(str, shape))}-{p}-{np.dtype(dtype).name}",
                      measure_ref.random_volume(shape, p), random_image(shape, dtype, k)))
    return cases


def contention_cases():
    big = np.full((16, 16, 16), 1, dtype=np.int16)
    rng = np.random.default_rng(7)
    return {"constant": (big, np.full(big.shape, 100, dtype=np.int16), 32),
            "uniform-128": (big, rng.integers(0, 128, big.shape).astype(np.int16), 128)}


@functools.lru_cache(maxsize=None)
def cached_selection():
    return selection_cases()


@functools.lru_cache(maxsize=None)
def cached_selection_table(index, connectivity, min_lesion_voxels):
    """lesion_texture of a selection case (region WT, 32 bins), computed once per session; do not modify."""
    _, labels, image = cached_selection()[index]
    return lesion_texture(labels, image, "WT", connectivity, 32, None, min_lesion_voxels)
