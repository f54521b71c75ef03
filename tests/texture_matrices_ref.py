"""The per-lesion run-length, size-zone, dependence and neighbourhood-difference tables of gts.texture (GLRLM, GLSZM,
GLDM, NGTDM) in scipy and numpy, written from the definitions and independent of the package: lesions
and levels as tests/texture_ref.py states them, run starts and neighbourhoods from shifted-array comparison, zones
from scipy's label with the full 3 x 3 x 3 structure per lesion and level (no lists, no chunks, no union-find), and
every float feature in exact rational arithmetic (math.fsum where a logarithm is needed) beside the sum of the
absolute values of its terms.  Also the cases only these families need."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

from tests import measure_ref
from tests import texture_ref

DIRECTIONS = texture_ref.DIRECTIONS
NEIGHBOURS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
MATRICES = ("glrlm", "glszm", "gldm", "ngtdm")
TABLE_KEYS = ("glrlm", "zones", "gldm", "ngtdm_n", "ngtdm_s")
_HEAD = ("{short}_emphasis", "{long}_emphasis", "low_grey_level_{unit}_emphasis", "high_grey_level_{unit}_emphasis",
         "{s}_low_grey_level_emphasis", "{s}_high_grey_level_emphasis", "{l}_low_grey_level_emphasis",
         "{l}_high_grey_level_emphasis", "grey_level_non_uniformity", "grey_level_non_uniformity_normalised",
         "{size}_non_uniformity", "{size}_non_uniformity_normalised")


def _keys(prefix, tail, **words):
    return tuple(f"{prefix}_{key.format(**words)}" for key in _HEAD + tail)


GLRLM_KEYS = _keys("glrlm", ("run_percentage", "grey_level_variance", "run_length_variance", "run_entropy"),
                   short="short_runs", long="long_runs", unit="run", s="short_run", l="long_run", size="run_length")
GLSZM_KEYS = _keys("glszm", ("zone_percentage", "grey_level_variance", "zone_size_variance", "zone_size_entropy"),
                   short="small_zone", long="large_zone", unit="zone", s="small_zone", l="large_zone", size="zone_size")
GLDM_KEYS = _keys("gldm", ("grey_level_variance", "dependence_count_variance", "dependence_count_entropy",
                           "dependence_count_energy"),
                  short="low_dependence", long="high_dependence", unit="count", s="low_dependence",
                  l="high_dependence", size="dependence_count")
NGTDM_KEYS = ("ngtdm_coarseness", "ngtdm_contrast", "ngtdm_busyness", "ngtdm_complexity", "ngtdm_strength")


def _volumes(labels, image, region, connectivity, bins, bin_width, min_lesion_voxels):
    """(row: the selected lesion of every voxel in texture_ref's order or -1, level: its grey level) as volumes."""
    mask = measure_ref.region_mask(labels, region)
    structure = ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1)
    lab, count = ndimage.label(mask, structure=structure)
    sizes = np.bincount(lab.ravel(), minlength=count + 1)
    chosen = [k for k in range(1, count + 1) if sizes[k] >= min_lesion_voxels]
    row_of = np.full(count + 1, -1, dtype=np.int64)
    row_of[chosen] = np.arange(len(chosen))
    row = row_of[lab]
    level = np.zeros(labels.shape, dtype=np.int64)
    boxes = ndimage.find_objects(lab)
    for k in chosen:
        where = lab[boxes[k - 1]] == k
        values = image[boxes[k - 1]][where]
        level[boxes[k - 1]][where] = texture_ref.grey_levels(values, values.min(), values.max(), bins, bin_width)[0]
    return row, level, boxes, chosen


def _shifted(shape, delta):
    """(here, there): slices with volume[there] = volume[here] moved by delta, over the voxels where both exist."""
    here = tuple(slice(max(0, -s), shape[a] - max(0, s)) for a, s in enumerate(delta))
    there = tuple(slice(max(0, s), shape[a] - max(0, -s)) for a, s in enumerate(delta))
    return here, there


def _runs(row, level, L, G):
    """glrlm [L, 13, G, R]."""
    shape = row.shape
    found = []
    for d, delta in enumerate(DIRECTIONS):
        here, there = _shifted(shape, delta)
        follows = np.zeros(shape, dtype=bool)            # the voxel continues the run of its predecessor p - delta
        follows[there] = (row[there] >= 0) & (row[there] == row[here]) & (level[there] == level[here])
        at = np.argwhere((row >= 0) & ~follows)          # the run starts
        rows, levels = row[tuple(at.T)], level[tuple(at.T)]
        length = np.ones(len(at), dtype=np.int64)
        alive = np.arange(len(at))
        pos = at.copy()
        while len(alive):
            pos = pos + np.array(delta)
            ok = np.all((pos >= 0) & (pos < np.array(shape)), axis=1)
            ok[ok] = follows[tuple(pos[ok].T)]
            alive, pos = alive[ok], pos[ok]
            length[alive] += 1
        found.append((rows, levels, length))
    R = max((int(f[2].max()) for f in found if len(f[2])), default=1)
    glrlm = np.zeros((L, len(DIRECTIONS), G, R), dtype=np.int64)
    for d, (rows, levels, length) in enumerate(found):
        np.add.at(glrlm, (rows, d, levels, length - 1), 1)
    return glrlm


def _zones(row, level, boxes, chosen):
    """zones [K, 4]: (lesion, level, size, count), ascending."""
    full = np.ones((3, 3, 3), dtype=bool)
    records = []
    for l, k in enumerate(chosen):
        box = boxes[k - 1]
        mine, levels = row[box] == l, level[box]
        if mine.sum() == 1:
            records.append((l, int(levels[mine][0]), 1))
            continue
        for g in np.unique(levels[mine]):
            lab, count = ndimage.label(mine & (levels == g), structure=full)
            records += [(l, int(g), int(s)) for s in np.bincount(lab.ravel())[1:]]
    if not records:
        return np.zeros((0, 4), dtype=np.int64)
    rows, count = np.unique(np.array(records, dtype=np.int64), axis=0, return_counts=True)
    return np.concatenate([rows, count[:, None]], axis=1).astype(np.int64)


def _neighbourhoods(row, level, L, G, alpha):
    """(gldm, ngtdm_n, ngtdm_s), each [L, G, 27]."""
    shape = row.shape
    m = np.zeros(shape, dtype=np.int64)
    total = np.zeros(shape, dtype=np.int64)
    alike = np.zeros(shape, dtype=np.int64)
    for delta in NEIGHBOURS:
        here, there = _shifted(shape, delta)
        same = (row[here] >= 0) & (row[here] == row[there])
        m[here] += same
        total[here] += np.where(same, level[there] + 1, 0)
        alike[here] += same & (np.abs(level[here] - level[there]) <= alpha)
    on = row >= 0
    rows, levels, m, total, alike = row[on], level[on], m[on], total[on], alike[on]
    gldm, ngtdm_n, ngtdm_s = (np.zeros((L, G, 27), dtype=np.int64) for _ in range(3))
    np.add.at(gldm, (rows, levels, alike), 1)
    np.add.at(ngtdm_n, (rows, levels, m), 1)
    np.add.at(ngtdm_s, (rows, levels, m), np.abs((levels + 1) * m - total))
    return gldm, ngtdm_n, ngtdm_s


def lesion_matrices(labels, image, region, connectivity=26, bins=32, bin_width=None, min_lesion_voxels=1,
                    dependence_alpha=0):
    """texture_ref.lesion_texture's dict with glrlm [L, 13, G, R], zones [K, 4], gldm, ngtdm_n and ngtdm_s
    [L, G, 27] (all int64) beside its keys."""
    labels, image = np.asarray(labels), np.asarray(image)
    table = texture_ref.lesion_texture(labels, image, region, connectivity, bins, bin_width, min_lesion_voxels)
    row, level, boxes, chosen = _volumes(labels, image, region, connectivity, bins, bin_width, min_lesion_voxels)
    L, G = len(chosen), table["hist"].shape[1]
    assert L == len(table["root"])
    gldm, ngtdm_n, ngtdm_s = _neighbourhoods(row, level, L, G, dependence_alpha)
    return dict(table, glrlm=_runs(row, level, L, G), zones=_zones(row, level, boxes, chosen), gldm=gldm,
                ngtdm_n=ngtdm_n, ngtdm_s=ngtdm_s)


def identities_hold(table):
    """The four sums that give back the histogram, for every lesion and level."""
    hist, glrlm = table["hist"], table["glrlm"]
    lengths = np.arange(1, glrlm.shape[3] + 1)
    by_zone = np.zeros_like(hist)
    np.add.at(by_zone, (table["zones"][:, 0], table["zones"][:, 1]), table["zones"][:, 2] * table["zones"][:, 3])
    return bool(((glrlm * lengths).sum(axis=3) == hist[:, None, :]).all() and (by_zone == hist).all() and
                (table["gldm"].sum(axis=2) == hist).all() and (table["ngtdm_n"].sum(axis=2) == hist).all())


# ------------------------------------------------------------------ the float features, exactly
def _matrix_features(cells, n, keys):
    """{key: (exact value, sum of |terms|)} of the count matrix {(i, j): count}, i the level from 1, j the run length,
    zone size or dependence, in the order of GLRLM_KEYS (the GLDM has no percentage and has an energy)."""
    N = sum(cells.values())
    p = {ij: Fraction(c, N) for ij, c in cells.items()}
    by_level, by_size = {}, {}
    for (i, j), c in cells.items():
        by_level[i] = by_level.get(i, 0) + c
        by_size[j] = by_size.get(j, 0) + c
    mu_i = sum(i * q for (i, j), q in p.items())
    mu_j = sum(j * q for (i, j), q in p.items())
    terms = [-(float(q) * math.log2(float(q))) for q in p.values()]
    values = [sum(Fraction(c, j * j) for j, c in by_size.items()) / N,
              sum(Fraction(j * j * c) for j, c in by_size.items()) / N,
              sum(Fraction(c, i * i) for i, c in by_level.items()) / N,
              sum(Fraction(i * i * c) for i, c in by_level.items()) / N,
              sum(Fraction(c, i * i * j * j) for (i, j), c in cells.items()) / N,
              sum(Fraction(i * i * c, j * j) for (i, j), c in cells.items()) / N,
              sum(Fraction(j * j * c, i * i) for (i, j), c in cells.items()) / N,
              sum(Fraction(i * i * j * j * c) for (i, j), c in cells.items()) / N,
              Fraction(sum(c * c for c in by_level.values()), N), Fraction(sum(c * c for c in by_level.values()), N * N),
              Fraction(sum(c * c for c in by_size.values()), N), Fraction(sum(c * c for c in by_size.values()), N * N),
              Fraction(N, n),
              sum((i - mu_i) ** 2 * q for (i, j), q in p.items()), sum((j - mu_j) ** 2 * q for (i, j), q in p.items()),
              None, sum(q * q for q in p.values())]
    out = {name: (v, v) for name, v in zip(keys[:12], values[:12])}        # every term is positive
    tail = dict(percentage=values[12], grey_level_variance=values[13], variance=values[14],
                entropy=(math.fsum(terms), math.fsum(abs(t) for t in terms)), energy=values[16])
    for name in keys[12:]:
        kind = next(k for k in ("percentage", "grey_level_variance", "variance", "entropy", "energy")
                    if name.endswith(k))
        out[name] = tail[kind] if kind == "entropy" else (tail[kind], tail[kind])
    return out


def _dense(matrix):
    return {(int(i) + 1, int(j) + 1): int(matrix[i, j]) for i, j in zip(*np.nonzero(matrix))}


def glrlm_features(table, k):
    """Per direction, then the mean over the 13 directions."""
    n_levels, n = int(table["levels"][k]), int(table["n"][k])
    per = [_matrix_features(_dense(m[:n_levels]), n, GLRLM_KEYS) for m in table["glrlm"][k]]
    return {key: tuple(sum(f[key][s] for f in per) / len(per) for s in (0, 1)) for key in GLRLM_KEYS}


def glszm_features(table, k):
    rows = table["zones"][table["zones"][:, 0] == k]
    return _matrix_features({(int(g) + 1, int(s)): int(c) for _, g, s, c in rows}, int(table["n"][k]), GLSZM_KEYS)


def gldm_features(table, k):
    n_levels = int(table["levels"][k])
    return _matrix_features(_dense(table["gldm"][k][:n_levels]), int(table["n"][k]), GLDM_KEYS)


def ngtdm_features(table, k):
    """{key: (value, sum of |terms|)}; None for a lesion none of whose voxels has a neighbour.  The stated values of
    the degenerate cases: coarseness 1e6 at sum p s = 0, contrast 0 at one level, busyness and strength 0 at a zero
    denominator."""
    n_levels = int(table["levels"][k])
    counts, sums = table["ngtdm_n"][k][:n_levels], table["ngtdm_s"][k][:n_levels]
    n_i = [int(counts[i, 1:].sum()) for i in range(n_levels)]
    N_v = sum(n_i)
    if N_v == 0:
        return None
    p = {i + 1: Fraction(n_i[i], N_v) for i in range(n_levels) if n_i[i]}
    s = {i: sum(Fraction(int(sums[i - 1, m]), m) for m in range(1, 27)) for i in p}
    ps, total, n_gp = sum(p[i] * s[i] for i in p), sum(s.values()), len(p)
    busy = sum(abs(i * p[i] - j * p[j]) for i in p for j in p)
    contrast = sum(p[i] * p[j] * (i - j) ** 2 for i in p for j in p) / (n_gp * (n_gp - 1)) * total / N_v \
        if n_gp > 1 else Fraction(0)
    out = dict(ngtdm_coarseness=1 / ps if ps else Fraction(10 ** 6), ngtdm_contrast=contrast,
               ngtdm_busyness=ps / busy if busy else Fraction(0),
               ngtdm_complexity=sum(abs(i - j) * (p[i] * s[i] + p[j] * s[j]) / (p[i] + p[j]) for i in p for j in p) / N_v,
               ngtdm_strength=sum((p[i] + p[j]) * (i - j) ** 2 for i in p for j in p) / total if total else Fraction(0))
    return {key: (value, value) for key, value in out.items()}         # every term is positive


# ------------------------------------------------------------------ the cases only these families need
def line_case(length=300):
    """A 1 x 1 x length lesion of one level: one run longer than a workgroup, one zone that is one chain."""
    return np.full((1, 1, length), 1, dtype=np.int16), np.full((1, 1, length), 5, dtype=np.int16)


def serpentine_case(shape=(12, 12, 3)):
    """One lesion filling the volume, at two levels: a one-voxel-wide path snakes along Y through every other row of
    the planes z = 0 and z = 2, turning at alternate ends, the two planes' paths joined by one voxel at z = 1; the
    rest is the other level.  Two zones; every voxel of the path is a Z line of its own."""
    labels = np.full(shape, 1, dtype=np.int16)
    image = np.zeros(shape, dtype=np.int16)
    X, Y, _ = shape
    for z in (0, 2):
        for x in range(0, X, 2):
            image[x, :, z] = 100
            if x + 1 < X:
                image[x + 1, (Y - 1) if (x // 2) % 2 == 0 else 0, z] = 100     # the turn into the next row
    image[0, 0, 1] = 100
    return labels, image


@functools.lru_cache(maxsize=None)
def cached_selection_matrices(index, connectivity, min_lesion_voxels):
    """lesion_matrices of a selection case of texture_ref (region WT, 32 bins, alpha 0), once per session."""
    _, labels, image = texture_ref.cached_selection()[index]
    return lesion_matrices(labels, image, "WT", connectivity, 32, None, min_lesion_voxels)
