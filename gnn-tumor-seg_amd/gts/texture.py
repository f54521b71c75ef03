"""What the tissue inside each lesion looks like on a scan: per lesion the range of the scan's values, the grey levels,
their histogram and the grey-level co-occurrence matrix (GLCM) over the 13 directions at distance 1, on the device
(X1-X3, csrc/gts_texture.hip; definitions: DESIGN.md 4aa), and the first-order and texture features derived from
them on the host.

A lesion is a connected component (connectivity 6 or 26) of a region's mask (WT, CT or ET), as in gts.measure; lesions
are listed by ascending root and only those of at least min_lesion_voxels voxels are selected and get rows.  Every
device quantity is an integer (or a value of the scan) equal to the numpy statement of its definition:

    lo, hi   the smallest and largest value over the lesion.  A float32 NaN or Inf inside a selected lesion is refused.
    levels   bins=N (default 32):  g = min(N - 1, floor((double(v) - lo) * double(N) / (hi - lo))), 0 when hi == lo;
             levels = N, or 1 when hi == lo.
             bin_width=w:  g = floor(double(v) / w) - floor(lo / w), levels = floor(hi / w) - floor(lo / w) + 1.
             More than MAX_LEVELS (128) levels are refused: widen the bins.
    hist     hist[l][g] = voxels of lesion l at level g.
    glcm     glcm[l][d][i][j] = ordered pairs (p, q), q = p +- DIRECTIONS[d], both of lesion l (the same root, not
             merely the same mask), g(p) = i and g(q) = j: symmetric, every unordered neighbouring pair twice.  Index
             space, distance 1; the voxel spacing is not used (as pyradiomics without resampling).

With matrices= the run-length, size-zone, dependence and neighbourhood-difference tables (GLRLM, GLSZM, GLDM, NGTDM)
are made as well, by X4-X6 (csrc/gts_texture_matrices.hip; definitions: DESIGN.md 4ab and lesion_texture's docstring).

The float64 features are derived on the host from the integer tables, each by one written expression (`derive`).
Everything runs on the current stream.
"""
import itertools
import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib, _volume
from ._lesions import RegionLesions, grid_arg, table_head
from ._lib import check, current_stream, ptr

MAX_LEVELS = _lib.const("GTS_TEXTURE_MAX_LEVELS")
CHUNK = _lib.const("GTS_TEXTURE_CHUNK")
HEAD_I64 = _lib.const("GTS_TEXTURE_HEAD_I64")
COUNT_ROW_I64 = _lib.const("GTS_TEXTURE_COUNT_ROW_I64")
RANGE_ROW_I64 = _lib.const("GTS_TEXTURE_RANGE_ROW_I64")
PLAN_I64 = _lib.const("GTS_TEXTURE_PLAN_I64")
MAX_TABLE_BYTES = _lib.const("GTS_TEXTURE_MAX_TABLE_BYTES")
DIRECTIONS = tuple(d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0))
LIMITS = "every extent in [1, 4097], fewer than 2^31 voxels"
TABLE_KEYS = ("root", "n", "lo", "hi", "levels", "hist", "glcm")
HIST_KEYS = ("min", "max", "range", "levels", "mean_level", "variance", "skewness", "kurtosis", "median_level",
             "p10_level", "p90_level", "mode_level", "entropy", "uniformity", "mean_intensity_approx")
GLCM_KEYS = ("joint_maximum", "joint_average", "joint_variance", "joint_entropy", "difference_average",
             "difference_variance", "difference_entropy", "sum_average", "sum_variance", "sum_entropy",
             "angular_second_moment", "contrast", "dissimilarity", "inverse_difference", "inverse_difference_moment",
             "correlation", "autocorrelation", "cluster_tendency", "cluster_shade", "cluster_prominence",
             "information_correlation_1", "information_correlation_2")
FEATURE_KEYS = HIST_KEYS + GLCM_KEYS
# the further families, asked for with matrices=; their features are not part of FEATURE_KEYS
MATRICES = ("glrlm", "glszm", "gldm", "ngtdm")
MATRIX_TABLE_KEYS = {"glrlm": ("glrlm",), "glszm": ("zones",), "gldm": ("gldm",), "ngtdm": ("ngtdm_n", "ngtdm_s")}
DEPENDENCES = _lib.const("GTS_TEXTURE_DEPENDENCES")
MAX_RUN = _lib.const("GTS_TEXTURE_MAX_RUN")
ZONE_RECORD_I32 = _lib.const("GTS_TEXTURE_ZONE_RECORD_I32")
_COMMON = ("grey_level_non_uniformity", "grey_level_non_uniformity_normalised")
GLRLM_KEYS = tuple("glrlm_" + key for key in (
    "short_runs_emphasis", "long_runs_emphasis", "low_grey_level_run_emphasis", "high_grey_level_run_emphasis",
    "short_run_low_grey_level_emphasis", "short_run_high_grey_level_emphasis", "long_run_low_grey_level_emphasis",
    "long_run_high_grey_level_emphasis") + _COMMON + (
    "run_length_non_uniformity", "run_length_non_uniformity_normalised", "run_percentage", "grey_level_variance",
    "run_length_variance", "run_entropy"))
GLSZM_KEYS = tuple("glszm_" + key for key in (
    "small_zone_emphasis", "large_zone_emphasis", "low_grey_level_zone_emphasis", "high_grey_level_zone_emphasis",
    "small_zone_low_grey_level_emphasis", "small_zone_high_grey_level_emphasis", "large_zone_low_grey_level_emphasis",
    "large_zone_high_grey_level_emphasis") + _COMMON + (
    "zone_size_non_uniformity", "zone_size_non_uniformity_normalised", "zone_percentage", "grey_level_variance",
    "zone_size_variance", "zone_size_entropy"))
GLDM_KEYS = tuple("gldm_" + key for key in (
    "low_dependence_emphasis", "high_dependence_emphasis", "low_grey_level_count_emphasis",
    "high_grey_level_count_emphasis", "low_dependence_low_grey_level_emphasis",
    "low_dependence_high_grey_level_emphasis", "high_dependence_low_grey_level_emphasis",
    "high_dependence_high_grey_level_emphasis") + _COMMON + (
    "dependence_count_non_uniformity", "dependence_count_non_uniformity_normalised", "grey_level_variance",
    "dependence_count_variance", "dependence_count_entropy", "dependence_count_energy"))
NGTDM_KEYS = ("ngtdm_coarseness", "ngtdm_contrast", "ngtdm_busyness", "ngtdm_complexity", "ngtdm_strength")
MATRIX_FEATURE_KEYS = {"glrlm": GLRLM_KEYS, "glszm": GLSZM_KEYS, "gldm": GLDM_KEYS, "ngtdm": NGTDM_KEYS}
_NUMPY = {torch.int16: np.int16, torch.float32: np.float32}

assert len(DIRECTIONS) == _lib.const("GTS_TEXTURE_DIRECTIONS")
assert DEPENDENCES == _lib.const("GTS_TEXTURE_NEIGHBOURS") + 1 == 27


def binning_args(bins, bin_width, what):
    """(bins, bin_width as the library takes them): a bin number in [1, MAX_LEVELS] and 0.0, or 0 and a positive
    finite width."""
    if bin_width is not None:
        if isinstance(bin_width, bool) or not isinstance(bin_width, (int, float)) or \
                not (math.isfinite(bin_width) and bin_width > 0):
            raise _lib.GtsError(f"{what}: bin_width {bin_width!r} (a positive finite number)")
        return 0, float(bin_width)
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= MAX_LEVELS:
        raise _lib.GtsError(f"{what}: bins {bins!r} (1 .. {MAX_LEVELS})")
    return bins, 0.0


def min_voxels_arg(min_lesion_voxels, what):
    if isinstance(min_lesion_voxels, bool) or not isinstance(min_lesion_voxels, int) or min_lesion_voxels < 1:
        raise _lib.GtsError(f"{what}: min_lesion_voxels {min_lesion_voxels!r} (1 or more)")
    return min_lesion_voxels


def image_arg(image, labels, what):
    """The scan's dtype code after the checks: int16 or float32, labels' shape and device, contiguous."""
    code = _volume.scan_volume(image, what)[0]
    if tuple(image.shape) != tuple(labels.shape):
        raise _lib.GtsError(f"{what}: the image's shape {tuple(image.shape)} is not the labels' {tuple(labels.shape)}")
    _lib.require_device(labels, image)
    return code


def table_words(lesions, levels, what="lesion_texture"):
    """int32 words of the device table of `lesions` lesions at `levels` levels: lesions x (levels + 13 levels (levels
    + 1) / 2); more than MAX_TABLE_BYTES is refused, not allocated."""
    words = int(_lib.load().gts_texture_table_words(lesions, levels))
    if words <= 0:
        raise _lib.GtsError(f"{what}: the tables of {lesions} lesions at {levels} levels exceed {MAX_TABLE_BYTES} "
                            f"bytes: raise min_lesion_voxels or widen the bins")
    return words


def matrices_arg(matrices, dependence_alpha, what):
    """(the families asked for in MATRICES' order, alpha) after the checks: names of MATRICES, an integer alpha >= 0
    (levels differ by less than MAX_LEVELS, so a larger alpha is passed on as MAX_LEVELS)."""
    if isinstance(matrices, str):
        matrices = (matrices,)
    matrices = tuple(matrices)
    unknown = [m for m in matrices if m not in MATRICES]
    if unknown:
        raise _lib.GtsError(f"{what}: matrices {unknown!r} (a subset of {MATRICES})")
    if isinstance(dependence_alpha, bool) or not isinstance(dependence_alpha, (int, np.integer)) or \
            dependence_alpha < 0:
        raise _lib.GtsError(f"{what}: dependence_alpha {dependence_alpha!r} (an integer, 0 or more)")
    return tuple(m for m in MATRICES if m in matrices), min(int(dependence_alpha), MAX_LEVELS)


def run_table_words(lesions, levels, longest, what="lesion_texture"):
    """int32 words of the device run table, lesions x 13 x levels x longest; more than MAX_TABLE_BYTES is refused,
    not allocated."""
    words = int(_lib.load().gts_texture_run_words(lesions, levels, longest))
    if words <= 0:
        raise _lib.GtsError(f"{what}: the run-length tables of {lesions} lesions at {levels} levels and runs of up to "
                            f"{longest} voxels exceed {MAX_TABLE_BYTES} bytes: raise min_lesion_voxels or widen the "
                            f"bins")
    return words


def chunk_units(n, chunk=CHUNK):
    """X6's plan: int32 [units, 2] of (lesion, chunk), every chunk of every lesion's list once."""
    chunks = -(-np.asarray(n, dtype=np.int64) // chunk)
    lesion = np.repeat(np.arange(len(chunks)), chunks)
    first = np.cumsum(chunks) - chunks
    return np.stack([lesion, np.arange(len(lesion)) - first[lesion]], axis=1).astype(np.int32).reshape(-1, 2)


def count_zones(records):
    """int64 [K, 4] rows (lesion, level, size, count), ascending, of X5's records [zones, 3] in any order."""
    records = np.asarray(records, dtype=np.int64).reshape(-1, ZONE_RECORD_I32)
    if not len(records):
        return np.zeros((0, 4), dtype=np.int64)
    rows, count = np.unique(records, axis=0, return_counts=True)
    return np.concatenate([rows, count[:, None].astype(np.int64)], axis=1)


def empty_matrices(matrices):
    """The tables of `matrices` for no lesion at all: empty arrays of the right rank."""
    shapes = dict(glrlm=(0, len(DIRECTIONS), 1, 1), zones=(0, 4), gldm=(0, 1, DEPENDENCES),
                  ngtdm_n=(0, 1, DEPENDENCES), ngtdm_s=(0, 1, DEPENDENCES))
    return {key: np.zeros(shapes[key], dtype=np.int64) for m in matrices for key in MATRIX_TABLE_KEYS[m]}


def level_counts(lo, hi, bins, bin_width):
    """`levels` per lesion from float64 lo and hi, the expressions of the module's docstring."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if bin_width > 0.0:
        return (np.floor(hi / bin_width) - np.floor(lo / bin_width)).astype(np.int64) + 1
    return np.where(hi == lo, 1, bins).astype(np.int64)


def work_units(n, chunk=CHUNK):
    """X3's plan: int32 [units, 3] of (lesion, direction, chunk), every chunk of every lesion's list once per
    direction."""
    chunks = -(-np.asarray(n, dtype=np.int64) // chunk)
    lesion = np.repeat(np.arange(len(chunks)), chunks)
    first = np.cumsum(chunks) - chunks
    part = np.arange(len(lesion)) - first[lesion]
    units = np.stack([np.repeat(lesion, len(DIRECTIONS)), np.tile(np.arange(len(DIRECTIONS)), len(lesion)),
                      np.repeat(part, len(DIRECTIONS))], axis=1)
    return units.astype(np.int32).reshape(-1, 3)


def decode_range(words, dtype):
    """The values of X1's encoded lo / hi words (int64 array) as the image's dtype."""
    words = np.asarray(words, dtype=np.int64)
    if dtype == torch.int16:
        return (words - 32768).astype(np.int16)
    bits = words.astype(np.uint32)
    bits = np.where(bits & np.uint32(0x80000000), bits & np.uint32(0x7FFFFFFF), ~bits)
    return bits.astype(np.uint32).view(np.float32)


def unfold(folded, levels):
    """The dense symmetric int64 [.., G, G] of folded triangles [.., G (G + 1) / 2]: the entry of (i, j), i <= j, is
    j (j + 1) / 2 + i; the diagonal counts twice."""
    i, j = np.triu_indices(levels)
    dense = np.zeros(folded.shape[:-1] + (levels, levels), dtype=np.int64)
    dense[..., i, j] = folded[..., j * (j + 1) // 2 + i]
    dense[..., j, i] += folded[..., j * (j + 1) // 2 + i]
    return dense


def lesion_texture(labels, image, region, connectivity=26, *, bins=32, bin_width=None, min_lesion_voxels=1,
                   grid_blocks=0, mark=None, matrices=(), dependence_alpha=0):
    """The integer tables of one region's selected lesions on one scan: a dict of numpy arrays in lesion order
    (ascending root): root, n [L] int64, lo, hi [L] (the image's dtype), levels [L] int64, hist [L, G] int64 and
    glcm [L, 13, G, G] int64 (symmetric, DIRECTIONS' order), G the largest `levels`; `bins` and `bin_width` as given.

    labels: int16 CUDA tensor [X, Y, Z] of internal labels; image: int16 or float32 CUDA tensor of the same shape;
    region "WT", "CT" or "ET" (or 0..2).  Two small copies come to the host for the plan (the lesions' sizes, their
    ranges) and one for the results.  grid_blocks: workgroups of every pass (0: the library's choice); no value
    depends on it.  mark: called with a stage's name once the stage is enqueued.

    matrices: a subset of MATRICES; the dict then also carries (X4-X6; all int64, every other key being
    what the call returns without them), the 26-neighbourhood of p being the voxels p + delta, delta in {-1, 0, 1}^3
    without 0, inside the volume and of p's root:

        "glrlm"   glrlm [L, 13, G, R]: glrlm[l][d][g][r - 1] = the runs of lesion l along DIRECTIONS[d] at level g of
                  length r (maximal sets p, p + delta, .. of the lesion's voxels at one level); R the longest run.
        "glszm"   zones [K, 4]: rows (lesion, level, size, count), ascending, one per distinct (lesion, level, size); a
                  zone is a 26-connected set of voxels of one lesion at one level, whatever connectivity formed the
                  lesions.
        "gldm"    gldm [L, G, 27]: gldm[l][g][k - 1] = the voxels at level g with dependence k = 1 + the neighbours q
                  with |g(p) - g(q)| <= dependence_alpha (an integer >= 0).
        "ngtdm"   ngtdm_n, ngtdm_s [L, G, 27]: the voxels at level g with m neighbours, and over them the sum of
                  |(g + 1) m - S(p)|, S(p) the sum of g(q) + 1 over the neighbours.  Column 0 holds counts only.

    For these one more small copy (the longest run, the number of zones) comes to the host per family."""
    what = "lesion_texture"
    grid_blocks = grid_arg(grid_blocks, what)
    bins_c, width_c = binning_args(bins, bin_width, what)
    min_voxels_arg(min_lesion_voxels, what)
    matrices, alpha = matrices_arg(matrices, dependence_alpha, what)
    front = RegionLesions(labels, region, (1, 1, 1), connectivity, what, LIMITS, mark)
    return _texture(front, image, bins_c, width_c, min_lesion_voxels, grid_blocks, matrices, alpha)


def _matrices(front, matrices, alpha, state, grid_blocks):
    """X4-X6 on what X1-X3 left on the device (`state`): {key: int64 array} of the families of `matrices`."""
    what = "lesion_texture"
    lib, roots, (x, y, z), mark, stream = front.lib, front.roots, front.shape, front.mark, current_stream()
    L, G, n_listed, dev = state["L"], state["G"], state["n_listed"], roots.device
    seg, plan, listed, levels = state["segments"], state["plan"], state["list"], state["levels"]
    workspace, size = state["workspace"]
    out = {}
    if "glrlm" in matrices:
        run_table_words(L, G, 1, what)                                 # the smallest table these lesions can take
        lengths = torch.empty(len(DIRECTIONS) * n_listed, dtype=torch.int16, device=dev)      # uint16 on the device
        head = torch.empty(HEAD_I64, dtype=torch.int64, device=dev)
        units = state["units"]
        check(lib.gts_texture_run_lengths(ptr(roots), x, y, z, ptr(units), len(units), ptr(seg), ptr(plan), L,
                                          ptr(listed), ptr(levels), n_listed, ptr(lengths), lengths.numel(), ptr(head),
                                          ptr(workspace), size, grid_blocks, stream), "gts_texture_run_lengths")
        mark("X4 run lengths")
        longest = int(head[0].item())
        if not 1 <= longest <= MAX_RUN:
            raise _lib.GtsError(f"{what}: the longest run is {longest} voxels (1 .. {MAX_RUN})")
        words = run_table_words(L, G, longest, what)
        table = torch.empty(words, dtype=torch.int32, device=dev)
        check(lib.gts_texture_runs(ptr(units), len(units), ptr(seg), ptr(plan), L, ptr(levels), ptr(lengths),
                                   n_listed, ptr(table), words, G, longest, grid_blocks, stream), "gts_texture_runs")
        mark("X4 run counts")
        out["glrlm"] = table
    if "glszm" in matrices:
        scratch = torch.empty(2 * x * y * z, dtype=torch.int32, device=dev)
        records = torch.empty(ZONE_RECORD_I32 * n_listed, dtype=torch.int32, device=dev)
        head = torch.empty(HEAD_I64, dtype=torch.int64, device=dev)
        check(lib.gts_texture_zones(ptr(roots), x, y, z, ptr(seg), ptr(plan), L, ptr(listed), ptr(levels), n_listed,
                                    ptr(scratch), scratch.numel(), ptr(records), records.numel(), ptr(head),
                                    ptr(workspace), size, grid_blocks, stream), "gts_texture_zones")
        mark("X5 zones")
        zones, lost = (int(v) for v in head[:2].cpu())
        if lost or not 1 <= zones <= n_listed:
            raise _lib.GtsError(f"{what}: the zones' union-find did not close ({lost} searches passed {n_listed} "
                                f"steps, {zones} zones of {n_listed} voxels)")
        out["zones"] = records[:ZONE_RECORD_I32 * zones]
    if "gldm" in matrices or "ngtdm" in matrices:
        entries = int(lib.gts_texture_neighbourhood_i64s(L, G))
        if entries <= 0:
            raise _lib.GtsError(f"{what}: the neighbourhood tables of {L} lesions at {G} levels exceed "
                                f"{MAX_TABLE_BYTES} bytes: raise min_lesion_voxels or widen the bins")
        units = torch.from_numpy(chunk_units(state["n"])).to(dev)
        table = torch.empty(entries, dtype=torch.int64, device=dev)
        check(lib.gts_texture_neighbourhood(ptr(roots), x, y, z, ptr(units), len(units), ptr(seg), ptr(plan), L,
                                            ptr(listed), ptr(levels), n_listed, alpha, ptr(table), entries, G,
                                            ptr(workspace), size, grid_blocks, stream), "gts_texture_neighbourhood")
        mark("X6 neighbourhood")
        out["neighbourhood"] = table
    host = {key: value.cpu().numpy() for key, value in out.items()}
    mark("matrices (copy)")
    result = {}
    if "glrlm" in host:
        result["glrlm"] = host["glrlm"].astype(np.int64).reshape(L, len(DIRECTIONS), G, -1)
    if "zones" in host:
        result["zones"] = count_zones(host["zones"])
    if "neighbourhood" in host:
        gldm, ngtdm_n, ngtdm_s = host["neighbourhood"].reshape(3, L, G, DEPENDENCES)
        if "gldm" in matrices:
            result["gldm"] = gldm
        if "ngtdm" in matrices:
            result["ngtdm_n"], result["ngtdm_s"] = ngtdm_n, ngtdm_s
    return result


def _texture(front, image, bins, bin_width, min_lesion_voxels=1, grid_blocks=0, matrices=(), alpha=0):
    """lesion_texture's own stages, X1-X3 and for `matrices` X4-X6, on a front end; bins and bin_width as
    binning_args gives them, matrices and alpha as matrices_arg does."""
    what = "lesion_texture"
    lib, labels, roots, (x, y, z), mark = front.lib, front.labels, front.roots, front.shape, front.mark
    code, dev, stream = image_arg(image, labels, what), labels.device, current_stream()
    image = image.contiguous()
    workspace, size = _volume.workspace(lib.gts_texture_workspace, x, y, z, dev, what, LIMITS)
    ints = lib.gts_texture_count_i64s(x, y, z, front.connectivity)
    counts = torch.empty(ints, dtype=torch.int64, device=dev)
    check(lib.gts_texture_counts(ptr(roots), x, y, z, front.connectivity, ptr(counts), ints, ptr(workspace), size,
                                 grid_blocks, stream), "gts_texture_counts")
    mark("X1 counts")
    head = table_head(counts, lambda head: HEAD_I64 + COUNT_ROW_I64 * int(head[0]))
    rows = head[HEAD_I64:].reshape(-1, COUNT_ROW_I64)
    chosen = np.flatnonzero(rows[:, 1] >= min_lesion_voxels)
    chosen = chosen[np.argsort(rows[chosen, 0])]                       # lesion order: ascending root
    root, n = rows[chosen, 0].copy(), rows[chosen, 1].copy()
    L = len(chosen)
    if L == 0:      # nothing to report: nothing more is launched
        return dict(root=root, n=n, lo=np.zeros(0, _NUMPY[image.dtype]), hi=np.zeros(0, _NUMPY[image.dtype]),
                    levels=np.zeros(0, np.int64), hist=np.zeros((0, 1), np.int64),
                    glcm=np.zeros((0, len(DIRECTIONS), 1, 1), np.int64), bins=bins or None,
                    bin_width=bin_width or None, **empty_matrices(matrices))
    table_words(L, 1, what)                                            # the smallest table these lesions can take
    select = np.full(len(rows), -1, dtype=np.int32)
    select[chosen] = np.arange(L, dtype=np.int32)
    segments = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    n_listed = int(segments[-1])
    plan_dev = torch.from_numpy(np.concatenate([select, segments])).to(dev)
    select_dev, segments_dev = plan_dev[:len(rows)], plan_dev[len(rows):]
    ranges = torch.empty(HEAD_I64 + RANGE_ROW_I64 * L, dtype=torch.int64, device=dev)
    listed = torch.empty(n_listed, dtype=torch.int32, device=dev)
    check(lib.gts_texture_ranges(ptr(roots), ptr(image), code, x, y, z, ptr(select_dev), len(rows), ptr(segments_dev),
                                 L, ptr(ranges), ranges.numel(), ptr(listed), n_listed, ptr(workspace), size,
                                 grid_blocks, stream), "gts_texture_ranges")
    mark("X1 ranges, lists")
    head = table_head(ranges, lambda head: ranges.numel())
    spans = head[HEAD_I64:].reshape(L, RANGE_ROW_I64)
    if int(head[0]):
        bad = np.flatnonzero(spans[:, 3])
        raise _lib.GtsError(f"{what}: {int(head[0])} NaN or Inf voxel(s) inside the lesion(s) of root "
                            f"{', '.join(str(int(r)) for r in root[bad])}: mask or repair the scan first")
    if not np.array_equal(spans[:, 2], segments[1:]):
        raise _lib.GtsError(f"{what}: the lists of the lesions do not match their sizes")
    lo, hi = decode_range(spans[:, 0], image.dtype), decode_range(spans[:, 1], image.dtype)
    levels = level_counts(lo, hi, bins, bin_width)
    if int(levels.max()) > MAX_LEVELS:
        k = int(np.argmax(levels))
        raise _lib.GtsError(f"{what}: the lesion of root {int(root[k])} spans {int(levels[k])} levels at bin_width "
                            f"{bin_width!r}, more than {MAX_LEVELS}: widen the bins")
    G = int(levels.max())
    words = table_words(L, G, what)
    plan = np.empty((L, PLAN_I64), dtype=np.int64)
    plan[:, 0] = lo.astype(np.float64).view(np.int64)
    plan[:, 1] = hi.astype(np.float64).view(np.int64)
    plan[:, 2], plan[:, 3] = levels, root
    units = work_units(n)
    plan_dev = torch.from_numpy(plan).to(dev)
    units_dev = torch.from_numpy(units).to(dev)
    level_list = torch.empty(n_listed, dtype=torch.uint8, device=dev)
    table = torch.empty(words, dtype=torch.int32, device=dev)
    mark("plan (copy, host, upload)")
    check(lib.gts_texture_levels(ptr(image), code, x, y, z, bins, bin_width, ptr(segments_dev), ptr(plan_dev), L,
                                 ptr(listed), n_listed, ptr(level_list), ptr(table), words, G, ptr(workspace), size,
                                 grid_blocks, stream), "gts_texture_levels")
    mark("X2 levels, histogram")
    check(lib.gts_texture_glcm(ptr(roots), x, y, z, ptr(units_dev), len(units), ptr(segments_dev), ptr(plan_dev), L,
                               ptr(listed), ptr(level_list), n_listed, ptr(table), words, G, ptr(workspace), size,
                               grid_blocks, stream), "gts_texture_glcm")
    mark("X3 co-occurrence")
    host = table.cpu().numpy().astype(np.int64)
    mark("results (copy)")
    hist = host[:L * G].reshape(L, G)
    folded = host[L * G:].reshape(L, len(DIRECTIONS), G * (G + 1) // 2)
    more = {}
    if matrices:
        state = dict(L=L, G=G, n=n, n_listed=n_listed, segments=segments_dev, plan=plan_dev, list=listed,
                     levels=level_list, units=units_dev, workspace=(workspace, size))
        more = _matrices(front, matrices, alpha, state, grid_blocks)
    return dict(root=root, n=n, lo=lo, hi=hi, levels=levels, hist=hist, glcm=unfold(folded, G), bins=bins or None,
                bin_width=bin_width or None, **more)


# ------------------------------------------------------------------ the float features
def _entropy(counts, total):
    """-sum p log2 p over the counts that are not zero, p = c / total, by math.fsum."""
    return math.fsum(-((c / total) * math.log2(c / total)) for c in counts if c)


def _histogram_features(table, k):
    n_levels, n = int(table["levels"][k]), int(table["n"][k])
    c = [int(v) for v in table["hist"][k][:n_levels]]
    lo, hi = float(table["lo"][k]), float(table["hi"][k])
    s1 = sum(i * v for i, v in enumerate(c, 1))
    a = {r: sum((n * i - s1) ** r * v for i, v in enumerate(c, 1)) for r in (2, 3, 4)}   # n^(r+1) x the r-th moment
    cumulative = list(itertools.accumulate(c))

    def reach(num, den):
        return next(i for i, total in enumerate(cumulative, 1) if total * den >= n * num)

    mean = s1 / n
    if table["bin_width"] is not None:
        centre = (math.floor(lo / table["bin_width"]) + mean - 0.5) * table["bin_width"]
    else:
        centre = lo + (mean - 0.5) * ((hi - lo) / table["bins"]) if hi != lo else lo
    return dict(min=table["lo"][k].item(), max=table["hi"][k].item(), range=hi - lo, levels=n_levels, mean_level=mean,
                variance=a[2] / n ** 3,
                skewness=(a[3] / n ** 4) / math.pow(a[2] / n ** 3, 1.5) if a[2] else 0.0,
                kurtosis=(a[4] * n) / (a[2] * a[2]) - 3.0 if a[2] else 0.0,
                median_level=reach(1, 2), p10_level=reach(1, 10), p90_level=reach(9, 10),
                mode_level=1 + c.index(max(c)), entropy=_entropy(c, n),
                uniformity=sum(v * v for v in c) / (n * n), mean_intensity_approx=centre)


def _direction_features(matrix):
    """The GLCM family of one direction's symmetric count matrix (at least one pair), levels numbered from 1."""
    i, j = np.nonzero(matrix)
    cells = [(int(a) + 1, int(b) + 1, int(matrix[a, b])) for a, b in zip(i, j)]
    N = sum(c for _, _, c in cells)
    row, diff, plus = {}, {}, {}
    for a, b, c in cells:
        row[a] = row.get(a, 0) + c
        diff[abs(a - b)] = diff.get(abs(a - b), 0) + c
        plus[a + b] = plus.get(a + b, 0) + c
    s1 = sum(a * c for a, c in row.items())
    s2 = sum(a * a * c for a, c in row.items())
    sij = sum(a * b * c for a, b, c in cells)
    d1, d2 = sum(k * c for k, c in diff.items()), sum(k * k * c for k, c in diff.items())
    p1, p2 = sum(k * c for k, c in plus.items()), sum(k * k * c for k, c in plus.items())
    var_n2 = N * s2 - s1 * s1                                    # N^2 x the joint variance
    hxy, hx = _entropy([c for _, _, c in cells], N), _entropy(row.values(), N)
    hxy1 = math.fsum(-((c / N) * math.log2((row[a] / N) * (row[b] / N))) for a, b, c in cells)
    hxy2 = math.fsum(-(((ra * rb) / (N * N)) * math.log2((ra / N) * (rb / N))) for ra in row.values()
                     for rb in row.values())
    gap = hxy2 - hxy
    return dict(joint_maximum=max(c for _, _, c in cells) / N, joint_average=s1 / N, joint_variance=var_n2 / (N * N),
                joint_entropy=hxy, difference_average=d1 / N, difference_variance=(N * d2 - d1 * d1) / (N * N),
                difference_entropy=_entropy(diff.values(), N), sum_average=p1 / N,
                sum_variance=(N * p2 - p1 * p1) / (N * N), sum_entropy=_entropy(plus.values(), N),
                angular_second_moment=sum(c * c for _, _, c in cells) / (N * N), contrast=d2 / N,
                dissimilarity=d1 / N,
                inverse_difference=float(sum(Fraction(c, 1 + k) for k, c in diff.items()) / N),
                inverse_difference_moment=float(sum(Fraction(c, 1 + k * k) for k, c in diff.items()) / N),
                correlation=(N * sij - s1 * s1) / var_n2 if var_n2 else 1.0, autocorrelation=sij / N,
                cluster_tendency=sum((N * k - 2 * s1) ** 2 * c for k, c in plus.items()) / N ** 3,
                cluster_shade=sum((N * k - 2 * s1) ** 3 * c for k, c in plus.items()) / N ** 4,
                cluster_prominence=sum((N * k - 2 * s1) ** 4 * c for k, c in plus.items()) / N ** 5,
                information_correlation_1=(hxy - hxy1) / hx if hx > 0.0 else 0.0,
                information_correlation_2=math.sqrt(1.0 - math.exp(-2.0 * gap)) if gap > 0.0 else 0.0)


_SIZE_MATRIX_FIELDS = ("short", "long", "low", "high", "short_low", "short_high", "long_low", "long_high", "glnu",
                       "glnu_normalised", "snu", "snu_normalised", "percentage", "gl_variance", "size_variance",
                       "entropy", "energy")
_FAMILY_FIELDS = {"glrlm": _SIZE_MATRIX_FIELDS[:16], "glszm": _SIZE_MATRIX_FIELDS[:16],
                  "gldm": _SIZE_MATRIX_FIELDS[:12] + _SIZE_MATRIX_FIELDS[13:]}
_LCM_26 = math.lcm(*range(1, DEPENDENCES))       # every s_i = sum_m ngtdm_s[i][m] / m is a multiple of 1 / _LCM_26


def _size_matrix_features(cells, n):
    """{field of _SIZE_MATRIX_FIELDS: exact Fraction, `entropy` a float} of one count matrix given as its cells
    [(i, j, count)] that are not zero, i the level from 1, j the run length, zone size or dependence; n the lesion's
    voxels.  Sums are exact integers (the terms in 1 / i^2 over the common denominator lcm(i)^2), so a caller rounds
    once."""
    N = sum(c for _, _, c in cells)
    scale = math.lcm(*{i for i, _, _ in cells}) ** 2
    by_size, by_level = {}, {}
    for i, j, c in cells:
        count, low, high = by_size.get(j, (0, 0, 0))
        by_size[j] = (count + c, low + c * (scale // (i * i)), high + c * i * i)
        by_level[i] = by_level.get(i, 0) + c
    low = sum(v[1] for v in by_size.values())
    high = sum(v[2] for v in by_size.values())
    s1, s2 = sum(i * c for i, c in by_level.items()), sum(i * i * c for i, c in by_level.items())
    t1 = sum(j * v[0] for j, v in by_size.items())
    t2 = sum(j * j * v[0] for j, v in by_size.items())
    glnu, snu = sum(c * c for c in by_level.values()), sum(v[0] ** 2 for v in by_size.values())
    return dict(short=sum(Fraction(v[0], j * j) for j, v in by_size.items()) / N, long=Fraction(t2, N),
                low=Fraction(low, scale * N), high=Fraction(high, N),
                short_low=sum(Fraction(v[1], j * j) for j, v in by_size.items()) / (scale * N),
                short_high=sum(Fraction(v[2], j * j) for j, v in by_size.items()) / N,
                long_low=Fraction(sum(j * j * v[1] for j, v in by_size.items()), scale * N),
                long_high=Fraction(sum(j * j * v[2] for j, v in by_size.items()), N),
                glnu=Fraction(glnu, N), glnu_normalised=Fraction(glnu, N * N), snu=Fraction(snu, N),
                snu_normalised=Fraction(snu, N * N), percentage=Fraction(N, n),
                gl_variance=Fraction(N * s2 - s1 * s1, N * N), size_variance=Fraction(N * t2 - t1 * t1, N * N),
                entropy=_entropy([c for _, _, c in cells], N), energy=Fraction(sum(c * c for _, _, c in cells), N * N))


def _dense_cells(matrix):
    """[(level from 1, column from 1, count)] of the entries of an integer matrix [levels, columns] that are not 0."""
    i, j = np.nonzero(matrix)
    return [(int(a) + 1, int(b) + 1, int(matrix[a, b])) for a, b in zip(i, j)]


def _family_features(family, matrices, n):
    """{key: float} of MATRIX_FEATURE_KEYS[family] from the cells of one matrix, or of one per direction (glrlm): each
    rational feature is summed exactly over the directions and rounded once, an entropy is the math.fsum of the
    directions' entropies over their number."""
    per = [_size_matrix_features(cells, n) for cells in matrices]
    out = {}
    for key, field in zip(MATRIX_FEATURE_KEYS[family], _FAMILY_FIELDS[family]):
        if field == "entropy":
            out[key] = math.fsum(f[field] for f in per) / len(per)
        else:
            out[key] = float(sum(f[field] for f in per) / len(per))
    return out


def _ngtdm_features(counts, sums):
    """NGTDM_KEYS of one lesion's ngtdm_n and ngtdm_s [levels, 27]; exact integers over the common denominator of the
    1 / m, each feature rounded once."""
    n_i = {i: int(row[1:].sum()) for i, row in enumerate(counts, 1) if row[1:].any()}
    N_v = sum(n_i.values())
    if N_v == 0:
        return dict.fromkeys(NGTDM_KEYS)
    s_i = {i: sum(int(sums[i - 1][m]) * (_LCM_26 // m) for m in range(1, DEPENDENCES)) for i in n_i}   # x _LCM_26
    ps, s = sum(n_i[i] * s_i[i] for i in n_i), sum(s_i.values())             # x N_v _LCM_26, x _LCM_26
    pairs = [(i, j) for i in n_i for j in n_i]
    n_gp = len(n_i)
    spread = sum(n_i[i] * n_i[j] * (i - j) ** 2 for i, j in pairs)          # x N_v^2
    busy = sum(abs(i * n_i[i] - j * n_i[j]) for i, j in pairs)              # x N_v
    by_den = {}
    for i, j in pairs:
        if i != j:
            den = n_i[i] + n_i[j]
            by_den[den] = by_den.get(den, 0) + abs(i - j) * (n_i[i] * s_i[i] + n_i[j] * s_i[j])
    complexity = sum(Fraction(num, den) for den, num in by_den.items()) / (_LCM_26 * N_v)
    strength = sum((n_i[i] + n_i[j]) * (i - j) ** 2 for i, j in pairs)      # x N_v
    return dict(ngtdm_coarseness=float(Fraction(N_v * _LCM_26, ps)) if ps else 1e6,
                ngtdm_contrast=float(Fraction(spread * s, N_v ** 3 * _LCM_26 * n_gp * (n_gp - 1))) if n_gp > 1 else 0.0,
                ngtdm_busyness=float(Fraction(ps, _LCM_26 * busy)) if busy else 0.0,
                ngtdm_complexity=float(complexity),
                ngtdm_strength=float(Fraction(strength * _LCM_26, N_v * s)) if s else 0.0)


def _matrix_features(table, k):
    """The features of whichever of glrlm, zones, gldm, ngtdm_n / ngtdm_s `table` holds, for lesion k."""
    n_levels, n = int(table["levels"][k]), int(table["n"][k])
    out = {}
    if "glrlm" in table:
        out.update(_family_features("glrlm", [_dense_cells(m[:n_levels]) for m in table["glrlm"][k]], n))
    if "zones" in table:
        rows = table["zones"][table["zones"][:, 0] == k]
        out.update(_family_features("glszm", [[(int(g) + 1, int(s), int(c)) for _, g, s, c in rows]], n))
    if "gldm" in table:
        out.update(_family_features("gldm", [_dense_cells(table["gldm"][k][:n_levels])], n))
    if "ngtdm_n" in table:
        out.update(_ngtdm_features(table["ngtdm_n"][k][:n_levels], table["ngtdm_s"][k][:n_levels]))
    return out


def derive(table, k):
    """The float64 features of lesion k of a lesion_texture, each one fixed expression; sums of integers are exact
    Python integers, so a rational feature is rounded once or twice, and an entropy is a math.fsum of its rounded
    terms.  Levels are numbered from 1 (IBSI's discretised intensities): level = g + 1.  With c the histogram, n its
    sum and m_r = sum (level - mean)^r c / n:

        min, max, range      lo, hi, float(hi) - float(lo)            levels   the lesion's number of levels
        mean_level           sum level c / n                          variance m_2
        skewness             m_3 / m_2^1.5 (0.0 at m_2 = 0)           kurtosis m_4 / m_2^2 - 3 (0.0 at m_2 = 0)
        median_level, p10_level, p90_level   the smallest level whose cumulative count reaches n / 2, n / 10, 9 n / 10
        mode_level           the fullest level, the smallest on ties
        entropy              -sum p log2 p, p = c / n                 uniformity   sum p^2
        mean_intensity_approx   the centre of mean_level's bin mapped back to the scan's values, lo + (mean_level -
                             0.5) (hi - lo) / N (lo at hi == lo), or (floor(lo / w) + mean_level - 0.5) w: approximate
                             to half a bin

    and the GLCM family (GLCM_KEYS, IBSI's names): per direction on the matrix divided by its sum P, with the marginal
    p_x, the difference distribution p_(x-y)(k) over k = |i - j| and the sum distribution p_(x+y)(k) over k = i + j,
    mu = sum i p_x(i), then the mean over the directions that hold at least one pair (pyradiomics' default, IBSI
    "averaged"); every key is None for a lesion with no pair in any direction (a lone voxel).  Degenerate cases:
    correlation is 1.0 when the joint variance is 0 (one level; pyradiomics); information_correlation_1 is 0.0 when
    the marginal entropy is 0; information_correlation_2 is 0.0 when HXY2 - HXY is not positive.

    A table made with matrices= also gives the features of the families it holds, under GLRLM_KEYS,
    GLSZM_KEYS, GLDM_KEYS and NGTDM_KEYS; a table without them gives exactly the keys above.  For GLRLM, GLSZM and
    GLDM, with M[i][j] the counts (i the level, j the run length, zone size or dependence), N_s their sum, m_i. and
    m_.j the marginal sums, p = M / N_s and n the lesion's voxels:

        short_runs / small_zone / low_dependence emphasis   sum_j m_.j / j^2 / N_s      long / large / high: j^2
        low / high grey_level (run, zone, count) emphasis   sum_i m_i. / i^2 / N_s      and i^2
        short_low, short_high, long_low, long_high          sum M / (i^2 j^2) / N_s, i^2 / j^2, j^2 / i^2, i^2 j^2
        grey_level_non_uniformity (_normalised)             sum_i m_i.^2 / N_s (/ N_s^2)
        run_length / zone_size / dependence_count non_uniformity (_normalised)   sum_j m_.j^2 / N_s (/ N_s^2)
        run_percentage, zone_percentage                     N_s / n (GLDM has none: it is 1)
        grey_level_variance, run_length / zone_size / dependence_count variance  those of p's marginals
        run / zone_size / dependence_count entropy          -sum p log2 p
        gldm_dependence_count_energy                        sum p^2

    each an exact rational rounded once, the entropy a math.fsum of rounded terms.  The GLRLM features are the mean
    over the 13 directions, every one of which holds a run.  For NGTDM, with n_i the voxels of level i that have a
    neighbour, N_v their sum, p_i = n_i / N_v, s_i = sum_m ngtdm_s[i][m] / m, N_gp the levels with p_i > 0, and
    double sums over those levels:

        ngtdm_coarseness   1 / sum p_i s_i                  ngtdm_busyness   sum p_i s_i / sum sum |i p_i - j p_j|
        ngtdm_contrast     [sum sum p_i p_j (i - j)^2 / (N_gp (N_gp - 1))] [sum s_i / N_v]
        ngtdm_complexity   sum sum |i - j| (p_i s_i + p_j s_j) / (p_i + p_j) / N_v
        ngtdm_strength     sum sum (p_i + p_j) (i - j)^2 / sum s_i

    Degenerate cases: all five are None when N_v = 0 (a lone voxel); coarseness is 1e6 when sum p_i s_i = 0
    (pyradiomics' value); contrast is 0.0 at N_gp = 1; busyness and strength are 0.0 when their denominator is 0."""
    out = dict(root=int(table["root"][k]), n=int(table["n"][k]), **_histogram_features(table, k))
    n_levels = int(table["levels"][k])
    per = [_direction_features(m[:n_levels, :n_levels]) for m in table["glcm"][k] if m.any()]
    for key in GLCM_KEYS:
        out[key] = sum(f[key] for f in per) / len(per) if per else None
    out.update(_matrix_features(table, k))
    return out


def texture_features(labels, image, region, connectivity=26, *, bins=32, bin_width=None, min_lesion_voxels=1,
                     grid_blocks=0, matrices=(), dependence_alpha=0):
    """lesion_texture's lesions as a list of dicts in lesion order, each with the features of `derive`."""
    table = lesion_texture(labels, image, region, connectivity, bins=bins, bin_width=bin_width,
                           min_lesion_voxels=min_lesion_voxels, grid_blocks=grid_blocks, matrices=matrices,
                           dependence_alpha=dependence_alpha)
    return [derive(table, k) for k in range(len(table["root"]))]
