"""The exact integer reference of the HD95 / surface-distance kernels (H1-H5 and H3w-H5w of csrc/gts_hd95.hip),
every stage from its definition in numpy integers: no scipy, no float before the two ranks' `(n - 1) * 0.95`.

  border bits   the border rule on the lifted [X, Y, Z] volume and the WT / CT / ET region rule;
  g1            the 1-D index distance along Z to the nearest border voxel of a channel, 0xFFFF without one;
  g2            min over the (y, z) plane of uz^2 dz^2 + uy^2 dy^2, the kernels' infinity for an empty plane;
  D2            min over the opposite side's border of sum_a u_a^2 (p_a - q_a)^2, by brute force over a
                |A| x |B| table; units (1, 1, 1) is the voxel path;
  the rest      the per-region multiset, n, the two ranks, the order statistics, the presence bits, the counts
                of D2 <= T, and the byte layout of both workspaces (Hd95Layout / SurfaceLayout restated once).

The second half holds the designed inputs of tests/test_gpu_hd95_edges.py, so that tests/test_hd95_ref_host.py can
assert on this reference alone that each of them still hits the edge it was designed for.

Channels: bit c of a border byte is B(region c % 3, side c // 3), regions WT / CT / ET, sides pred / truth.
"""
import math
from collections import namedtuple

import numpy as np

REGIONS = ("WT", "CT", "ET")
CHANNELS = 6
INF16, INF32, INF64 = 0xFFFF, 0x7FFFFFFF, (1 << 63) - 1
LIMIT = 1 << 62                     # every int64 quantity of the kernels stays below this (the admission bound)


# ---------------------------------------------------------------------------------------------- shapes, borders
def lift(shape):
    """(X, Y, Z, all_border): axes of extent 1 dropped, the rest right-aligned in 3-D; a unit axis makes scipy's
    erosion remove every voxel, so every region voxel is then border."""
    shape = tuple(int(s) for s in shape) or (1,)
    long_axes = [s for s in shape if s != 1]
    assert len(long_axes) <= 3
    x, y, z = [1] * (3 - len(long_axes)) + long_axes
    return x, y, z, 1 in shape


def border_lifted(mask, x, y, z, all_border):
    """The kernels' border rule, restated in numpy on the lifted [X, Y, Z] volume."""
    m = mask.reshape(x, y, z).astype(bool)
    if all_border:
        return m
    inner = m.copy()
    for axis in range(3):
        if m.shape[axis] == 1:
            continue
        padded = np.pad(m, [(1, 1) if a == axis else (0, 0) for a in range(3)], constant_values=False)
        n = m.shape[axis]
        inner &= np.take(padded, range(0, n), axis=axis) & np.take(padded, range(2, n + 2), axis=axis)
    return m & ~inner


def region_masks(labels):
    """(WT, CT, ET) of model/evaluation.py: v != 0, v in {2, 3}, v == 3; a label outside 0..3 is WT only."""
    labels = np.asarray(labels)
    return labels != 0, (labels == 2) | (labels == 3), labels == 3


def border_bits(pred, truth, all_border):
    """uint8 [X, Y, Z] of two lifted label volumes.  A lone voxel has no neighbour inside: its own border."""
    x, y, z = pred.shape
    all_border = bool(all_border) or (x, y, z) == (1, 1, 1)
    bits = np.zeros((x, y, z), dtype=np.uint8)
    for side, vol in enumerate((pred, truth)):
        for r, mask in enumerate(region_masks(vol)):
            bits |= border_lifted(mask, x, y, z, all_border).astype(np.uint8) << (3 * side + r)
    return bits


def channel(bits, c):
    return ((bits >> c) & 1).astype(bool)


# ---------------------------------------------------------------------------------------------- the distances
def bound(shape, units):
    """B = sum_a u_a^2 (N_a - 1)^2 in Python ints: the largest D2 and the largest h of a volume."""
    return sum(int(u) ** 2 * (int(n) - 1) ** 2 for u, n in zip(units, shape))


def admitted(shape, units):
    """The weighted kernels' admission rule in Python ints: B * max(N) < 2^62 (extents in [1, 4097], < 2^31 voxels)."""
    return all(1 <= n <= 4097 for n in shape) and math.prod(shape) < (1 << 31) and \
        all(1 <= u <= 1000000 for u in units) and bound(shape, units) * max(shape) < LIMIT


def g1_ref(bits):
    """uint16 [6, X, Y, Z]: |z - z'| to the nearest z' of the line (x, y, .) in the channel, 0xFFFF without one."""
    x, y, z = bits.shape
    zs = np.arange(z, dtype=np.int64)
    out = np.full((CHANNELS, x, y, z), INF16, dtype=np.int64)
    for c in range(CHANNELS):
        fx, fy, fz = np.nonzero(channel(bits, c))
        for s in range(0, len(fx), 4096):
            e = slice(s, s + 4096)
            np.minimum.at(out[c], (fx[e, None], fy[e, None], zs[None, :]), np.abs(zs[None, :] - fz[e, None]))
    return out.astype(np.uint16)


def g2_ref(bits, units):
    """int64 [6, X, Y, Z]: min over the channel's voxels (x, y', z') of plane x of uz^2 (z - z')^2 + uy^2 (y - y')^2,
    INF64 where the plane has none (the voxel path stores INF32 there)."""
    x, y, z = bits.shape
    assert bound(bits.shape, units) < LIMIT
    uy2, uz2 = np.int64(int(units[1]) ** 2), np.int64(int(units[2]) ** 2)
    ys, zs = np.arange(y, dtype=np.int64)[:, None, None], np.arange(z, dtype=np.int64)[None, :, None]
    out = np.full((CHANNELS, x, y, z), INF64, dtype=np.int64)
    for c in range(CHANNELS):
        on = channel(bits, c)
        for px in np.flatnonzero(on.any(axis=(1, 2))):
            fy, fz = np.nonzero(on[px])
            best = out[c, px]
            rows = max(1, (1 << 22) // (y * z))
            for s in range(0, len(fy), rows):
                dy, dz = ys - fy[None, None, s:s + rows], zs - fz[None, None, s:s + rows]
                np.minimum(best, (uy2 * dy * dy + uz2 * dz * dz).min(axis=2), out=best)
    return out


def nearest_d2(a, b, units):
    """int64 [|A|]: min over q in b of sum_a u_a^2 (p_a - q_a)^2 for every p in a (points as [k, 3] index rows),
    from the whole |A| x |B| table in chunks.  The largest entry is checked against 2^62 in Python ints first."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1, 3), np.asarray(b, dtype=np.int64).reshape(-1, 3)
    assert len(b)
    both = np.vstack((a, b))
    span = (both.max(axis=0) - both.min(axis=0)).tolist() if len(a) else [0, 0, 0]
    assert sum(int(u) ** 2 * s ** 2 for u, s in zip(units, span)) < LIMIT
    w = np.array([int(u) ** 2 for u in units], dtype=np.int64)
    out = np.empty(len(a), dtype=np.int64)
    rows = max(1, (1 << 21) // len(b))
    for s in range(0, len(a), rows):
        d = a[s:s + rows, None, :] - b[None, :, :]
        out[s:s + rows] = (d * d * w).sum(axis=2).min(axis=1)
    return out


def ranks95(n):
    """The two ranks np.percentile(., 95) interpolates between, from the kernels' and gts.metrics._lerp95's double
    expression: v = (n - 1) * 0.95, lo = floor(v), hi = lo + 1, or both n - 1 when v >= n - 1."""
    v = (n - 1) * 0.95
    if v >= n - 1:
        return n - 1, n - 1
    lo = int(math.floor(v))
    return lo, lo + 1


Region = namedtuple("Region", "n flags d2_pred d2_truth multiset lo hi d2_lo d2_hi")
Distances = namedtuple("Distances", "units regions")


def distances(bits, units):
    """Per region: n = |B(r, pred)| + |B(r, truth)|, the presence bits (1 pred, 2 truth), D2 of each side's border
    voxels to the other side's border (in index order), the sorted multiset of both, the ranks and the order
    statistics.  A region absent from a side has empty arrays and order statistics 0."""
    regions = []
    for r in range(3):
        p, t = np.argwhere(channel(bits, r)), np.argwhere(channel(bits, 3 + r))
        n, flags = len(p) + len(t), (1 if len(p) else 0) | (2 if len(t) else 0)
        if flags == 3:
            d2_pred, d2_truth = nearest_d2(p, t, units), nearest_d2(t, p, units)
            multiset = np.sort(np.concatenate((d2_pred, d2_truth)))
            lo, hi = ranks95(n)
            regions.append(Region(n, flags, d2_pred, d2_truth, multiset, lo, hi, int(multiset[lo]), int(multiset[hi])))
        else:
            empty = np.zeros(0, dtype=np.int64)
            regions.append(Region(n, flags, empty, empty, empty, 0, 0, 0, 0))
    return Distances(tuple(int(u) for u in units), regions)


def order_stats_rows(dist):
    """int64 [3, 4]: gts_hd95_order_stats_i16's table (and the first four columns of gts_surface_stats_i16's)."""
    return np.array([[g.n, g.d2_lo, g.d2_hi, g.flags] for g in dist.regions], dtype=np.int64)


def within_counts(dist, thresholds):
    """int64 [3, 2, 4]: per region and side (pred, truth) the number of that side's border voxels with D2 <= T_k."""
    out = np.zeros((3, 2, 4), dtype=np.int64)
    for r, g in enumerate(dist.regions):
        for side, d2 in enumerate((g.d2_pred, g.d2_truth)):
            for k, t in enumerate(thresholds):
                assert 0 <= int(t) < (1 << 63)
                out[r, side, k] = int((d2 <= np.int64(int(t))).sum())
    return out


def surface_rows(dist, thresholds):
    """int64 [3, 12]: gts_surface_stats_i16's table."""
    return np.hstack((order_stats_rows(dist), within_counts(dist, thresholds).reshape(3, 8)))


def pick_thresholds(dist):
    """Four thresholds among and between the reference's distinct D2: 0, the maximum, one distinct value from the
    middle and one that lies strictly between two neighbouring distinct values where a gap leaves room."""
    values = np.unique(np.concatenate([g.multiset for g in dist.regions] + [np.zeros(1, dtype=np.int64)])).tolist()
    top, mid = values[-1], values[len(values) // 2]
    gaps = [(a, b) for a, b in zip(values, values[1:]) if b - a > 1]
    between = gaps[len(gaps) // 2][0] + (gaps[len(gaps) // 2][1] - gaps[len(gaps) // 2][0]) // 2 if gaps else top + 1
    return [0, mid, between, top]


# ---------------------------------------------------------------------------------------------- the envelope
def envelope_walk(f, u2):
    """The lower-envelope stack discipline over one line: f[q] a Python int or None (no parabola), h(q) = f(q) +
    u2 q^2.  Returns (ties, largest |product|): how often the pop test (hq - hp)(p - pp) <= (hp - hpp)(q - p) was
    evaluated at equality, and the largest magnitude either side of it took."""
    stack, ties, largest = [], 0, 0
    for q, fq in enumerate(f):
        if fq is None:
            continue
        hq = fq + u2 * q * q
        while len(stack) >= 2:
            (pp, hpp), (p, hp) = stack[-2], stack[-1]
            lhs, rhs = (hq - hp) * (p - pp), (hp - hpp) * (q - p)
            ties += lhs == rhs
            largest = max(largest, abs(lhs), abs(rhs))
            if lhs > rhs:
                break
            stack.pop()
        stack.append((q, hq))
    return ties, largest


def envelope_census(g1, g2, units):
    """((ties, largest product) over every Y line, the same over every X line) of the reference's g values: the Y
    pass walks f = uz^2 g1^2 with curvature uy^2 along (x, ., z), the X pass f = g2 with ux^2 along (., y, z)."""
    ux2, uy2, uz2 = (int(u) ** 2 for u in units)
    _, x, y, z = g1.shape
    y_ties = y_big = x_ties = x_big = 0
    for c in range(CHANNELS):
        for i in range(x):
            for k in range(z):
                t, b = envelope_walk([None if g == INF16 else uz2 * g * g for g in g1[c, i, :, k].tolist()], uy2)
                y_ties, y_big = y_ties + t, max(y_big, b)
        for j in range(y):
            for k in range(z):
                t, b = envelope_walk([None if v == INF64 else v for v in g2[c, :, j, k].tolist()], ux2)
                x_ties, x_big = x_ties + t, max(x_big, b)
    return (y_ties, y_big), (x_ties, x_big)


# ---------------------------------------------------------------------------------------------- the workspaces
HEADER_BYTES = 256
SMALL_BINS = 1024                   # H4's LDS histogram: D2 below it is counted in LDS first
SELECT_THREADS = 1024               # H5: thread t sums bins [t * chunk, (t + 1) * chunk), chunk = ceil(bins / 1024)
MAX_BOUND = 1 << 24                 # the voxel path's largest (X-1)^2 + (Y-1)^2 + (Z-1)^2
RADIX_BINS = 256
SELECT_STATE_BYTES = 112            # SurfaceSelect: 2 x [3][2] uint64 and [3] uint32, padded to its 8-byte alignment
LDS_BUDGET = 64 * 1024

Hd95Layout = namedtuple("Hd95Layout", "bins n counts hist bits g1 g2 total")
SurfaceLayout = namedtuple("SurfaceLayout", "n top_shift counts cursor within sel_hist sel_state bits g1 g2 lists total")


def round256(b):
    return (b + 255) & ~255


def hd95_layout(x, y, z):
    """Byte offsets of gts_hd95_order_stats_i16's workspace, or None where the library refuses the volume."""
    if min(x, y, z) < 1 or x * y * z >= (1 << 31) or bound((x, y, z), (1, 1, 1)) > MAX_BOUND:
        return None
    n, bins = x * y * z, bound((x, y, z), (1, 1, 1)) + 1
    hist = HEADER_BYTES
    bits = hist + round256(3 * bins * 4)
    g1 = bits + round256(n)
    g2 = g1 + round256(CHANNELS * n * 2)
    return Hd95Layout(bins, n, 0, hist, bits, g1, g2, g2 + CHANNELS * n * 4)


def surface_layout(x, y, z, units):
    """Byte offsets of gts_surface_stats_i16's workspace, or None where the library refuses the volume."""
    if not admitted((x, y, z), units):
        return None
    n, top_shift = x * y * z, 0
    while top_shift < 56 and bound((x, y, z), units) >> (top_shift + 8):
        top_shift += 8
    sel_hist = HEADER_BYTES
    sel_state = sel_hist + 3 * 2 * RADIX_BINS * 4
    bits = sel_state + round256(SELECT_STATE_BYTES)
    g1 = bits + round256(n)
    g2 = g1 + round256(CHANNELS * n * 2)
    lists = g2 + round256(CHANNELS * n * 8)
    return SurfaceLayout(n, top_shift, 0, 32, 64, sel_hist, sel_state, bits, g1, g2, lists, lists + 3 * 2 * n * 8)


def lanes(bytes_per_lane, budget=LDS_BUDGET):
    """Lines per workgroup of a line pass: what fits the LDS budget, at most one wave of 64."""
    return min(64, budget // bytes_per_lane)


def pass_lanes(shape, weighted):
    """(lz, ly, lx): the Z pass stages 3 Z + 16 bytes per line, the Y pass 4 Y, the X pass 6 X beside the 4 KiB
    LDS histogram on the voxel path and 10 X on the weighted one."""
    x, y, z = shape
    lx = lanes(10 * x) if weighted else lanes(6 * x, LDS_BUDGET - 4 * SMALL_BINS)
    return lanes(3 * z + 16), lanes(4 * y), lx


def digits(value, top_shift):
    """The 8-bit digits of a key from the top digit of the volume's bound down: H5w's passes."""
    return [(int(value) >> s) & 255 for s in range(top_shift, -1, -8)]


# ============================================================================================== designed inputs
# A case: two lifted int16 volumes, the all_border flag, whether the voxel path admits the shape, the unit triples
# the weighted path runs at, and what the case claims (asserted by tests/test_hd95_ref_host.py on this reference).
Case = namedtuple("Case", "name pred truth all_border voxel units claim")

LATTICE_SHAPES = ((9, 8, 7), (5, 17, 6), (9, 1, 8), (1, 1, 13), (12, 11))
LATTICE_UNITS = ((1, 1, 5), (15, 15, 80), (10000, 9400, 33333), (1000000, 1000000, 1000000))
LATTICE_BACKGROUND = (0.98, 0.9, 0.6)
LATTICE_SEEDS = (0, 1)


def _case(name, pred, truth, all_border=False, voxel=True, units=((1, 1, 1),), claim=None):
    pred, truth = np.ascontiguousarray(pred, dtype=np.int16), np.ascontiguousarray(truth, dtype=np.int16)
    assert pred.shape == truth.shape and pred.ndim == 3
    pred.setflags(write=False)
    truth.setflags(write=False)
    return Case(name, pred, truth, bool(all_border), voxel, tuple(units), claim or {})


def _name(shape):
    return "x".join(str(s) for s in shape)


def _points(shape, points):
    vol = np.zeros(shape, dtype=np.int16)
    for (px, py, pz), label in points:
        vol[px, py, pz] = label
    return vol


def lattice_volume(shape, background, rng, labels=(1, 2, 3)):
    """Each voxel independently: 0 at probability `background`, else one of `labels` uniformly."""
    p = [background] + [(1 - background) / len(labels)] * len(labels)
    return rng.choice(np.array((0,) + tuple(labels), dtype=np.int16), size=shape, p=p)


def lattice_cases(shape):
    """Sparse lattice points of one shape (any rank; lifted here): three densities, several seeds, and for (9, 8, 7)
    one pair with labels outside 0..3."""
    x, y, z, all_border = lift(shape)
    cases = []
    for background in LATTICE_BACKGROUND:
        for seed in LATTICE_SEEDS:
            rng = np.random.default_rng([seed, int(background * 100)] + list(shape))
            pred, truth = lattice_volume(shape, background, rng), lattice_volume(shape, background, rng)
            cases.append(_case(f"lattice-{_name(shape)}-p{background}-s{seed}", pred.reshape(x, y, z),
                               truth.reshape(x, y, z), all_border, units=LATTICE_UNITS))
    if tuple(shape) == (9, 8, 7):
        rng = np.random.default_rng(97)
        pred = lattice_volume(shape, 0.8, rng, labels=(1, 2, 3, 5, -2, 7))
        truth = lattice_volume(shape, 0.8, rng, labels=(3, 4, -1, 2))
        cases.append(_case("lattice-9x8x7-odd-labels", pred, truth, units=LATTICE_UNITS, claim={"odd_labels": True}))
    return cases


# ---- tie lines: three parabolas through one point.  With parabolas at q = 0 and q = 4 of height 0 and one at q = 2
# of height 4 (a feature two steps away along the previous axis) all three meet at 2: the pop test is an equality.
TIE_UNITS = ((1, 1, 1), (7, 7, 7), (15, 15, 80))        # the ties need u equal on the two axes involved


def tie_cases():
    tie_y = _case("tie-y",
                  _points((3, 5, 6), [((1, 0, 1), 3), ((1, 4, 1), 3), ((1, 2, 3), 3)]),
                  _points((3, 5, 6), [((1, 2, 1), 3), ((1, 1, 1), 2), ((0, 3, 2), 1)]),
                  units=TIE_UNITS, claim={"ties": "y"})
    tie_x = _case("tie-x",
                  _points((5, 4, 6), [((0, 1, 1), 3), ((4, 1, 1), 3), ((2, 1, 3), 3)]),
                  _points((5, 4, 6), [((2, 1, 1), 3), ((1, 1, 1), 2), ((3, 2, 2), 1)]),
                  units=TIE_UNITS, claim={"ties": "x"})
    # the full board: pred holds one colour, truth the other, so every voxel is border of one side and every
    # distance ties; truth alternates 3 / 2 along x, which leaves ET a sparser lattice than WT and CT
    grid = np.indices((6, 6, 6))
    parity = grid.sum(axis=0) % 2
    pred = np.where(parity == 0, 3, 0)
    truth = np.where(parity == 1, np.where(grid[0] % 2 == 0, 3, 2), 0)
    board = _case("checkerboard", pred, truth, units=TIE_UNITS, claim={"ties": "xy"})
    return [tie_y, tie_x, board]


# ---- lane switches: sparse borders, with features of both sides in the first and the last line of the last
# workgroup of each of the three line passes.
def _last_group_lines(n_lines, per_group):
    first = per_group * ((n_lines - 1) // per_group)
    return sorted({first, n_lines - 1})


def sparse_pair(shape, seed, weighted, scattered=10):
    rng = np.random.default_rng([seed] + list(shape))
    x, y, z = shape
    pred, truth = np.zeros(shape, dtype=np.int16), np.zeros(shape, dtype=np.int16)
    for vol in (pred, truth):
        at = rng.choice(x * y * z, size=min(scattered, x * y * z), replace=False)
        vol.reshape(-1)[at] = rng.integers(1, 4, size=len(at))
    lz, ly, lx = pass_lanes(shape, weighted)
    for line in _last_group_lines(x * y, lz):                          # Z pass: lines are the flattened (x, y)
        pred[line // y, line % y, rng.integers(z)] = 3
        truth[line // y, line % y, rng.integers(z)] = 3
    for k in _last_group_lines(z, ly):                                 # Y pass: workgroup (z chunk, x)
        pred[x - 1, rng.integers(y), k] = 3
        truth[x - 1, rng.integers(y), k] = 3
    for k in _last_group_lines(z, lx):                                 # X pass: workgroup (z chunk, y)
        pred[rng.integers(x), y - 1, k] = 3
        truth[rng.integers(x), y - 1, k] = 3
    return pred, truth


# shape -> (voxel path?, weighted path?, the claimed (lz, ly, lx) per path; None = not claimed)
LANE_SHAPES = {
    (160, 3, 64): (True, False, {"voxel": (None, None, 64)}),
    (161, 3, 66): (True, False, {"voxel": (None, None, 63)}),
    (102, 3, 64): (False, True, {"weighted": (None, None, 64)}),
    (103, 3, 66): (False, True, {"weighted": (None, None, 63)}),
    (3, 256, 65): (True, True, {"voxel": (None, 64, None), "weighted": (None, 64, None)}),
    (3, 257, 66): (True, True, {"voxel": (None, 63, None), "weighted": (None, 63, None)}),
    (5, 7, 336): (True, True, {"voxel": (64, None, None), "weighted": (64, None, None)}),
    (5, 7, 337): (True, True, {"voxel": (63, None, None), "weighted": (63, None, None)}),
    (4, 3, 63): (True, True, {}),
    (4, 3, 64): (True, True, {}),
    (4, 3, 65): (True, True, {}),
}
LANE_UNITS = ((1, 1, 1), (15, 15, 80))


def lane_cases(shape):
    voxel, weighted, claim = LANE_SHAPES[shape]
    cases = []
    if voxel:
        cases.append(_case(f"lanes-voxel-{_name(shape)}", *sparse_pair(shape, 1, False), units=(),
                           claim={"lanes": claim.get("voxel")}))
    if weighted:
        cases.append(_case(f"lanes-weighted-{_name(shape)}", *sparse_pair(shape, 2, True), voxel=False, units=LANE_UNITS,
                           claim={"lanes": claim.get("weighted")}))
    return cases


# ---- the longest lines.  The voxel path takes (X-1)^2 + (Y-1)^2 + (Z-1)^2 <= 2^24, so a 4097-long line only beside
# two unit axes (bound exactly 2^24); with a 2 x 2 cross-section the longest voxel line is 4096.  The weighted path
# takes 2 x 2 x 4097 at small units: there the X pass has one lane per workgroup.
def long_line_case(shape, voxel, units):
    axis = int(np.argmax(shape))
    length = shape[axis]
    cross = [s - 1 for s in shape]

    def at(along, far):
        p = [c if far else 0 for c in cross]
        p[axis] = along
        return tuple(p)

    pred = _points(shape, [(at(0, False), 3), (at(length // 2, False), 1), (at(length - 1, True), 2)])
    truth = _points(shape, [(at(0, True), 2), (at(length // 2 + 1, True), 3), (at(length - 1, False), 3), (at(7, False), 1)])
    return _case(f"long-{_name(shape)}", pred, truth, all_border=1 in shape, voxel=voxel, units=units,
                 claim={"long_axis": axis})


LONG_VOXEL_SHAPES = ((1, 1, 4097), (1, 4097, 1), (4097, 1, 1), (2, 2, 4096), (2, 4096, 2), (4096, 2, 2))
LONG_WEIGHTED_SHAPES = ((2, 2, 4097), (2, 4097, 2), (4097, 2, 2))
LONG_UNITS = ((1, 1, 1), (3, 2, 5))


def long_line_cases():
    return [long_line_case(s, True, ()) for s in LONG_VOXEL_SHAPES] + \
        [long_line_case(s, False, LONG_UNITS) for s in LONG_WEIGHTED_SHAPES]


# ---- a single pred voxel at the origin and truth voxels at chosen offsets: every truth voxel of a sparse set is
# border, so the multiset is {the smallest |offset|^2} and every |offset|^2.
def origin_case(name, shape, offsets, units=((1, 1, 1),), claim=None, voxel=True):
    pred = _points(shape, [((0, 0, 0), 3)])
    truth = _points(shape, [(tuple(o), 3) for o in offsets])
    assert int((truth != 0).sum()) == len(offsets)
    return _case(name, pred, truth, all_border=1 in shape, voxel=voxel, units=units, claim=claim)


def small_bins_cases():
    """H4's LDS / global split at 1024: 1022 = 31^2 + 6^2 + 5^2, 1024 = 32^2, 1025 = 32^2 + 1 (1023 = 7 mod 8 is not
    a sum of three squares; 1024 and 1025 have no other representation inside 34 x 8 x 8, so those two touch)."""
    return [
        origin_case("small-bins-34x8x8", (34, 8, 8), [(31, 6, 5), (32, 0, 0), (32, 1, 0)],
                    claim={"contains": (1022, 1024, 1025), "bins": 1188}),
        origin_case("small-bins-32x7x6", (32, 7, 6), [(31, 6, 5)], claim={"contains": (1022,), "bins": 1023}),
        origin_case("small-bins-33x1x1", (33, 1, 1), [(32, 0, 0), (5, 0, 0)], claim={"contains": (25, 1024), "bins": 1025}),
    ]


def _distinct_offsets(shape, units, count):
    """`count` offsets inside `shape` with pairwise distinct weighted squared lengths, the shortest first."""
    grid = np.indices(shape).reshape(3, -1).T
    d2 = (grid.astype(np.int64) ** 2 * np.array([int(u) ** 2 for u in units], dtype=np.int64)).sum(axis=1)
    _, first = np.unique(d2, return_index=True)
    first = first[1:count + 1]                                          # without the origin itself
    assert len(first) == count
    return [tuple(int(v) for v in grid[i]) for i in first]


H5_SHAPE = (34, 8, 8)               # bins = 33^2 + 7^2 + 7^2 + 1 = 1188, chunk = 2
H5_COUNTS = (19, 20, 21, 22, 39, 40, 41, 42, 61)


def h5_cases():
    """Where the two ranks fall in H5's chunked walk.  claim: (kind, lo bin, hi bin)."""
    cases = [
        origin_case("h5-one-bin", H5_SHAPE, [(3, 0, 0), (0, 3, 0)], claim={"h5": ("one_bin", 9, 9)}),
        origin_case("h5-one-chunk", H5_SHAPE, [(2, 2, 0), (3, 0, 0)], claim={"h5": ("one_chunk", 8, 9)}),
        origin_case("h5-two-chunks", H5_SHAPE, [(3, 0, 0), (3, 1, 0)], claim={"h5": ("two_chunks", 9, 10)}),
        origin_case("h5-lone-maximum", H5_SHAPE, [(1, 0, 0), (33, 7, 7)], claim={"h5": ("last_bin", 1, 1187)}),
        origin_case("h5-n2", H5_SHAPE, [(2, 1, 1)], claim={"h5": ("n2", 6, 6)}),
    ]
    for n in H5_COUNTS:
        cases.append(origin_case(f"h5-n{n}", H5_SHAPE, _distinct_offsets(H5_SHAPE, (1, 1, 1), n - 1),
                                 claim={"h5": ("count", None, None), "n": n}))
    # (1, 1, 4097): bins = 2^24 + 1, chunk = 16385; 128^2 = 16384 is the last bin of chunk 0
    line = (1, 1, 4097)
    cases += [
        origin_case("h5-line-last-bin", line, [(0, 0, 128)], claim={"h5": ("chunk_last_bin", 16384, 16384)}),
        origin_case("h5-line-deep", line, [(0, 0, 3000), (0, 0, 3001)], claim={"h5": ("deep", 9000000, 9006001)}),
        origin_case("h5-line-across", line, [(0, 0, 128), (0, 0, 129)], claim={"h5": ("two_chunks", 16384, 16641)}),
    ]
    return cases


def h5w_cases():
    """Where the two ranks part in H5w's radix select.  claim: (kind, units): `same` the ranks agree in every digit,
    `top` they differ in the top digit, `last` in the last digit only."""
    u1, uz = (1, 1, 1), (1, 1, 1000)
    return [
        origin_case("h5w-same-u1", H5_SHAPE, [(3, 0, 0), (0, 3, 0)], units=(u1,), claim={"h5w": "same"}),
        origin_case("h5w-top-u1", H5_SHAPE, [(1, 0, 0), (33, 7, 7)], units=(u1,), claim={"h5w": "top"}),
        origin_case("h5w-last-u1", H5_SHAPE, [(16, 2, 0), (16, 2, 1)], units=(u1,), claim={"h5w": "last"}),
        origin_case("h5w-same-uz", H5_SHAPE, [(3, 0, 5)], units=(uz,), voxel=False, claim={"h5w": "same"}),
        origin_case("h5w-top-uz", H5_SHAPE, [(1, 0, 0), (3, 0, 5)], units=(uz,), voxel=False, claim={"h5w": "top"}),
        origin_case("h5w-last-uz", H5_SHAPE, [(3, 0, 5), (3, 1, 5)], units=(uz,), voxel=False, claim={"h5w": "last"}),
    ] + [origin_case(f"h5w-n{n}", H5_SHAPE, _distinct_offsets(H5_SHAPE, (15, 15, 80), n - 1), units=((15, 15, 80),),
                     voxel=False, claim={"h5w": "count", "n": n}) for n in (20, 21, 41)]


# ---- the admission edge.  B * max(N) < 2^62 with max(N) >= 2 gives B < 2^61; a digit at shift 56 would need
# B >= 2^56, hence max(N) < 2^6, while units <= 10^6 then cap B at 3 * 10^12 * 62^2 < 2^54: the highest top digit any
# admitted volume has is at shift 48.  The longest admitted line at unit 10^6 has it: B = 10^12 (N - 1)^2 + 2 with
# N the largest integer for which B * N < 2^62.
EDGE_UNIT = 1000000


def longest_admitted(cross, unit=EDGE_UNIT):
    """The largest N for which a line of N voxels at `unit` beside a cross x cross section is admitted, in Python ints."""
    n = 2
    while admitted((cross, cross, n + 1), (1, 1, unit)):
        n += 1
    return n


def admission_cases(n_long):
    """(2, 2, N) at units (1, 1, 10^6) and (N, 2, 2) at (10^6, 1, 1): features at both ends of the long line, so D2
    reaches B itself, and a third feature plane in the middle, so the long line's envelope evaluates the pop test
    with products near B * N / 3.  The multiset is {10^12, 10^12, 10^12 + 1, 10^12 (N // 2)^2 + 1, B}: rank hi holds
    B, whose top digit is the highest the admission rule allows."""
    cases = []
    for axis, units in ((2, (1, 1, EDGE_UNIT)), (0, (EDGE_UNIT, 1, 1))):
        shape = [2, 2, 2]
        shape[axis] = n_long

        def at(along, c1, c2):
            p = [c1, c2]
            p.insert(axis, along)
            return tuple(p)

        pred = _points(shape, [(at(0, 0, 0), 3)])
        truth = _points(shape, [(at(n_long - 1, 1, 1), 3), (at(1, 0, 0), 3), (at(1, 0, 1), 3), (at(n_long // 2, 0, 1), 3)])
        cases.append(_case(f"admission-{_name(shape)}", pred, truth, voxel=False, units=(units,),
                           claim={"admission": axis, "n_long": n_long}))
    return cases


def all_cases(n_long):
    """Every designed input, n_long being the longest admitted line of the admission cases."""
    cases = [c for shape in LATTICE_SHAPES for c in lattice_cases(shape)] + tie_cases()
    cases += [c for shape in LANE_SHAPES for c in lane_cases(shape)]
    return cases + long_line_cases() + small_bins_cases() + h5_cases() + h5w_cases() + admission_cases(n_long)
