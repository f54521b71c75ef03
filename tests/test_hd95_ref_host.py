"""tests/hd95_ref.py on its own, no GPU: the exact integer reference against the project's scipy routes, the
precondition of every designed input of tests/test_gpu_hd95_edges.py (an input that stops hitting its edge fails
here, on the reference alone), the restated workspace layouts against the library's sizes, and the admission edge."""
import ctypes
import functools

import numpy as np
import pytest

from tests import hd95_ref as R
from tests import surface_ref

SPACINGS = ((1.0, 1.0, 5.0), (0.9375, 0.9375, 5.0))         # units (1, 1, 5) and (15, 15, 80)
TOLERANCES = (0.5, 1.0, 2.0, 5.0)


def _units(*u):
    return (ctypes.c_int64 * 3)(*u)


# ------------------------------------------------------------------------------- the reference against scipy
@functools.lru_cache(maxsize=None)
def _volumes():
    """Some twenty small pairs: blobs and sparse points, 3-D, 2-D and unit-axis shapes, labels outside 0..3."""
    rng = np.random.default_rng(2024)
    pairs = []
    for shape in ((9, 8, 7), (6, 11, 5), (12, 11), (9, 1, 8), (1, 1, 13), (13,), (1, 7, 1, 6)):
        pairs.append((surface_ref.blobs(shape, rng), surface_ref.blobs(shape, rng)))
        for background in (0.9, 0.6):
            pairs.append((R.lattice_volume(shape, background, rng), R.lattice_volume(shape, background, rng)))
    pairs.append((R.lattice_volume((7, 6, 8), 0.7, rng, labels=(1, 2, 3, 5, -2, 7)),
                  R.lattice_volume((7, 6, 8), 0.7, rng, labels=(3, 4, -1))))
    pairs.append((surface_ref.blobs((8, 9, 7), rng, labels=(1, 2)), surface_ref.blobs((8, 9, 7), rng)))   # ET on one side
    pairs.append((np.zeros((5, 6, 4), np.int16), R.lattice_volume((5, 6, 4), 0.8, rng)))
    return pairs


def test_voxel_reference_equals_the_scipy_route():
    from gts.metrics import percentile95_from_order_stats
    from model import evaluation

    assert len(_volumes()) >= 20
    for pred, truth in _volumes():
        x, y, z, all_border = R.lift(pred.shape)
        bits = R.border_bits(pred.reshape(x, y, z), truth.reshape(x, y, z), all_border)
        got = []
        for n, d2_lo, d2_hi, flags in R.order_stats_rows(R.distances(bits, (1, 1, 1))).tolist():
            got.append(percentile95_from_order_stats(n, d2_lo, d2_hi) if flags == 3 else (0.0 if flags == 0 else 300.0))
        want = [float(v) for v in evaluation.calculate_hd95s(pred, truth)]
        assert got == want, (pred.shape, got, want)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_weighted_reference_equals_the_scipy_route(spacing):
    from gts.metrics import hd95_mm_from_row, spacing_units, surface_dices_from_row, tolerance_thresholds

    units, scale = spacing_units(spacing)
    assert units == surface_ref.units_of(spacing)[0]
    thresholds = tolerance_thresholds(TOLERANCES, spacing)
    for pred, truth in _volumes():
        x, y, z, _ = R.lift(pred.shape)
        pred, truth = pred.reshape(x, y, z), truth.reshape(x, y, z)       # scipy sees the 3-D volume
        rows = R.surface_rows(R.distances(R.border_bits(pred, truth, 1 in pred.shape), units), thresholds).tolist()
        want_hd, want_nsd = surface_ref.scores(pred, truth, spacing, TOLERANCES)
        assert [hd95_mm_from_row(row, scale) for row in rows] == want_hd, (pred.shape, spacing)
        per_region = [surface_dices_from_row(row, len(TOLERANCES)) for row in rows]
        assert [[per_region[r][k] for r in range(3)] for k in range(len(TOLERANCES))] == want_nsd, (pred.shape, spacing)


@pytest.mark.parametrize("units", [(1, 1, 1), (15, 15, 80), (10000, 9400, 33333)])
def test_intermediates_compose_to_the_distances(units):
    """g1 and g2 are written from their own definitions; chained as the passes chain them they must give D2."""
    for pred, truth in _volumes()[:9]:
        x, y, z, all_border = R.lift(pred.shape)
        bits = R.border_bits(pred.reshape(x, y, z), truth.reshape(x, y, z), all_border)
        g1, g2, dist = R.g1_ref(bits), R.g2_ref(bits, units), R.distances(bits, units)
        ys = np.arange(y, dtype=np.int64)
        for c in range(R.CHANNELS):
            f = np.where(g1[c] == R.INF16, np.int64(R.LIMIT), units[2] ** 2 * g1[c].astype(np.int64) ** 2)
            along_y = (f[:, None, :, :] + units[1] ** 2 * (ys[:, None] - ys[None, :])[None, :, :, None] ** 2).min(axis=2)
            assert np.array_equal(np.where(along_y >= R.LIMIT, R.INF64, along_y), g2[c])
            region, side = c % 3, c // 3
            g = dist.regions[region]
            if g.flags != 3:
                continue
            at = np.argwhere(R.channel(bits, 3 * (1 - side) + region))           # the opposite side's border
            want = g.d2_truth if side == 0 else g.d2_pred
            xs = np.arange(x, dtype=np.int64)
            col = g2[c][:, at[:, 1], at[:, 2]]                                    # [X, k]
            col = np.where(col == R.INF64, np.int64(R.LIMIT), col)
            assert np.array_equal((col + units[0] ** 2 * (xs[:, None] - at[None, :, 0]) ** 2).min(axis=0), want)


def test_ranks_are_numpys():
    for n in list(range(1, 400)) + [1000, 99999, 100001]:
        lo, hi = R.ranks95(n)
        values = np.arange(n, dtype=np.float64)
        assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1
        frac = (n - 1) * 0.95 - lo
        assert np.percentile(values, 95) == pytest.approx(lo + frac * (hi - lo), abs=1e-9 * n)


# ------------------------------------------------------------------------------- preconditions of the designed inputs
def _bits(case):
    return R.border_bits(case.pred, case.truth, case.all_border)


def test_lattice_cases_are_what_they_say():
    names = set()
    for shape in R.LATTICE_SHAPES:
        cases = R.lattice_cases(shape)
        assert len(cases) >= len(R.LATTICE_BACKGROUND) * len(R.LATTICE_SEEDS) >= 6
        for case in cases:
            names.add(case.name)
            assert case.pred.shape == R.lift(shape)[:3] and case.all_border == (1 in shape)
            assert case.units == R.LATTICE_UNITS and case.voxel
            for u in case.units:
                assert R.admitted(case.pred.shape, u)
        for background, group in zip(R.LATTICE_BACKGROUND, (cases[0:2], cases[2:4], cases[4:6])):
            share = np.mean([np.mean(c.pred == 0) for c in group] + [np.mean(c.truth == 0) for c in group])
            assert abs(share - background) < 0.1, (shape, background, share)
    odd = [c for c in R.lattice_cases((9, 8, 7)) if c.claim.get("odd_labels")]
    assert len(odd) == 1 and {5, -2, 7} <= set(odd[0].pred.ravel().tolist()) and {4, -1} <= set(odd[0].truth.ravel().tolist())
    assert len(names) == sum(len(R.lattice_cases(s)) for s in R.LATTICE_SHAPES)
    # the densest volumes still have a border on both sides of every region somewhere, the sparsest an absent one
    flags = [g.flags for s in R.LATTICE_SHAPES for c in R.lattice_cases(s) for g in R.distances(_bits(c), (1, 1, 1)).regions]
    assert 3 in flags and any(f != 3 for f in flags)


def test_tie_cases_evaluate_the_pop_test_at_equality():
    tie_y, tie_x, board = R.tie_cases()
    assert board.pred.shape == (6, 6, 6) and ((board.pred != 0) ^ (board.truth != 0)).all()
    assert (_bits(board) != 0).all()                                       # every voxel is border
    for case in (tie_y, tie_x, board):
        bits = _bits(case)
        g1 = R.g1_ref(bits)
        for units in ((1, 1, 1), (7, 7, 7)):
            (y_ties, _), (x_ties, _) = R.envelope_census(g1, R.g2_ref(bits, units), units)
            assert ("y" not in case.claim["ties"]) or y_ties > 0, (case.name, units)
            assert ("x" not in case.claim["ties"]) or x_ties > 0, (case.name, units)
    # on the board every distance ties as well: one value per region
    for g in R.distances(_bits(board), (1, 1, 1)).regions:
        assert g.flags == 3 and len(set(g.multiset.tolist())) <= 2


def test_lane_cases_sit_at_the_switches():
    # the launch geometry the shapes were chosen for: 64 lanes on one side of each switch, 63 on the other
    assert R.pass_lanes((160, 3, 64), False)[2] == 64 and R.pass_lanes((161, 3, 66), False)[2] == 63
    assert R.pass_lanes((102, 3, 64), True)[2] == 64 and R.pass_lanes((103, 3, 66), True)[2] == 63
    for weighted in (False, True):
        assert R.pass_lanes((3, 256, 65), weighted)[1] == 64 and R.pass_lanes((3, 257, 66), weighted)[1] == 63
        assert R.pass_lanes((5, 7, 336), weighted)[0] == 64 and R.pass_lanes((5, 7, 337), weighted)[0] == 63
    assert 35 % 63 != 0
    assert R.pass_lanes((4097, 2, 2), True)[2] == 1                        # one lane per workgroup
    for shape in R.LANE_SHAPES:
        for case in R.lane_cases(shape):
            weighted = not case.voxel
            lz, ly, lx = R.pass_lanes(shape, weighted)
            for got, want in zip((lz, ly, lx), case.claim["lanes"] or (None,) * 3):
                assert want is None or got == want, case.name
            x, y, z = shape
            bits = _bits(case)
            pred_on, truth_on = (bits & 7) != 0, (bits >> 3) != 0
            assert pred_on.sum() < 40 and truth_on.sum() < 40              # sparse
            for on in (pred_on, truth_on):
                lines = on.any(axis=2).reshape(-1)
                assert all(lines[k] for k in R._last_group_lines(x * y, lz)), case.name
                assert all(on[x - 1, :, k].any() for k in R._last_group_lines(z, ly)), case.name
                assert all(on[:, y - 1, k].any() for k in R._last_group_lines(z, lx)), case.name
    assert [len(R._last_group_lines(66, 63)), R._last_group_lines(66, 63)] == [2, [63, 65]]


def test_long_line_cases(hip_lib):
    assert hip_lib.gts_hd95_workspace(2, 2, 4097) == 0 and R.hd95_layout(2, 2, 4097) is None      # bound 2^24 + 2
    cases = R.long_line_cases()
    assert [c.pred.shape for c in cases] == list(R.LONG_VOXEL_SHAPES + R.LONG_WEIGHTED_SHAPES)
    for case in cases:
        shape, axis = case.pred.shape, case.claim["long_axis"]
        assert (R.hd95_layout(*shape) is not None) == case.voxel
        assert all(R.admitted(shape, u) for u in case.units)
        along = np.moveaxis(_bits(case), axis, 0).reshape(shape[axis], -1)
        for side in (7, 56):
            on = ((along & side) != 0).any(axis=1)
            assert on[0] and on[-1] and on[shape[axis] // 2 - 1: shape[axis] // 2 + 2].any(), case.name


def test_small_bins_cases_straddle_the_split():
    assert all(a * a + b * b + c * c != 1023 for a in range(32) for b in range(32) for c in range(32))
    first, below, above = R.small_bins_cases()
    for case in (first, below, above):
        values = R.distances(_bits(case), (1, 1, 1)).regions[0].multiset.tolist()
        assert set(case.claim["contains"]) <= set(values), case.name
        assert R.hd95_layout(*case.pred.shape).bins == case.claim["bins"], case.name
    assert {1022, 1024, 1025} <= set(R.distances(_bits(first), (1, 1, 1)).regions[0].multiset.tolist())
    assert R.hd95_layout(32, 7, 6).bins == 1023 < R.SMALL_BINS < R.hd95_layout(33, 1, 1).bins == 1025
    assert max(R.distances(_bits(below), (1, 1, 1)).regions[0].multiset.tolist()) == 1022     # the last bin below 1024


def test_h5_cases_put_the_ranks_where_they_say():
    seen = set()
    for case in R.h5_cases():
        layout = R.hd95_layout(*case.pred.shape)
        chunk = -(-layout.bins // R.SELECT_THREADS)
        assert chunk == (2 if case.pred.shape == R.H5_SHAPE else 16385)
        regions = R.distances(_bits(case), (1, 1, 1)).regions
        assert all(g.flags == 3 and g.multiset.tolist() == regions[0].multiset.tolist() for g in regions)
        g = regions[0]
        kind, lo, hi = case.claim["h5"]
        seen.add((kind, chunk))
        assert lo is None or (g.d2_lo, g.d2_hi) == (lo, hi), (case.name, g.d2_lo, g.d2_hi)
        lo, hi = g.d2_lo, g.d2_hi
        if kind == "one_bin":
            assert lo == hi and g.lo != g.hi
        elif kind == "one_chunk":
            assert lo // chunk == hi // chunk and lo % chunk == 0 and hi == lo + 1
        elif kind == "two_chunks":
            assert hi // chunk == lo // chunk + 1 and lo % chunk == chunk - 1
            assert chunk != 2 or (lo % 2 == 1 and hi == lo + 1)                   # bins 2t + 1 and 2t + 2
        elif kind == "last_bin":
            assert hi == layout.bins - 1 == int(g.multiset[-1]) and g.multiset.tolist().count(hi) == 1 and lo < hi
        elif kind == "n2":
            assert g.n == 2 and (g.lo, g.hi) == (0, 1)
        elif kind == "count":
            values = g.multiset.tolist()
            assert g.n == case.claim["n"] and len(set(values)) == g.n - 1 and lo < hi
        elif kind == "chunk_last_bin":
            assert lo == hi and lo % chunk == chunk - 1
        elif kind == "deep":
            assert lo // chunk == hi // chunk and lo != hi
            assert all(1000 < v % chunk < chunk - 1000 for v in (lo, hi))
        else:
            raise AssertionError(kind)
    assert seen == {("one_bin", 2), ("one_chunk", 2), ("two_chunks", 2), ("last_bin", 2), ("n2", 2), ("count", 2),
                    ("chunk_last_bin", 16385), ("deep", 16385), ("two_chunks", 16385)}
    # the counts around multiples of 20 include the exact products 19.0 and 38.0 and both neighbours
    assert {R.ranks95(n) for n in (20, 21, 22)} == {(18, 19), (19, 20)} and R.ranks95(41) == (38, 39)
    assert {20, 21, 22, 40, 41, 42} <= set(R.H5_COUNTS)


def test_h5w_cases_part_at_the_digit_they_claim():
    seen = set()
    for case in R.h5w_cases():
        (units,) = case.units
        layout = R.surface_layout(*case.pred.shape, units)
        g = R.distances(_bits(case), units).regions[0]
        lo, hi = R.digits(g.d2_lo, layout.top_shift), R.digits(g.d2_hi, layout.top_shift)
        kind = case.claim["h5w"]
        seen.add((kind, len(lo)))
        assert g.flags == 3 and g.d2_hi >> (layout.top_shift + 8) == 0
        if kind == "same":
            assert lo == hi and g.lo != g.hi
        elif kind == "top":
            assert lo[0] != hi[0]
        elif kind == "last":
            assert len(lo) >= 2 and lo[:-1] == hi[:-1] and lo[-1] != hi[-1]
        else:
            assert kind == "count" and g.n == case.claim["n"] and g.d2_lo < g.d2_hi
    assert {("same", 2), ("top", 2), ("last", 2), ("same", 4), ("top", 4), ("last", 4)} <= seen


def test_no_admitted_volume_has_a_digit_at_shift_56():
    """B * max(N) < 2^62 with B >= 2^56 needs max(N) < 64, and then B <= 3 * 10^12 * 62^2 < 2^56."""
    assert all(3 * 10 ** 12 * (n - 1) ** 2 < (1 << 56) for n in range(1, 64))
    assert (1 << 56) * 64 >= R.LIMIT


def test_admission_edge(hip_lib):
    ws = hip_lib.gts_surface_workspace
    n = 2
    while ws(2, 2, n + 1, _units(1, 1, R.EDGE_UNIT)) > 0:
        n += 1
    assert n == R.longest_admitted(2)
    assert ws(2, 2, n, _units(1, 1, R.EDGE_UNIT)) > 0 and ws(2, 2, n + 1, _units(1, 1, R.EDGE_UNIT)) == 0
    assert ws(n, 2, 2, _units(R.EDGE_UNIT, 1, 1)) > 0 and ws(n + 1, 2, 2, _units(R.EDGE_UNIT, 1, 1)) == 0
    b = lambda k: 10 ** 12 * (k - 1) ** 2 + 2                                      # noqa: E731
    assert b(n) * n < (1 << 62) <= b(n + 1) * (n + 1)
    for case in R.admission_cases(n):
        (units,) = case.units
        shape = case.pred.shape
        layout = R.surface_layout(*shape, units)
        assert layout.top_shift == 48 and R.bound(shape, units) == b(n)
        bits = _bits(case)
        g = R.distances(bits, units).regions[0]
        middle = 10 ** 12 * (n // 2) ** 2 + 1
        assert g.multiset.tolist() == [10 ** 12, 10 ** 12, 10 ** 12 + 1, middle, b(n)]
        assert (g.d2_lo, g.d2_hi) == (middle, b(n))
        assert R.digits(g.d2_hi, 48)[0] == b(n) >> 48 > R.digits(g.d2_lo, 48)[0] > 0
        (_, y_big), (_, x_big) = R.envelope_census(R.g1_ref(bits), R.g2_ref(bits, units), units)
        assert max(y_big, x_big) < (1 << 63)
        if case.claim["admission"] == 0:                                          # the long line is the X pass's
            assert x_big > (1 << 60), x_big


# ------------------------------------------------------------------------------- the layouts
def test_restated_layouts_give_the_librarys_sizes(hip_lib):
    n_long = R.longest_admitted(2)
    shapes = set()
    for case in R.all_cases(n_long):
        x, y, z = case.pred.shape
        shapes.add((x, y, z))
        layout = R.hd95_layout(x, y, z)
        assert hip_lib.gts_hd95_workspace(x, y, z) == (layout.total if layout else 0), case.name
        assert (layout is not None) or not case.voxel, case.name
        for units in case.units + ((1, 1, 1),):
            layout = R.surface_layout(x, y, z, units)
            assert hip_lib.gts_surface_workspace(x, y, z, _units(*units)) == (layout.total if layout else 0), case.name
            assert layout is not None or units not in case.units, case.name
    assert len(shapes) > 30
    assert R.HEADER_BYTES == 256 and R.round256(1) == 256 and R.round256(256) == 256 and R.round256(257) == 512
    big = R.hd95_layout(240, 240, 155)
    assert hip_lib.gts_hd95_workspace(240, 240, 155) == big.total and big.counts == 0 and big.hist == 256
    assert R.surface_layout(240, 240, 155, (15, 15, 80)).total == hip_lib.gts_surface_workspace(240, 240, 155, _units(15, 15, 80))
    assert R.surface_layout(1, 1, 4097, (1, 1, 99971)) is None and R.hd95_layout(1, 1, 4098) is None


# ------------------------------------------------------------------------------- what the multiset criterion adds
def test_single_value_perturbations_old_and_new_criterion(capsys):
    """+1 on one border voxel's D2 of a blob pair: the two ranks the percentile reads see a few percent of them, the
    multiset every one.  The old figure is printed for the record, the new one asserted."""
    rng = np.random.default_rng(16)
    pred, truth = surface_ref.blobs((16, 16, 16), rng), surface_ref.blobs((16, 16, 16), rng)
    dist = R.distances(R.border_bits(pred, truth, False), (1, 1, 1))
    tried = old = new = 0
    for g in dist.regions:
        assert g.flags == 3
        for i in rng.choice(g.n, size=min(g.n, 150), replace=False):
            wrong = g.multiset.copy()
            wrong[i] += 1
            wrong.sort()
            tried += 1
            old += (int(wrong[g.lo]), int(wrong[g.hi])) != (g.d2_lo, g.d2_hi)
            new += not np.array_equal(wrong, g.multiset)
    with capsys.disabled():
        print(f"\n+1 perturbations: {tried} tried, two-rank criterion sees {old}, multiset criterion sees {new}")
    assert tried >= 300 and new == tried and old < tried
