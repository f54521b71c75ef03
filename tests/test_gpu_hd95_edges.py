"""The HD95 and surface-distance kernels (H1-H5 and H3w-H5w of csrc/gts_hd95.hip) one stage at a time, against the
exact integer reference of tests/hd95_ref.py.  Both entry points leave every intermediate in the caller's workspace,
so each call is followed by a read of the border counts and bits, g1, g2, then the histograms and the output row
(voxel path) or the appended lists, their cursors, the threshold counts and the output row (weighted path).  Every
comparison is == on integers; the multiset of every region is compared whole, not at the two ranks the percentile
reads.  tests/test_hd95_ref_host.py asserts, on the reference alone, that each designed input hits its edge, and
that the layouts restated in hd95_ref.py give the library's workspace sizes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import hd95_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _stream():
    from gts import _lib

    return _lib.current_stream()


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int16, order="C")).cuda()        # a copy: the cases are read-only


def _read(ws, offset, count, dtype):
    """`count` items of `dtype` at byte `offset` of the device workspace, as a numpy array."""
    return ws[offset:offset + count * np.dtype(dtype).itemsize].cpu().numpy().view(dtype)


# the reference of a case is computed once and shared by the voxel and the weighted checks (read-only)
@functools.lru_cache(maxsize=None)
def _stage12(case_key):
    case = _CASES[case_key]
    bits = R.border_bits(case.pred, case.truth, case.all_border)
    counts = np.array([int(R.channel(bits, c).sum()) for c in range(R.CHANNELS)], dtype=np.uint32)
    g1 = R.g1_ref(bits)
    for a in (bits, counts, g1):
        a.setflags(write=False)
    return bits, counts, g1


_CASES = {}


def _key(case):
    _CASES[case.name] = case
    return case.name


def _check_front(case, ws, layout):
    """Counts, border bits and g1: the stages both paths share."""
    bits, counts, g1 = _stage12(_key(case))
    n = layout.n
    assert np.array_equal(_read(ws, layout.counts, 6, np.uint32), counts), case.name
    assert np.array_equal(_read(ws, layout.bits, n, np.uint8), bits.reshape(-1)), case.name
    assert np.array_equal(_read(ws, layout.g1, 6 * n, np.uint16), g1.reshape(-1)), case.name
    return bits


def _check_multiset(values_and_counts, want, what):
    """A histogram given by its nonzero bins (values, counts) == np.bincount of the reference multiset."""
    values, counts = values_and_counts
    want_values, want_counts = np.unique(want, return_counts=True)
    assert np.array_equal(values, want_values), what
    assert np.array_equal(counts, want_counts), what


def run_voxel(lib, case):
    """gts_hd95_order_stats_i16 on a workspace the test owns; returns the per-region histograms' nonzero bins."""
    x, y, z = case.pred.shape
    layout = R.hd95_layout(x, y, z)
    assert layout is not None and lib.gts_hd95_workspace(x, y, z) == layout.total, case.name
    ws = torch.full((layout.total,), 0xA5, dtype=torch.uint8, device="cuda")      # nothing relies on a clean workspace
    out = torch.full((3, 4), -7, dtype=torch.int64, device="cuda")
    pred, truth = _dev(case.pred), _dev(case.truth)
    code = lib.gts_hd95_order_stats_i16(pred.data_ptr(), truth.data_ptr(), x, y, z, int(case.all_border), out.data_ptr(),
                                        ws.data_ptr(), layout.total, _stream())
    assert code == 0, case.name
    torch.cuda.synchronize()
    bits = _check_front(case, ws, layout)
    g2 = R.g2_ref(bits, (1, 1, 1))
    want_g2 = np.where(g2 == R.INF64, R.INF32, g2).astype(np.int32)
    assert np.array_equal(_read(ws, layout.g2, 6 * layout.n, np.int32), want_g2.reshape(-1)), case.name
    dist = R.distances(bits, (1, 1, 1))
    hist = _read(ws, layout.hist, 3 * layout.bins, np.uint32).reshape(3, layout.bins)
    found = []
    for r, g in enumerate(dist.regions):
        nonzero = np.flatnonzero(hist[r])
        found.append((nonzero, hist[r][nonzero].astype(np.int64)))
        _check_multiset(found[r], g.multiset, (case.name, R.REGIONS[r]))          # all zero for an absent region
    assert np.array_equal(out.cpu().numpy(), R.order_stats_rows(dist)), case.name
    return found


def run_weighted(lib, case, units):
    """gts_surface_stats_i16 on a workspace the test owns; returns the per-region lists as (values, counts)."""
    x, y, z = case.pred.shape
    layout = R.surface_layout(x, y, z, units)
    c_units = (ctypes.c_int64 * 3)(*units)
    assert layout is not None and lib.gts_surface_workspace(x, y, z, c_units) == layout.total, (case.name, units)
    bits, _, _ = _stage12(_key(case))
    dist = R.distances(bits, units)
    thresholds = R.pick_thresholds(dist)
    assert thresholds[0] == 0 and thresholds[3] == max([0] + [int(g.multiset[-1]) for g in dist.regions if g.flags == 3])
    ws = torch.full((layout.total,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((3, 12), -7, dtype=torch.int64, device="cuda")
    pred, truth = _dev(case.pred), _dev(case.truth)
    code = lib.gts_surface_stats_i16(pred.data_ptr(), truth.data_ptr(), x, y, z, int(case.all_border), c_units,
                                     (ctypes.c_int64 * 4)(*thresholds), 4, out.data_ptr(), ws.data_ptr(), layout.total,
                                     _stream())
    assert code == 0, (case.name, units)
    torch.cuda.synchronize()
    _check_front(case, ws, layout)
    n = layout.n
    assert np.array_equal(_read(ws, layout.g2, 6 * n, np.int64), R.g2_ref(bits, units).reshape(-1)), (case.name, units)
    cursor = _read(ws, layout.cursor, 3, np.uint32)
    found = []
    for r, g in enumerate(dist.regions):
        held = len(g.multiset)                                                     # n_r, or 0 for an absent region
        assert int(cursor[r]) == held and held in (0, g.n), (case.name, units, R.REGIONS[r])
        got = np.sort(_read(ws, layout.lists + r * 2 * n * 8, held, np.int64))
        assert np.array_equal(got, g.multiset), (case.name, units, R.REGIONS[r])
        found.append(np.unique(got, return_counts=True))
    within = _read(ws, layout.within, 24, np.uint32).reshape(3, 2, 4)
    assert np.array_equal(within, R.within_counts(dist, thresholds)), (case.name, units, thresholds)
    assert np.array_equal(out.cpu().numpy(), R.surface_rows(dist, thresholds)), (case.name, units, thresholds)
    return found


def run_case(lib, case):
    """Both paths as the case allows.  A volume the voxel path takes also runs the weighted path at units (1, 1, 1),
    where the list's bincount must be the voxel path's histogram."""
    hist = run_voxel(lib, case) if case.voxel else None
    units_run = case.units + (((1, 1, 1),) if case.voxel and (1, 1, 1) not in case.units else ())
    assert units_run, case.name
    for units in units_run:
        lists = run_weighted(lib, case, units)
        if hist is not None and tuple(units) == (1, 1, 1):
            for r in range(3):
                assert np.array_equal(hist[r][0], lists[r][0]) and np.array_equal(hist[r][1], lists[r][1]), (case.name, r)


def _id(shape):
    return "x".join(str(s) for s in shape)


# ---- sparse lattice points: isolated voxels make three parabolas meet in one point all the time -------------------
@pytest.mark.parametrize("shape", R.LATTICE_SHAPES, ids=_id)
def test_sparse_lattice_points(lib, shape):
    cases = R.lattice_cases(shape)
    assert len(cases) >= 6
    for case in cases:
        assert case.voxel and case.units == R.LATTICE_UNITS
        run_case(lib, case)


# ---- tie lines ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(3), ids=["tie-y", "tie-x", "checkerboard"])
def test_envelope_ties(lib, index):
    run_case(lib, R.tie_cases()[index])


# ---- exactly at the lane switches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(R.LANE_SHAPES), ids=_id)
def test_lane_switches(lib, shape):
    cases = R.lane_cases(shape)
    assert cases
    for case in cases:
        run_case(lib, case)


@pytest.mark.parametrize("index", range(len(R.LONG_VOXEL_SHAPES) + len(R.LONG_WEIGHTED_SHAPES)),
                         ids=[_id(s) for s in R.LONG_VOXEL_SHAPES + R.LONG_WEIGHTED_SHAPES])
def test_longest_lines(lib, index):
    """The voxel path admits a 4097-long line only beside two unit axes ((X-1)^2 + (Y-1)^2 + (Z-1)^2 <= 2^24), so the
    2 x 2 cross-sections run 4096 long there and 4097 long on the weighted path."""
    run_case(lib, R.long_line_cases()[index])


# ---- H4's LDS / global split --------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(3), ids=["34x8x8", "32x7x6-bins-1023", "33x1x1-bins-1025"])
def test_small_bins_split(lib, index):
    run_case(lib, R.small_bins_cases()[index])


# ---- where the ranks fall: H5's chunks, H5w's digits -----------------------------------------------------------------
def test_h5_rank_placement_chunk_2(lib):
    cases = [c for c in R.h5_cases() if c.pred.shape == R.H5_SHAPE]
    assert len(cases) == 5 + len(R.H5_COUNTS)
    for case in cases:
        run_case(lib, case)


@pytest.mark.parametrize("name", ["h5-line-last-bin", "h5-line-deep", "h5-line-across"])
def test_h5_rank_placement_chunk_16385(lib, name):
    (case,) = [c for c in R.h5_cases() if c.name == name]
    run_case(lib, case)


def test_h5w_digit_placement(lib):
    cases = R.h5w_cases()
    assert len(cases) == 9
    for case in cases:
        run_case(lib, case)


# ---- the admission edge ---------------------------------------------------------------------------------------------
def test_admission_edge_top_digit_and_largest_products(lib):
    """The longest line the library admits at unit 10^6.  B * max(N) < 2^62 with max(N) >= 2 gives B < 2^61; a digit
    at shift 56 would need B >= 2^56, hence max(N) < 64, and units <= 10^6 cap B at 3 * 10^12 * 62^2 < 2^54 then:
    shift 48 is the highest top digit an admitted volume has, and this one has it (asserted on the host)."""
    unit = (ctypes.c_int64 * 3)(1, 1, R.EDGE_UNIT)
    n = 2
    while lib.gts_surface_workspace(2, 2, n + 1, unit) > 0:
        n += 1
    assert n == R.longest_admitted(2)
    for case in R.admission_cases(n):
        (units,) = case.units
        assert R.surface_layout(*case.pred.shape, units).top_shift == 48
        run_case(lib, case)
