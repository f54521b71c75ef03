"""The clustered K1 / K2 kernels (csrc/gts_spmm_cluster.hip) over schedules made by hand (tests/cluster_ref.py, proven on the
CPU by tests/test_cluster_ref_host.py) against the per-row references of tests/spmm_ref.py, bit for bit, on a real MI355X:
every ordered pair of degrees in one wave slot, clusters of 1 .. 32 rows, a neighbour list as long as the limits and the LDS
allow, records on both sides of one LDS-DMA piece, cluster counts and unit counts on both sides of every threshold of the
launch geometry under all three dealing modes, every tuning option, signed zeros, NaN and Inf, batches, repeated launches.

The kernels are called through the C ABI with the schedule uploaded as gts.graph._DeviceSchedule uploads it; outputs and
winners are carved from fenced buffers, and after every launch the fences are intact and every element was written (or, for
a refused launch, none).  No tolerance anywhere.  K2 always runs on the winners K1 has just written."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import gts
from gts import _lib
from gts.graph import _DeviceSchedule
from gts.ops import current_stream, ptr
from gts.schedule import ClusterSchedule
from tests import cluster_ref as C
from tests import nonfinite_ref as NF
from tests import spmm_ref as R
from tests import test_gpu_spmm_edges as P
from tests.helpers import slots_to_sources
from tests.test_gpu_spmm_edges import _arg_checked, _fenced_arg, _float_checked, _slots, _up

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = C.F
OK, SHAPE = _lib.const("GTS_OK"), _lib.const("GTS_ERR_SHAPE")
OPTION_DEFAULTS = {_lib.const("GTS_OPT_CLUSTER_DEALING"): 0, _lib.const("GTS_OPT_CLUSTER_RING"): 0,
                   _lib.const("GTS_OPT_CLUSTER_PER_CU"): 0, _lib.const("GTS_OPT_CLUSTER_CONSUMERS"): 0,
                   _lib.const("GTS_OPT_CLUSTER_STREAMING"): -1}
DEALING, RING, PER_CU, CONSUMERS, STREAMING = OPTION_DEFAULTS


@pytest.fixture(scope="module", autouse=True)
def lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_lib


def _current_options():
    return {k: _lib.load().gts_get_option(k) for k in OPTION_DEFAULTS}


@contextmanager
def _options(values):
    lib = _lib.load()
    assert _current_options() == OPTION_DEFAULTS
    try:
        for k, v in values.items():
            assert lib.gts_set_option(k, v) == 0
        yield
    finally:
        for k, v in OPTION_DEFAULTS.items():
            lib.gts_set_option(k, v)
    assert _current_options() == OPTION_DEFAULTS


def _counters():
    return torch.zeros(_lib.const("GTS_CLUSTER_COUNTER_WORDS"), dtype=torch.int32, device=DEV)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ---------------------------------------------------------------- fenced launches through the C ABI
_uploaded = {}


def _ds(sched):
    if id(sched) not in _uploaded:
        _uploaded[id(sched)] = (sched, _DeviceSchedule(sched, torch.device("cuda", torch.cuda.current_device())))
    return _uploaded[id(sched)][1]


@pytest.fixture(autouse=True)
def _forget_uploads():
    yield
    _uploaded.clear()


def _k1(sched, xd, arg_bytes, relu_input=False, counters=None, expect=OK, what="K1"):
    """gts_spmm_max_fwd_cluster_f32 -> (out as numpy, the winner record on the device or None); a refused launch: (None, None)
    after the fenced outputs have shown that nothing ran."""
    ds, n = _ds(sched), sched.n_rows
    out, obuf = NF.fenced_empty((n, F), DEV)
    arg, abuf = _fenced_arg((n, F), 1) if arg_bytes else (None, None)
    code = _lib.load().gts_spmm_max_fwd_cluster_f32(*_DeviceSchedule.launch_args(ds), ptr(xd), ptr(out), ptr(arg), arg_bytes,
                                                    1 if relu_input else 0, n, F, ptr(counters), current_stream())
    torch.cuda.synchronize()
    assert code == expect, (what, code)
    ran = expect == OK
    if arg_bytes:
        _arg_checked(arg, abuf, 1, what, written=ran)
    got = _float_checked(out, obuf, what, written=ran)
    if counters is not None:
        assert int(counters.abs().sum()) == 0, f"{what}: counters left non-zero"
    return (got, arg) if ran else (None, None)


def _k2(sched, goutd, arg, counters=None, expect=OK, what="K2"):
    ds, n = _ds(sched), sched.n_rows
    gx, buf = NF.fenced_empty((n, F), DEV)
    code = _lib.load().gts_spmm_max_bwd_cluster_f32(*_DeviceSchedule.launch_args(ds), ptr(goutd), ptr(arg), 1, ptr(gx), n, F,
                                                    ptr(counters), current_stream())
    torch.cuda.synchronize()
    assert code == expect, (what, code)
    got = _float_checked(gx, buf, what, written=expect == OK)
    if counters is not None:
        assert int(counters.abs().sum()) == 0, f"{what}: counters left non-zero"
    return got if expect == OK else None


_refs = {}


def _ref(g, x, relu):
    key = (id(g), id(x), relu)
    if key not in _refs:
        _refs[key] = (g, x, R.max_ref_full(g, x, relu))
    return _refs[key][2]


@pytest.fixture(scope="module", autouse=True)
def _forget_refs():
    yield
    _refs.clear()


def _hold(g, s_in, s_out, x, gout, what, counters=None, relus=(False, True), value_only=True, plain=True):
    """K1 without and with winners, relu_input off and on, then K2 on K1's own winners: value, winner slot and winner source
    against max_ref_full, the gradient against max_bwd_ref, and all of it against the plain kernels on the same inputs.
    Returns {relu: (out, slots, gx)}."""
    xd, goutd = _up(x), _up(gout)
    got = {}
    for relu in relus:
        want, want_src, want_slot = _ref(g, x, relu)
        if value_only:
            out, none = _k1(s_in, xd, 0, relu, counters, what=f"{what}: K1 without winners")
            assert none is None and R.same_bits(out, want), (what, relu)
        out, arg = _k1(s_in, xd, 1, relu, counters, what=f"{what}: K1")
        assert R.same_bits(out, want) and not np.isnan(out).any(), (what, relu)
        slots = _slots(arg)
        assert np.array_equal(slots, want_slot), (what, relu)
        assert np.array_equal(slots_to_sources(g, arg), want_src), (what, relu)
        gx = _k2(s_out, goutd, arg, counters, what=f"{what}: K2")
        assert R.same_bits(gx, R.max_bwd_ref(g, gout, slots)), (what, relu)
        if plain:
            gd = P._dev(g)
            out_p, arg_p = P._k1(gd, xd, 1, relu)
            assert R.same_bits(out, out_p) and torch.equal(arg, arg_p), (what, relu)
            assert R.same_bits(gx, P._k2(gd, goutd, arg)), (what, relu)
        got[relu] = (out, slots, gx)
    return got


def _schedules(c, other_limits=None):
    """(s_in, s_out) of a case: its hand-made schedule and the greedy one of the other CSR (at the default limits)."""
    g = c["g"]
    if c["which"] == "in":
        return c["sched"], C.other_schedule(g, "out", other_limits)
    return C.other_schedule(g, "in", other_limits), c["sched"]


def _features(g, seed):
    return {"integers": R.integers(g.n, F, seed), "gaussian": R.gaussian(g.n, F, seed + 1)}, R.gaussian(g.n, F, seed + 2)


# ---------------------------------------------------------------- pairs
@pytest.mark.parametrize("which", ["in", "out"])
def test_every_ordered_pair_of_degrees_in_one_wave_slot(which):
    """225 pairs of {0 .. 9, 15, 16, 17, 24, 25}, clusters of 1 (with and without edges), 2, 3, 31 and 32 rows, a zero-degree
    last row whose first chunk lies one past a full section, equal pairs at 8 and 9; then three launches give identical bytes."""
    c = C.pair_case(which)
    g = c["g"]
    s_in, s_out = _schedules(c)
    feats, gout = _features(g, 11)
    for kind, x in feats.items():
        _hold(g, s_in, s_out, x, gout, (which, kind))
    x = feats["gaussian"]
    xd, goutd = _up(x), _up(gout)
    runs = []
    for _ in range(3):
        out, arg = _k1(s_in, xd, 1)
        runs.append((out.tobytes(), arg.cpu().numpy().tobytes(), _k2(s_out, goutd, arg).tobytes()))
    assert runs[0] == runs[1] == runs[2]


# ---------------------------------------------------------------- long rows and full lists
def _hub_inputs(c):
    g = c["g"]
    x = R.integers(g.n, F, 21)
    if c["which"] == "in":
        x = C.hub_columns(x, g, "in", c["hubs"][::-1])      # hub 0 last: its columns hold whatever the others share
    return x


def _hold_long(c, what, counters=None, other_limits=None, **kw):
    g = c["g"]
    s_in, s_out = _schedules(c, other_limits)
    x, gout = _hub_inputs(c), R.gaussian(g.n, F, 22)
    got = _hold(g, s_in, s_out, x, gout, what, counters, **kw)
    if c["which"] == "in":      # the unique maximum in the first slot, in the last slot of the last chunk, and a full tie
        deg, cols = c["n_srcs"][0], np.arange(F) % 3
        hub = got[False][1][0]
        assert (hub[cols == 0] == 0).all() and (hub[cols == 1] == deg - 1).all() and (hub[cols == 2] == 0).all(), what
    _hold(g, s_in, s_out, R.gaussian(g.n, F, 23), gout, what, counters, relus=(False,), value_only=False, plain=False)


@pytest.mark.parametrize("which", ["in", "out"])
def test_a_neighbour_list_as_long_as_the_limits_and_as_the_lds_allow(which, lib):
    """One row whose degree is max_srcs (76 in, 60 out; then the largest limit whose two images fit the LDS, computed from
    gts_cluster_lds_bytes), lists of 1, 2, 3, 7, 8, 9 and an odd maximum of neighbours, a cluster at exactly max_edges padded
    edges.  One neighbour more than fits is refused with GTS_ERR_SHAPE before anything runs."""
    top = C.largest_max_srcs(lib, which)
    assert top > C.DEFAULT_LIMITS[which][1]
    for s in (C.DEFAULT_LIMITS[which][1], top):
        c = C.long_case(which, s)
        assert c["sched"].limits[1] == s and C.n_srcs_of(c["sched"])[0] == s
        _hold_long(c, (which, s))
    c = C.long_case(which, top + 1)
    s_in, s_out = _schedules(c)
    x, gout = _hub_inputs(c), R.gaussian(c["g"].n, F, 22)
    if which == "in":
        for arg_bytes in (0, 1):
            assert _k1(s_in, _up(x), arg_bytes, expect=SHAPE) == (None, None)
    else:
        _, arg = _k1(s_in, _up(x), 1)
        assert _k2(s_out, _up(gout), arg, expect=SHAPE) is None


# ---------------------------------------------------------------- records
RECORD_WORDS = [("in", w) for w in (252, 256, 260, 512)] + [("out", w) for w in (248, 256, 264, 512)]


@pytest.mark.parametrize("which,words", RECORD_WORDS)
def test_records_on_both_sides_of_one_piece_and_at_the_largest_size(which, words):
    """Record sizes are multiples of 4 words (8 with tags): the sizes next to 256 and 256 itself, one and two LDS-DMA pieces,
    and 512, the largest a launch takes.  The same schedule with loc_words widened by 4 and by 8 gives the same bits."""
    c = C.record_case(which, words)
    g, sched = c["g"], c["sched"]
    assert sched.layout.words == words
    s_in, s_out = _schedules(c)
    feats, gout = _features(g, 31)
    base = _hold(g, s_in, s_out, feats["gaussian"], gout, (which, words))
    _hold(g, s_in, s_out, feats["integers"], gout, (which, words), value_only=False, plain=False)
    for more in (4, 8):
        wide = sched.with_loc_words(sched.loc_words + more)
        if wide.layout.words > 512:
            continue
        assert wide.layout.words == words + more * (2 if which == "out" else 1)
        pair = (wide, s_out) if which == "in" else (s_in, wide)
        got = _hold(g, *pair, feats["gaussian"], gout, (which, words, more), plain=False)
        for relu in (False, True):
            assert all(R.same_bits(a, b) for a, b in zip(got[relu], base[relu]))


# ---------------------------------------------------------------- cluster counts and dealing
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 7, 8, 9])
def test_fewer_clusters_than_xcd_spans_and_a_few_more(count):
    """1 .. 9 clusters: with fewer than four, some of the eight spans of units are empty; the grid is clamped to 8 and 16
    workgroups.  Static dealing, dealing off the counters and the automatic choice; the counters are zero afterwards."""
    for which in ("in", "out"):
        c = C.count_case(which, count)
        g = c["g"]
        s_in, s_out = _schedules(c)
        assert c["sched"].n_clusters == count
        feats, gout = _features(g, 41)
        for dealing in (0, 1, 2):
            with _options({DEALING: dealing}):
                _hold(g, s_in, s_out, feats["gaussian"], gout, (which, count, dealing), _counters(), plain=dealing == 0)


def _unit_thresholds(lib):
    """name -> number of one-row clusters (units = twice that) on both sides of: the grid of two workgroups per CU, the grid of
    three (short backward launches), the 24 units per CU up to which a backward launch gets three, and the 16 units per
    workgroup from which units are dealt off the counters (read from gts_cluster_uses_counters)."""
    cus = _cus()
    uses = lambda n, bwd: lib.gts_cluster_uses_counters(n, C.ONE_ROW_LIMITS[0], C.ONE_ROW_LIMITS[1], 4, bwd)      # noqa: E731
    sizes = {"grid2": cus, "grid3": 3 * cus // 2, "short": 12 * cus}
    for bwd in (0, 1):
        n = 1
        while not uses(n, bwd) and n < 64 * cus:
            n += 1
        assert uses(n, bwd) and not uses(n - 1, bwd)
        sizes["deal-k2" if bwd else "deal-k1"] = n
    return sizes


@pytest.mark.parametrize("side", [-1, 0, 1])
@pytest.mark.parametrize("edge", ["grid2", "grid3", "short", "deal-k1", "deal-k2"])
def test_unit_counts_on_both_sides_of_every_launch_geometry_threshold(edge, side, lib):
    """One-row clusters, so that thousands of units need only thousands of rows.  Each count under GTS_OPT_CLUSTER_DEALING
    0 (automatic), 1 (counters wherever given) and 2 (never), counters given each time and zero after every launch; the
    dealt count is launched three times into NaN-filled outputs and gives identical bytes."""
    n = _unit_thresholds(lib)[edge] + side
    c = C.one_row_case(n)
    g, s_in, s_out = c["g"], c["s_in"], c["s_out"]
    assert s_in.n_clusters == s_out.n_clusters == n == g.n
    x, gout = R.integers(n, F, 51), R.gaussian(n, F, 52)
    if edge.startswith("deal") and side != 0:
        for s, bwd in ((s_in, 0), (s_out, 1)):
            want = 1 if side > 0 else 0
            if edge == ("deal-k2" if bwd else "deal-k1"):
                assert lib.gts_cluster_uses_counters(n, s.limits[0], s.limits[1], s.loc_words, bwd) == want
    counters = _counters()
    for dealing in (0, 1, 2):
        with _options({DEALING: dealing}):
            _hold(g, s_in, s_out, x, gout, (edge, side, dealing), counters, relus=(False,), value_only=False, plain=dealing == 2)
    if edge.startswith("deal") and side == 0:
        xd, goutd = _up(x), _up(gout)
        runs = []
        for _ in range(3):
            out, arg = _k1(s_in, xd, 1, counters=counters)
            runs.append((out.tobytes(), arg.cpu().numpy().tobytes(), _k2(s_out, goutd, arg, counters).tobytes()))
        assert runs[0] == runs[1] == runs[2]


@pytest.mark.parametrize("which", ["in", "out"])
def test_gathers_two_units_ahead_where_three_images_fit_and_just_beyond(which, lib):
    """GTS_OPT_CLUSTER_RING = 2: the largest neighbour limit whose three images fit the LDS runs two units ahead, the next one
    falls back to one; both give the reference's bits, as does the pair case."""
    fits = C.largest_max_srcs(lib, which, depth=2)
    assert C.DEFAULT_LIMITS[which][1] < fits < C.largest_max_srcs(lib, which)
    with _options({RING: 2}):
        for s in (fits, fits + 1):
            _hold_long(C.long_case(which, s), (which, "ring 2", s), plain=False)
        c = C.pair_case(which)
        feats, gout = _features(c["g"], 11)
        _hold(c["g"], *_schedules(c), feats["gaussian"], gout, (which, "ring 2"), _counters(), plain=False)


@pytest.mark.parametrize("per_cu", [1, 3])
def test_one_and_three_persistent_workgroups_per_cu(per_cu):
    with _options({PER_CU: per_cu}):
        for which in ("in", "out"):
            c = C.pair_case(which)
            feats, gout = _features(c["g"], 11)
            _hold(c["g"], *_schedules(c), feats["gaussian"], gout, (which, per_cu), _counters(), plain=False)
        c = C.one_row_case(2 * _cus() + 3)
        _hold(c["g"], c["s_in"], c["s_out"], R.integers(c["g"].n, F, 51), R.gaussian(c["g"].n, F, 52), ("one row", per_cu),
              _counters(), relus=(False,), plain=False)


@pytest.mark.parametrize("waves", [1, 2, 4, 16])
def test_waves_per_workgroup_and_the_longest_list_they_can_gather(waves, lib):
    """GTS_OPT_CLUSTER_CONSUMERS.  The gathers spread the neighbour ids over the lanes of `waves` waves: valid up to
    max_srcs = 64 * waves, refused one beyond.  One wave: 64 (a record of one piece: one wave fetches one piece); two waves:
    128 for K1, and what the LDS holds (below 128) for K2; four and sixteen waves could gather 256 and more, which no LDS
    plan holds: they run the longest list there is.  Static dealing and dealing off the counters (the dealer is the last
    wave, which with one wave is the only one)."""
    top = {w: C.largest_max_srcs(lib, w) for w in ("in", "out")}
    assert top["out"] < 128 < top["in"] < 256
    runs = {1: [("in", 64, True), ("out", 64, True), ("in", 65, False), ("out", 65, False)],
            2: [("in", 128, True), ("out", top["out"], True), ("in", 129, False)],
            4: [("in", top["in"], True), ("out", top["out"], True)],
            16: [("in", top["in"], True), ("out", top["out"], True)]}[waves]
    with _options({CONSUMERS: waves}):
        for which, s, fits in runs:
            c = C.long_case(which, s, max_edges=256, max_rows=8) if waves == 1 else C.long_case(which, s)
            assert c["sched"].limits[1] == s and C.n_srcs_of(c["sched"])[0] == s
            small = C.ONE_PIECE_LIMITS if waves == 1 else None
            s_in, s_out = _schedules(c, small)
            assert waves > 1 or max(s_in.layout.words, s_out.layout.words) <= 256
            if fits:
                _hold_long(c, (waves, which, s), other_limits=small, plain=False)
                continue
            x, gout = _hub_inputs(c), R.gaussian(c["g"].n, F, 22)
            if which == "in":
                assert _k1(s_in, _up(x), 1, expect=SHAPE) == (None, None)
            else:
                _, arg = _k1(s_in, _up(x), 1)
                assert _k2(s_out, _up(gout), arg, expect=SHAPE) is None
    with _options({CONSUMERS: waves, DEALING: 1}):
        c = C.count_case("in", 9, limits=C.ONE_PIECE_LIMITS["in"] if waves == 1 else None)
        feats, gout = _features(c["g"], 41)
        s_in, s_out = _schedules(c, C.ONE_PIECE_LIMITS if waves == 1 else None)
        assert waves > 1 or max(s_in.layout.words, s_out.layout.words) <= 256
        _hold(c["g"], s_in, s_out, feats["gaussian"], gout, (waves, "dealt"), _counters(), plain=False)


def test_a_record_of_two_pieces_is_refused_by_a_workgroup_of_one_wave():
    """fetch_record: wave p brings piece p.  With GTS_OPT_CLUSTER_CONSUMERS = 1 nobody would bring the second piece of a record
    above 256 words (the tail of loc, all of tag): the launch returns GTS_ERR_SHAPE and touches nothing, as the GAT launch does."""
    k1, k2 = C.record_case("in", 260), C.pair_case("out")
    assert k1["sched"].layout.words == 260 and k2["sched"].layout.words > 256
    with _options({CONSUMERS: 1}):
        x = R.gaussian(k1["g"].n, F, 61)
        for arg_bytes in (0, 1):
            assert _k1(k1["sched"], _up(x), arg_bytes, expect=SHAPE) == (None, None)
        one_piece = C.long_case("in", 64, max_edges=256, max_rows=8)      # 64 neighbours: what one wave can gather
        assert one_piece["sched"].layout.words <= 256
        out, _ = _k1(one_piece["sched"], _up(R.gaussian(one_piece["g"].n, F, 61)), 1)
        assert R.same_bits(out, R.max_ref_full(one_piece["g"], R.gaussian(one_piece["g"].n, F, 61))[0])
    g = k2["g"]
    x, gout = R.gaussian(g.n, F, 62), R.gaussian(g.n, F, 63)
    _, arg = _k1(C.other_schedule(g, "in"), _up(x), 1)
    with _options({CONSUMERS: 1}):
        assert _k2(k2["sched"], _up(gout), arg, expect=SHAPE) is None
    with _options({CONSUMERS: 2}):
        assert R.same_bits(_k2(k2["sched"], _up(gout), arg), R.max_bwd_ref(g, gout, _slots(arg)))


@pytest.mark.parametrize("streaming", [0, 1])
def test_streaming_stores_change_no_bit(streaming):
    with _options({STREAMING: streaming}):
        c = C.pair_case("in")
        feats, gout = _features(c["g"], 11)
        _hold(c["g"], *_schedules(c), feats["gaussian"], gout, ("streaming", streaming), plain=False)


# ---------------------------------------------------------------- values
def test_signed_zeros_nan_and_inf_in_chosen_wave_slots():
    """On the pair case (every placed row shares its wave with a row of another degree): -0.0 against +0.0 (the first wins),
    NaN never wins, a +-Inf maximum is dead, and with relu_input a maximum of +0.0, -0.0 or a negative denormal keeps its value
    and loses its winner."""
    c = C.pair_case("in")
    g = c["g"]
    s_in, s_out = _schedules(c)
    gout = R.gaussian(g.n, F, 71)
    x, rows = R.signed_zeros(g, F, 5)
    got = _hold(g, s_in, s_out, x, gout, "signed zeros")
    bits = got[False][0].view(np.int32)
    assert (bits[rows["neg"]] == np.int32(-2 ** 31)).all() and (bits[rows["neg_then_pos"]] == np.int32(-2 ** 31)).all()
    assert (bits[rows["pos_then_neg"]] == 0).all()
    for v in rows.values():
        assert (got[False][1][v] == 0).all() and (got[True][1][v] == -1).all()
    x, rows = C.nonfinite_in(g, 6)
    got = _hold(g, s_in, s_out, x, gout, "non-finite")
    out, slots, slots_relu = got[False][0], got[False][1], got[True][1]
    for k in ("nan_only", "pos_inf", "neg_inf_all"):
        assert (out[rows[k]].view(np.int32) == 0).all() and (slots[rows[k]] == -1).all(), k
    assert (slots[rows["nan_among"]] >= 0).all() and (slots[rows["nan_among"]] != 1).all()
    assert (slots[rows["last_slot"]] == 24).all() and (slots_relu[rows["last_slot"]] == 24).all()
    assert (out[rows["neg_denormal"]] == np.float32(-1e-40)).all()
    assert (out[rows["pos_zero"]].view(np.int32) == 0).all() and (out[rows["neg_zero"]].view(np.int32) == np.int32(-2 ** 31)).all()
    for k in ("neg_denormal", "pos_zero", "neg_zero"):
        assert (slots[rows[k]] == 1).all() and (slots_relu[rows[k]] == -1).all(), k
    x = np.full((g.n, F), -np.inf, dtype=np.float32)
    got = _hold(g, s_in, s_out, x, gout, "all -Inf")
    assert (got[False][0].view(np.int32) == 0).all() and (got[False][1] == -1).all() and (got[False][2].view(np.int32) == 0).all()


@pytest.mark.parametrize("which", ["in", "out"])
def test_nan_and_inf_gradients_stay_on_the_edges_that_won(which):
    """K2 adds a selected +0.0 for an edge that lost: a NaN or Inf gradient of a destination reaches exactly the sources that
    won there.  Winners of 0xFF everywhere give +0.0 everywhere."""
    c = C.pair_case(which)
    g = c["g"]
    s_in, s_out = _schedules(c)
    x, gout = R.gaussian(g.n, F, 81), R.gaussian(g.n, F, 82)
    _, arg = _k1(s_in, _up(x), 1)
    slots = _slots(arg)
    rng = np.random.default_rng(83)
    hit = rng.permutation(g.n)[:g.n // 3]
    gout[hit[0::3]], gout[hit[1::3]], gout[hit[2::3]] = np.nan, np.inf, -np.inf
    with np.errstate(invalid="ignore"):          # Inf - Inf where both won
        want = R.max_bwd_ref(g, gout, slots)
    touched = np.zeros((g.n, F), dtype=bool)          # sources with an edge, won or lost, to a destination that was hit
    for u in range(g.n):
        d = g.t_indices[g.t_indptr[u]:g.t_indptr[u + 1]]
        touched[u] = np.isin(d, hit).any()
    bad = ~np.isfinite(want)
    assert bad.any() and (touched & ~bad).sum() > bad.sum(), "most edges to a hit destination lost"
    got = _k2(s_out, _up(gout), arg)
    assert R.same_bits(got, want) and np.array_equal(~np.isfinite(got), bad)
    assert R.same_bits(got, P._k2(P._dev(g), _up(gout), arg))
    none = torch.full((g.n, F), 0xFF, dtype=torch.uint8, device=DEV)
    assert (_k2(s_out, _up(gout), none).view(np.int32) == 0).all()


# ---------------------------------------------------------------- batches
@pytest.mark.parametrize("which", ["in", "out"])
def test_concatenated_hand_made_schedules_give_the_members_bits(which):
    """ClusterSchedule.concat of hand-made parts with different loc_words, one of them a single row: the batch's rows hold
    what the members give on their own."""
    lim = C.DEFAULT_LIMITS[which]
    members = [C.count_case(which, 5), C.make_case(which, [[2]], lim, 91)[:2], C.pair_case(which), C.count_case(which, 2)]
    members = [(m["g"], m["sched"]) if isinstance(m, dict) else m for m in members]
    assert len({s.loc_words for _, s in members}) >= 3 and members[1][0].n == 1
    other = "out" if which == "in" else "in"
    offsets = np.concatenate([[0], np.cumsum([g.n for g, _ in members])]).tolist()
    b = gts.batch([g for g, _ in members])
    mine = ClusterSchedule.concat([s for _, s in members], offsets)
    theirs = ClusterSchedule.concat([C.other_schedule(g, other) for g, _ in members], offsets)
    assert mine.n_clusters == sum(s.n_clusters for _, s in members) and mine.n_rows == b.n
    s_in, s_out = (mine, theirs) if which == "in" else (theirs, mine)
    x, gout = R.gaussian(b.n, F, 92), R.gaussian(b.n, F, 93)
    whole = _hold(b, s_in, s_out, x, gout, ("batch", which))
    for (g, s), at in zip(members, offsets):
        m_in, m_out = (s, C.other_schedule(g, "out")) if which == "in" else (C.other_schedule(g, "in"), s)
        part = _hold(g, m_in, m_out, x[at:at + g.n].copy(), gout[at:at + g.n].copy(), ("member", which, at), plain=False)
        for relu in (False, True):
            assert R.same_bits(part[relu][0], whole[relu][0][at:at + g.n])
            assert np.array_equal(part[relu][1], whole[relu][1][at:at + g.n])
            assert R.same_bits(part[relu][2], whole[relu][2][at:at + g.n])


def test_options_are_back_at_their_defaults():
    """Last in the file: nothing above leaves an option of the clustered kernels changed."""
    assert _current_options() == OPTION_DEFAULTS
