"""The plain CSR reducers (csrc/gts_spmm.hip: K1 max forward, K2 max backward, K3/K4 sum family; the row walk of
csrc/gts_rows.h they share with the GAT kernels) against the per-row references of tests/spmm_ref.py, bit for bit, on a
real MI355X, at the degree, width and grid edges where they can go wrong: in- and out-degrees on both sides of every
chunk remainder and of the uint8 / int32 winner record (0 .. 10, 15 - 17, 23 - 25, 63 - 65, 127, 128, 253 - 256, 300) with
empty rows and hubs in one wave, every (VEC, LPR) instantiation, widths whose last lane group or last column pass is
partly idle, row counts on both sides of a workgroup and of the grids 8, 9 and 18, both tuning options, all sixteen
flag combinations of the sum family, signed zeros, NaN and Inf.

The kernels are called through the C ABI, never through the routing wrappers of gts.ops, so F = 256 runs the plain
kernels too.  Every output is carved from a fenced buffer: after every launch the pads are intact and every element of
the output was written.  No tolerance anywhere: the kernels promise the references' order of operations
(-ffp-contract=off).  The references and the case lists are validated on the CPU in tests/test_spmm_ref_host.py."""
import math

import numpy as np
import pytest
import torch

from gts import _lib
from gts.ops import current_stream, ptr
from tests import nonfinite_ref as NF
from tests import spmm_ref as R
from tests.helpers import slots_to_sources

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPT_ROWS_PER_WAVE = _lib.const("GTS_OPT_SPMM_ROWS_PER_WAVE")
OPT_STREAMING = _lib.const("GTS_OPT_SPMM_STREAMING")
OPTION_DEFAULTS = {OPT_ROWS_PER_WAVE: 0, OPT_STREAMING: -1}
# winner fences: neither a slot (<= 253 under uint8, >= 0 under int32) nor "no winner" (0xFF, -1)
ARG_FENCE = {1: 0xFE, 4: -0x21524111}
ARG_DTYPE = {1: torch.uint8, 4: torch.int32}
ARG_NONE = {1: 0xFF, 4: -1}
PAD = 64


@pytest.fixture(scope="module", autouse=True)
def lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_lib


# ---------------------------------------------------------------- fenced launches through the C ABI
_device_graphs = {}


def _dev(g):
    if id(g) not in _device_graphs:
        _device_graphs[id(g)] = (g, g.to(DEV))
    return _device_graphs[id(g)][1]


@pytest.fixture(autouse=True)
def _forget_large_graphs():
    """The graphs of the largest row counts (up to 1.6 M edges) are used by one test each: not kept, on either side."""
    yield
    for key in [k for k, (g, _) in _device_graphs.items() if g.number_of_edges() > 200_000]:
        del _device_graphs[key]
    R.forget_graphs_above(200_000)


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fenced_arg(shape, arg_bytes):
    n = math.prod(shape)
    back = max(n, PAD) + (-(PAD + n + max(n, PAD))) % PAD
    buf = torch.full((PAD + n + back,), ARG_FENCE[arg_bytes], dtype=ARG_DTYPE[arg_bytes], device=DEV)
    return buf[PAD:PAD + n].view(shape), buf


def _arg_checked(arg, buf, arg_bytes, what, written=True):
    fence, n = ARG_FENCE[arg_bytes], arg.numel()
    assert bool((buf[:PAD] == fence).all()) and bool((buf[PAD + n:] == fence).all()), f"{what}: wrote outside its winners"
    if written:
        assert not bool((arg == fence).any()), f"{what}: left winners unwritten"
    else:
        assert bool((arg == fence).all()), f"{what}: wrote winners it should not have"


def _float_checked(out, buf, what, written=True):
    assert NF.fence_intact(buf, out), f"{what}: wrote outside its output"
    untouched = out.view(torch.int32) == NF.FENCE_BITS
    if written:
        assert not bool(untouched.any()), f"{what}: left {int(untouched.sum())} elements unwritten"
    else:
        assert bool(untouched.all()), f"{what}: wrote an output it should not have"
    return out.cpu().numpy()


def _k1(gd, x, arg_bytes, relu_input=False):
    """gts_spmm_max_fwd_f32 -> (out as numpy, the winner record on the device or None)."""
    d, (n, f) = gd.dev(), x.shape
    out, obuf = NF.fenced_empty((n, f), DEV)
    arg, abuf = _fenced_arg((n, f), arg_bytes) if arg_bytes else (None, None)
    _lib.check(_lib.load().gts_spmm_max_fwd_f32(ptr(d.indptr), ptr(d.indices), ptr(x), ptr(out), ptr(arg), arg_bytes,
                                                1 if relu_input else 0, n, f, current_stream()), "gts_spmm_max_fwd_f32")
    if arg_bytes:
        _arg_checked(arg, abuf, arg_bytes, "K1")
    return _float_checked(out, obuf, "K1"), arg


def _k2(gd, gout, arg, relu_src=None):
    d, (n, f) = gd.dev(), gout.shape
    gx, buf = NF.fenced_empty((n, f), DEV)
    _lib.check(_lib.load().gts_spmm_max_bwd_f32(ptr(d.t_indptr), ptr(d.t_indices), ptr(d.t_slot), ptr(gout), ptr(arg),
                                                arg.element_size(), ptr(relu_src), ptr(gx), n, f, current_stream()),
               "gts_spmm_max_bwd_f32")
    return _float_checked(gx, buf, "K2")


def _ksum(gd, x, transposed=False, div_in=None, div_out=None, add_self=False, accum=None):
    d, (n, f) = gd.dev(), x.shape
    indptr, indices = (d.t_indptr, d.t_indices) if transposed else (d.indptr, d.indices)
    out, buf = NF.fenced_empty((n, f), DEV)
    _lib.check(_lib.load().gts_spmm_sum_f32(ptr(indptr), ptr(indices), ptr(x), ptr(out), ptr(div_in), ptr(div_out), ptr(accum),
                                            1 if add_self else 0, n, f, current_stream()), "gts_spmm_sum_f32")
    return _float_checked(out, buf, "sum")


def _slots(arg):
    """The device's winner record as slots with -1 = none (what tests/spmm_ref.py: max_bwd_ref takes)."""
    s = arg.cpu().numpy().astype(np.int64)
    s[s == ARG_NONE[arg.element_size()]] = -1
    return s


def _hold_k1(g, xd, x, relu_input, what):
    """K1 with winners of the graph's own width: value, winners as source ids and as slots.  Returns the device record."""
    want, want_src, want_slot = R.max_ref_full(g, x, relu_input)
    out, arg = _k1(_dev(g), xd, g.arg_bytes, relu_input)
    assert arg.dtype == ARG_DTYPE[g.arg_bytes]
    assert R.same_bits(out, want) and not np.isnan(out).any(), what
    assert np.array_equal(slots_to_sources(g, arg), want_src), what
    assert np.array_equal(_slots(arg), want_slot), what       # a later duplicate of the same source is another slot
    return arg, want


def _hold_k2(g, goutd, gout, arg, what, relu_srcd=None, relu_src=None):
    got = _k2(_dev(g), goutd, arg, relu_srcd)
    assert R.same_bits(got, R.max_bwd_ref(g, gout, _slots(arg), relu_src)) and not np.isnan(got).any(), what


def _sum_operands(c, flags, div_kind):
    """Host operands of one flag combination; 'random' divides the rows by other values than the sources."""
    div_in, div_out, add_self, accum = flags
    div = c["divisors"][div_kind]
    return dict(div_in=div if div_in else None, div_out=(div if div_kind == "deg" else div[::-1].copy()) if div_out else None,
                add_self=bool(add_self), accum=c["accum"] if accum else None)


def _hold_sum(g, xd, x, transposed, host, what):
    dev = {k: (_up(v) if isinstance(v, np.ndarray) else v) for k, v in host.items()}
    got = _ksum(_dev(g), xd, transposed, **dev)
    indptr, indices = (g.t_indptr, g.t_indices) if transposed else (g.indptr, g.indices)
    assert R.same_bits(got, R.sum_ref(indptr, indices, x, **host)), what


WIDTH_CASES = [(w, name, t) for w in R.WIDTHS for name in R.LADDERS for t in (False, True)]


# ---------------------------------------------------------------- every width on the ladder
@pytest.mark.parametrize("width,name,transpose", WIDTH_CASES)
def test_max_forward_and_backward_at_every_width(width, name, transpose):
    c = R.width_inputs(width, name, transpose)
    g, gout = c["g"], c["gout"]
    goutd = _up(gout)
    for kind in ("integers", "gaussian"):
        x, xd = c[kind], _up(c[kind])
        arg, want = _hold_k1(g, xd, x, False, kind)
        out_only, none = _k1(_dev(g), xd, 0)                              # arg_bytes = 0, arg = NULL
        assert none is None and R.same_bits(out_only, want), kind
        arg_relu, _ = _hold_k1(g, xd, x, True, kind + " relu_input")
        _hold_k2(g, goutd, gout, arg, kind)
        _hold_k2(g, goutd, gout, arg_relu, kind + " relu_input")
        _hold_k2(g, goutd, gout, arg, kind + " relu_src", xd, x)


@pytest.mark.parametrize("width,name,transpose", WIDTH_CASES)
def test_sum_family_flags_at_every_width(width, name, transpose):
    """All sixteen combinations of (div_in, div_out, add_self, accum), over the in-CSR and the out-CSR."""
    c = R.width_inputs(width, name, transpose)
    g = c["g"]
    for kind in ("integers", "gaussian"):
        x, xd = c[kind], _up(c[kind])
        for transposed in (False, True):
            for flags in R.SUM_FLAGS:
                for div_kind in (("deg", "random") if flags[0] or flags[1] else ("deg",)):
                    _hold_sum(g, xd, x, transposed, _sum_operands(c, flags, div_kind), (kind, transposed, flags, div_kind))


# ---------------------------------------------------------------- every row count
def _row_count_case(n, width, transpose=False):
    g = R.ladder(n, "u8", n, transpose)
    return dict(g=g, gaussian=R.gaussian(n, width, n + 1), integers=R.integers(n, width, n + 2), gout=R.gaussian(n, width, n + 3),
                accum=R.gaussian(n, width, n + 4), divisors={"deg": R.divisors(g, "deg", 0), "random": R.divisors(g, "random", n + 5)})


def _hold_row_count(n, width):
    """K1, K2 (on the transposed ladder: its out-CSR rows carry the degrees) and the sum with all four flags, n rows."""
    c = _row_count_case(n, width)
    g, x = c["g"], c["gaussian"]
    xd = _up(x)
    _hold_k1(g, xd, x, False, ("K1", n))
    _hold_sum(g, xd, x, False, _sum_operands(c, (1, 1, 1, 1), "random"), ("sum", n))
    c = _row_count_case(n, width, transpose=True)
    g, x, gout = c["g"], c["integers"], c["gout"]
    xd, goutd = _up(x), _up(gout)
    arg, _ = _hold_k1(g, xd, x, False, ("K1 transposed", n))
    _hold_k2(g, goutd, gout, arg, ("K2", n), xd, x)
    _hold_k2(g, goutd, gout, arg, ("K2 unmasked", n))


@pytest.mark.parametrize("width", R.ROW_COUNT_WIDTHS)
def test_row_counts_around_a_workgroup_and_the_grids_8_9_18(width):
    """One width per (VEC, LPR); each kernel's own rows per workgroup R (K1 walks 2 rows per wave, K2 and the sums 1):
    1, R - 1, R, R + 1, 7R + 1, 8R, 9R - 1, 17R + 3 rows."""
    counts = []
    for seq in (R.SEQ_K1, R.SEQ_K2, R.SEQ_SUM):
        counts += [n for n in R.row_counts(R.geometry(1, width, seq)[2]) if n not in counts]
    for n in counts:
        _hold_row_count(n, width)


# ---------------------------------------------------------------- the two tuning options
def _options():
    return {k: _lib.load().gts_get_option(k) for k in OPTION_DEFAULTS}


@pytest.mark.parametrize("rows_per_wave", R.OPTION_ROWS_PER_WAVE)
@pytest.mark.parametrize("width", R.OPTION_WIDTHS)
def test_rows_per_wave_and_streaming_change_no_bit(width, rows_per_wave):
    """GTS_OPT_SPMM_ROWS_PER_WAVE x GTS_OPT_SPMM_STREAMING (bit 0: store_nt of out / gx, bit 1: load_nt of relu_src), at
    the row counts of that many rows per wave: every result equals the reference, and therefore every other."""
    lib = _lib.load()
    before = _options()
    assert before == OPTION_DEFAULTS
    try:
        assert lib.gts_set_option(OPT_ROWS_PER_WAVE, rows_per_wave) == 0
        for n in R.row_counts(R.geometry(1, width, 0, rows_per_wave)[2]):
            c = _row_count_case(n, width)
            g, x, gout = c["g"], c["gaussian"], c["gout"]
            xd, goutd = _up(x), _up(gout)
            want, _, want_slot = R.max_ref_full(g, x)
            want_gx = R.max_bwd_ref(g, gout, want_slot, x)
            for streaming in R.OPTION_STREAMING:
                assert lib.gts_set_option(OPT_STREAMING, streaming) == 0
                out, arg = _k1(_dev(g), xd, g.arg_bytes)
                assert R.same_bits(out, want) and np.array_equal(_slots(arg), want_slot), (n, streaming)
                assert R.same_bits(_k2(_dev(g), goutd, arg, xd), want_gx), (n, streaming)
            _hold_sum(g, xd, x, False, _sum_operands(c, (1, 1, 1, 1), "random"), ("sum", n))
    finally:
        for k, v in before.items():
            lib.gts_set_option(k, v)
    assert _options() == OPTION_DEFAULTS


# ---------------------------------------------------------------- the winner-width boundary
@pytest.mark.parametrize("width", R.HUB_WIDTHS)
@pytest.mark.parametrize("deg", R.HUB_DEGREES)
def test_winner_record_on_both_sides_of_254(deg, width):
    """uint8 up to in-degree 254 (0xFF = none, so the last slot reads 253), int32 from 255 (the last slot reads 254, and
    255 at degree 256): the unique maximum in the first slot, in the last slot, and a full tie, by column."""
    g, x = R.hub_graph(deg), R.hub_features(deg, width)
    assert g.arg_bytes == (1 if deg <= 254 else 4)
    xd = _up(x)
    arg, _ = _hold_k1(g, xd, x, False, deg)
    hub = arg[0].cpu().numpy().astype(np.int64)
    cols = np.arange(width) % 3
    assert (hub[cols == 0] == 0).all() and (hub[cols == 1] == deg - 1).all() and (hub[cols == 2] == 0).all()
    gout = R.gaussian(g.n, width, deg)
    _hold_k2(g, _up(gout), gout, arg, deg)
    _hold_k2(g, _up(gout), gout, arg, deg, xd, x)
    # the hub's gradient alone: it lands on exactly the source that won, first slot -> node 1, last slot -> node deg
    only = np.zeros_like(gout)
    only[0] = np.abs(gout[0]) + 1
    want = np.zeros_like(gout)
    want[1, cols != 1] = only[0, cols != 1]
    want[deg, cols == 1] = only[0, cols == 1]
    assert R.same_bits(_k2(_dev(g), _up(only), arg), want)


# ---------------------------------------------------------------- value classes
def _value_graph():
    return R.ladder(R.VALUE_ROWS, "u8", seed=3)


def _hold_value_classes(g, x, width):
    c = dict(accum=R.gaussian(g.n, width, 11), divisors={"deg": R.divisors(g, "deg", 0), "random": R.divisors(g, "random", 12)})
    gout = R.gaussian(g.n, width, 13)
    xd, goutd = _up(x), _up(gout)
    arg, out = _hold_k1(g, xd, x, False, "plain")
    arg_relu, _ = _hold_k1(g, xd, x, True, "relu_input")
    for record in (arg, arg_relu):
        _hold_k2(g, goutd, gout, record, "K2")
        _hold_k2(g, goutd, gout, record, "K2 relu_src", xd, x)
    for flags in R.SUM_FLAGS:
        _hold_sum(g, xd, x, False, _sum_operands(c, flags, "random"), flags)
    for flags in ((0, 0, 0, 0), (1, 1, 1, 1)):
        _hold_sum(g, xd, x, True, _sum_operands(c, flags, "deg"), flags)
    return out, _slots(arg), _slots(arg_relu)


@pytest.mark.parametrize("width", R.VALUE_WIDTHS)
def test_signed_zeros_keep_their_sign(width):
    g = _value_graph()
    x, rows = R.signed_zeros(g, width, 5)
    out, slots, slots_relu = _hold_value_classes(g, x, width)
    bits = out.view(np.int32)
    assert (bits[rows["neg"]] == np.int32(-2 ** 31)).all() and (bits[rows["neg_then_pos"]] == np.int32(-2 ** 31)).all()
    assert (bits[rows["pos_then_neg"]] == 0).all()
    for v in rows.values():                 # a zero wins like any other maximum, and is no winner once x is a ReLU output
        assert (slots[v] == 0).all() and (slots_relu[v] == -1).all()


@pytest.mark.parametrize("width", R.VALUE_WIDTHS)
def test_nan_and_inf_neighbours(width):
    g = _value_graph()
    x, rows = R.nonfinite(g, width, 6)
    out, slots, slots_relu = _hold_value_classes(g, x, width)
    for k in ("nan_only", "pos_inf", "neg_inf_single"):
        assert (out[rows[k]].view(np.int32) == 0).all() and (slots[rows[k]] == -1).all(), k
    assert (slots[rows["nan_among"]] >= 0).all() and (slots[rows["nan_among"]] != 1).all()
    assert (slots[rows["last_slot"]] == 253).all() and (slots_relu[rows["last_slot"]] == 253).all()


# ---------------------------------------------------------------- nothing to do
def test_empty_and_rejected_calls_launch_nothing():
    """n = 0 is GTS_OK, arg_bytes = 2 GTS_ERR_ARGKIND, n_feat = 0 GTS_ERR_SHAPE; none of them touches an output, and the
    next real launch reports a clean status (the library's status is hipGetLastError)."""
    lib = _lib.load()
    c = R.width_inputs(12, "u8")
    g, f = c["g"], 12
    d = _dev(g).dev()
    xd, st = _up(c["gaussian"]), current_stream()
    ok, argkind, shape = _lib.const("GTS_OK"), _lib.const("GTS_ERR_ARGKIND"), _lib.const("GTS_ERR_SHAPE")
    out, obuf = NF.fenced_empty((g.n, f), DEV)
    arg, abuf = _fenced_arg((g.n, f), 1)
    arg4, abuf4 = _fenced_arg((g.n, f), 4)

    def fwd(arg_, arg_bytes, n, n_feat):
        return lib.gts_spmm_max_fwd_f32(ptr(d.indptr), ptr(d.indices), ptr(xd), ptr(out), ptr(arg_), arg_bytes, 0, n, n_feat, st)

    def bwd(arg_, arg_bytes, n, n_feat):
        return lib.gts_spmm_max_bwd_f32(ptr(d.t_indptr), ptr(d.t_indices), ptr(d.t_slot), ptr(xd), ptr(arg_), arg_bytes, None,
                                        ptr(out), n, n_feat, st)

    def total(n, n_feat):
        return lib.gts_spmm_sum_f32(ptr(d.indptr), ptr(d.indices), ptr(xd), ptr(out), None, None, None, 0, n, n_feat, st)

    assert fwd(arg, 1, 0, f) == ok and fwd(arg4, 4, 0, f) == ok and fwd(None, 0, 0, f) == ok
    assert bwd(arg, 1, 0, f) == ok and bwd(arg4, 4, 0, f) == ok and total(0, f) == ok
    assert fwd(arg, 2, g.n, f) == argkind and bwd(arg, 2, g.n, f) == argkind and bwd(arg, 0, g.n, f) == argkind
    assert fwd(arg, 1, g.n, 0) == shape and bwd(arg, 1, g.n, 0) == shape and total(g.n, 0) == shape
    torch.cuda.synchronize()
    _float_checked(out, obuf, "rejected call", written=False)
    _arg_checked(arg, abuf, 1, "rejected call", written=False)
    _arg_checked(arg4, abuf4, 4, "rejected call", written=False)
    _hold_k1(g, xd, c["gaussian"], False, "after the rejected calls")     # _lib.check: launch_status() is clean


def test_options_are_back_at_their_defaults():
    """Last in the file: nothing above leaves GTS_OPT_SPMM_ROWS_PER_WAVE or GTS_OPT_SPMM_STREAMING changed."""
    assert _options() == OPTION_DEFAULTS
