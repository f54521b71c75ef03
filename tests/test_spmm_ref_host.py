"""The cases and references of tests/test_gpu_spmm_edges.py, validated on the CPU (tests/spmm_ref.py): the case lists
cover the geometries they claim, the per-row references agree bit for bit with the independently written oracle
(oracle/torch_ref.py), the fp32 sum stays inside a derived bound of its float64 twin, and the inputs tell every
deliberately wrong kernel from the right one."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import graph_ref, torch_ref
from tests import spmm_ref as R
from tests.helpers import HAND_EDGES, HAND_X

LPRS = (1, 2, 4, 8, 16, 32, 64)
SEQS = (R.SEQ_K1, R.SEQ_K2, R.SEQ_SUM)


def _wide(widths=R.WIDTHS):
    return [w for w in widths if R.geometry(1, w, R.SEQ_K1)[1] == 64]


# ---------------------------------------------------------------- the case lists cover what they claim
def test_geometry_restates_the_launch_code():
    assert R.geometry(300, 256, R.SEQ_K1) == (4, 64, 8, 38)         # one wave per row, 2 rows per wave, 4 waves
    assert R.geometry(300, 256, R.SEQ_K2) == (4, 64, 4, 75)
    assert R.geometry(257, 20, R.SEQ_SUM) == (4, 8, 32, 9)          # 5 float4 columns -> 8 lanes, 8 rows per wave step
    assert R.geometry(300, 3, R.SEQ_K1) == (1, 4, 128, 3)
    assert R.geometry(10 ** 7, 4, R.SEQ_SUM)[2] == 64 * 4 * 4       # pick_seq lengthens the walk from 8192 waves per step
    assert R.geometry(10 ** 6, 4, R.SEQ_SUM)[2] == 64 * 1 * 4
    assert R.geometry(300, 256, R.SEQ_K1, rows_per_wave=3)[2] == 12
    assert [R.tile_of(b, 9) for b in range(9)] == [0, 2, 3, 4, 5, 6, 7, 8, 1]


def test_every_lane_group_class_occurs():
    pairs = {(v, l) for v in (1, 4) for l in LPRS}
    assert {R.geometry(1, w, R.SEQ_K1)[:2] for w in R.WIDTHS} == pairs
    assert sorted(R.geometry(1, w, R.SEQ_K1)[:2] for w in R.ROW_COUNT_WIDTHS) == sorted(pairs)      # each exactly once
    assert {R.geometry(1, w, 0)[0] for w in R.WIDTHS_VEC1} == {1} and {R.geometry(1, w, 0)[0] for w in R.WIDTHS_VEC4} == {4}
    for vec, widths in ((1, R.WIDTHS_VEC1), (4, R.WIDTHS_VEC4)):
        cols = [(w // vec, R.geometry(1, w, 0)[1]) for w in widths]
        assert any(c % lpr != 0 for c, lpr in cols), "no width whose last lane group is partly inactive"
        assert any(c > lpr and c % lpr == 1 for c, lpr in cols), "no column pass with a single active lane group"
    assert {R.geometry(1, w, 0)[1] for w in R.OPTION_WIDTHS} == {1, 8, 64}


def test_wave_per_row_widths_meet_every_chunk_remainder():
    """LPR == 64: each count 1..7 is its own instantiation of the chunk body; every remainder occurs with and without a
    full chunk of 8 before it, in the rows K1 and the sums walk (in-CSR) and in those K2 walks (out-CSR)."""
    seen = {"in": set(), "out": set()}
    for w in _wide():
        for name in R.LADDERS:
            for transpose in (False, True):
                g = R.width_graph(w, name, transpose)
                for which, ptr in (("in", g.indptr), ("out", g.t_indptr)):
                    seen[which] |= {(int(d) % 8, bool(d >= 8)) for d in np.diff(ptr)}
    want = {(r, full) for r in range(8) for full in (False, True)}
    assert seen["in"] == want and seen["out"] == want
    # and the ladder rows themselves hit the exact multiples the random degrees only meet by luck
    for name, degrees in R.LADDERS.items():
        met = set().union(*(np.diff(R.width_graph(w, name).indptr).tolist() for w in _wide()))
        assert {0, 8, 16, 24, 64, 128} <= met and {d for d in degrees if d >= 253} <= met
        assert all(R.width_graph(w, name).max_in_degree == max(degrees) for w in _wide())


def test_rows_of_very_different_degree_share_a_wave():
    """LPR < 64: an empty row and a 254-edge row sit in one wave (32 and 64 rows per wave hold the whole ladder)."""
    for w in (1, 2, 4, 8):
        lpr = R.geometry(1, w, 0)[1]
        g = R.width_graph(w, "u8")
        deg = np.diff(g.indptr)
        waves = [set(deg[i:i + 64 // lpr].tolist()) for i in range(0, g.n, 64 // lpr)]
        assert any({0, 254} <= s for s in waves), w


def test_row_counts_meet_every_grid_class():
    grids = set()
    for w in R.ROW_COUNT_WIDTHS:
        for seq in SEQS:
            rows = R.geometry(1, w, seq)[2]
            counts = R.row_counts(rows)
            assert all(R.geometry(n, w, seq)[2] == rows for n in counts)
            got = [R.geometry(n, w, seq)[3] for n in counts]
            assert got[-5:] == [2, 8, 8, 9, 18] and set(got[:-5]) == {1}
            classes = {(g >> 3 == 0, g & 7 == 0) for g in got}
            assert classes == {(True, False), (False, True), (False, False)}      # q = 0; q >= 1 with r = 0; with r != 0
            grids |= set(got)
    for w in R.OPTION_WIDTHS:
        for seq in R.OPTION_ROWS_PER_WAVE:
            rows = R.geometry(1, w, 0, seq)[2]
            assert rows == (64 // R.geometry(1, w, 0)[1]) * seq * 4
            grids |= {R.geometry(n, w, 0, seq)[3] for n in R.row_counts(rows)}
    for w in R.WIDTHS:
        n = R.width_graph(w, "u8").n
        grids |= {R.geometry(n, w, seq)[3] for seq in SEQS}
    assert {1, 2, 3, 5, 8, 9, 18} <= grids
    for grid in grids:
        assert sorted(R.tile_of(b, grid) for b in range(grid)) == list(range(grid)), grid


def test_small_ladders_keep_their_extremes():
    for name, degrees in R.LADDERS.items():
        for n in (2, 3, 5, 9, 11, 17, 23):
            deg = np.diff(R.ladder(n, name, seed=n).indptr)
            assert 0 in deg and deg.max() == max(degrees)
            above = {int(d) % 8 for d in deg if d > 8}
            assert len(above) >= min(n - 2, 5), (name, n, sorted(deg))
        assert R.ladder(1, name, seed=1).max_in_degree == max(degrees)
        g = R.ladder(400, name, seed=2)
        assert set(np.diff(g.indptr).tolist()) == set(degrees)
        assert (g.src == g.dst).any() and np.unique(np.stack([g.src, g.dst]), axis=1).shape[1] < g.src.size
        assert R.ladder(400, name, seed=2, transpose=True).max_out_degree == max(degrees)


# ---------------------------------------------------------------- two independently written references agree
def _tgraph(g):
    return torch_ref.TGraph(graph_ref.RefGraph(g.src, g.dst, g.n))


def _oracle_cases():
    import gts
    src, dst = map(np.array, zip(*HAND_EDGES))
    yield "hand", gts.Graph(src, dst, 6), {"hand": HAND_X, "gaussian": R.gaussian(6, 2, 1)}
    for w, name, transpose in ((5, "u8", False), (5, "i32", False), (28, "i32", True), (256, "u8", False), (65, "i32", True)):
        x = R.width_inputs(w, name, transpose)
        yield f"{w}-{name}-{transpose}", x["g"], {k: x[k] for k in ("integers", "gaussian")}
    g = R.ladder(R.VALUE_ROWS, "u8", seed=3)
    yield "values", g, {"signed_zeros": R.signed_zeros(g, 3, 5)[0], "nonfinite": R.nonfinite(g, 3, 6)[0]}


def test_references_equal_the_oracle_bit_for_bit():
    for what, g, feats in _oracle_cases():
        tg = _tgraph(g)
        for kind, x in feats.items():
            out, arg = torch_ref.spmm_max_with_arg(tg, torch.from_numpy(x))
            mine, src = R.max_ref(g, x)
            assert R.same_bits(mine, out) and not np.isnan(mine).any(), (what, kind)
            assert np.array_equal(src, arg.numpy()), (what, kind)
            deg = np.diff(g.indptr).astype(np.float32)
            xt = torch.from_numpy(x)
            with np.errstate(all="ignore"):
                assert R.same_bits(R.sum_ref(g.indptr, g.indices, x), torch_ref.spmm_sum(tg, xt)), (what, kind)
                assert R.same_bits(R.sum_ref(g.indptr, g.indices, x, div_out=np.maximum(deg, 1)), torch_ref.spmm_mean(tg, xt))
                assert R.same_bits(R.sum_ref(g.indptr, g.indices, x, div_out=deg + 1, add_self=True), torch_ref.spmm_gcn(tg, xt))
                # the oracle's backward of a sum is its sum over the out-CSR
                assert R.same_bits(R.sum_ref(g.t_indptr, g.t_indices, x),
                                   torch_ref.seq_spmm_sum(tg.t_indptr, tg.t_indices, tg.t_deg, xt)), (what, kind)


def test_max_backward_equals_the_oracles_gradient_on_integers():
    for w, name, transpose in ((5, "u8", False), (28, "i32", True), (256, "i32", False)):
        c = R.width_inputs(w, name, transpose)
        g, x = c["g"], c["integers"]
        gout = R.integers(g.n, w, w + 11)
        xr = torch.from_numpy(x).requires_grad_(True)
        torch_ref.spmm_max(_tgraph(g), xr).backward(torch.from_numpy(gout))
        slots = R.max_ref(g, x, slots=True)[1]
        assert R.same_bits(R.max_bwd_ref(g, gout, slots), xr.grad)
        assert R.same_bits(R.max_bwd_ref(g, gout, slots, relu_src=x), torch.where(xr.detach() > 0, xr.grad, torch.zeros(())))
        # relu_input: the record of the fused form routes what the masked form does when x is a ReLU output
        relu = np.maximum(x, 0)
        fused = R.max_bwd_ref(g, gout, R.max_ref(g, relu, relu_input=True, slots=True)[1])
        xr = torch.from_numpy(x).requires_grad_(True)
        torch_ref.spmm_max(_tgraph(g), torch.relu(xr)).backward(torch.from_numpy(gout))
        assert R.same_bits(fused, xr.grad)


def test_slots_and_sources_name_the_same_edge():
    c = R.width_inputs(12, "i32")
    g = c["g"]
    out_a, src = R.max_ref(g, c["integers"])
    out_b, slot = R.max_ref(g, c["integers"], slots=True)
    assert R.same_bits(out_a, out_b) and np.array_equal(src == -1, slot == -1)
    pos = g.indptr[:-1, None].astype(np.int64) + slot
    assert np.array_equal(g.indices[pos[slot >= 0]], src[slot >= 0])


@pytest.mark.parametrize("flags", R.SUM_FLAGS)
def test_fp32_sum_is_inside_the_derived_bound_of_its_fp64_twin(flags):
    """One rounding of at most 2^-24 relative per add or divide, on a chain of at most deg + 3 operations, each acting
    on a partial sum no larger than S (the sum of the absolute terms carried through the same divisions, plus |accum|):
    |fp32 - fp64| <= (deg + 3) 2^-24 S to first order; the bar is twice that, (deg + 4) 2^-23 S.  Derived, not measured,
    and it holds the reference, not the kernel (which is held to the reference's bits)."""
    div_in, div_out, add_self, accum = flags
    for w, name, transpose in ((5, "i32", False), (64, "u8", True), (260, "i32", False)):
        c = R.width_inputs(w, name, transpose)
        g, x = c["g"], c["gaussian"]
        for indptr, indices in ((g.indptr, g.indices), (g.t_indptr, g.t_indices)):
            kw = dict(div_in=c["divisors"]["random"] if div_in else None, div_out=c["divisors"]["deg"] if div_out else None,
                      add_self=bool(add_self))
            got = R.sum_ref(indptr, indices, x, accum=c["accum"] if accum else None, **kw)
            want = R.sum_ref64(indptr, indices, x, accum=c["accum"] if accum else None, **kw)
            size = R.sum_ref64(indptr, indices, np.abs(x), accum=np.abs(c["accum"]) if accum else None, **kw)
            deg = np.diff(indptr)[:, None]
            assert (np.abs(got.astype(np.float64) - want) <= (deg + 4) * 2.0 ** -23 * size).all()


# ---------------------------------------------------------------- the generators place what they say
def test_value_class_rows_are_where_the_generators_say():
    g = R.ladder(R.VALUE_ROWS, "u8", seed=3)
    assert g.arg_bytes == 1
    for f in R.VALUE_WIDTHS:
        x, rows = R.signed_zeros(g, f, 5)
        out, src = R.max_ref(g, x)
        bits = out.view(np.int32)
        assert (bits[rows["neg"]] == np.int32(-2 ** 31)).all() and (bits[rows["neg_then_pos"]] == np.int32(-2 ** 31)).all()
        assert (bits[rows["pos_then_neg"]] == 0).all()
        for k in rows:      # a zero maximum wins like any other: the first slot
            assert (src[rows[k]] == g.indices[g.indptr[rows[k]]]).all()
        assert (R.max_ref(g, x, relu_input=True)[1][list(rows.values())] == -1).all()
        assert 0.2 < float((bits == np.int32(-2 ** 31)).mean()) < 0.8

        x, rows = R.nonfinite(g, f, 6)
        out, slot = R.max_ref(g, x, slots=True)
        assert not np.isnan(out).any() and not np.isinf(out).any()
        for k in ("nan_only", "pos_inf", "neg_inf_single"):
            assert (out[rows[k]].view(np.int32) == 0).all() and (slot[rows[k]] == -1).all(), k
        v = rows["nan_among"]
        u = g.indices[g.indptr[v]:g.indptr[v + 1]]
        assert np.isnan(x[u[1]]).all() and (slot[v] != 1).all() and (slot[v] >= 0).all()
        assert np.array_equal(out[v], np.max(x[np.delete(u, 1)], axis=0))
        v = rows["last_slot"]
        u = g.indices[g.indptr[v]:g.indptr[v + 1]]
        assert u.size == 254 and (x[u[:-1]] <= 0).all() and (x[u[-1]] > 0).all() and (slot[v] == 253).all()
        assert (R.max_ref(g, x, relu_input=True, slots=True)[1][v] == 253).all()
        with np.errstate(all="ignore"):
            s = R.sum_ref(g.indptr, g.indices, x)
        assert np.isnan(s[rows["nan_only"]]).all() and np.isnan(s).mean() < 0.5 and np.isinf(s).any()


def test_hub_columns_win_where_they_should():
    for deg in R.HUB_DEGREES:
        g = R.hub_graph(deg)
        for f in R.HUB_WIDTHS:
            x = R.hub_features(deg, f)
            out, slot = R.max_ref(g, x, slots=True)
            cols = np.arange(f) % 3
            assert (slot[0, cols == 0] == 0).all() and (slot[0, cols == 1] == deg - 1).all() and (slot[0, cols == 2] == 0).all()
            assert (out[0, cols < 2] == 5).all() and (out[0, cols == 2] == 2).all()
            assert {0, 1, 2} <= set(cols.tolist())
    assert R.hub_graph(254).arg_bytes == 1 and R.hub_graph(255).arg_bytes == 4


# ---------------------------------------------------------------- the inputs discriminate
def _rows_edited(indptr, indices, edit, *more):
    """CSR whose row v is edit(v, row v), the same edit applied to every per-edge array of `more`."""
    parts = [[edit(v, a[indptr[v]:indptr[v + 1]]) for v in range(indptr.size - 1)] for a in (indices,) + more]
    ptr = np.concatenate([[0], np.cumsum([p.size for p in parts[0]])]).astype(indptr.dtype)
    return (ptr,) + tuple(np.concatenate(p) if p else a[:0] for p, a in zip(parts, (indices,) + more))


def _drop_last_of_8k_plus_1(v, row):
    return row[:-1] if row.size % 8 == 1 else row


def _clamped_tail_read_as_valid(v, row):
    """A chunk of 8 whose positions past the row's end are clamped to its last edge, with no valid(j)."""
    return row if row.size % 8 == 0 else np.concatenate([row, np.repeat(row[-1:], 8 - row.size % 8)])


def _self_first(v, row):
    return np.concatenate([np.asarray([v], dtype=row.dtype), row])


def _max_with_last_maximum(g, x):
    """The tie rule `<=`: the last maximum wins."""
    win = np.full((g.n, x.shape[1]), -1, dtype=np.int64)
    for v in range(g.n):
        u = g.indices[g.indptr[v]:g.indptr[v + 1]]
        if u.size:
            win[v] = u[u.size - 1 - np.argmax(x[u][::-1], axis=0)]
    return win


WRONG_CASES = [(w, name, t) for w in (1, 4, 17, 64, 256, 516) for name in ("u8", "i32") for t in (False, True)]
_noticed = {}


def _notices(width, name, transpose):
    """variant -> whether it differs from the true reference on the inputs of one case of the every-width GPU test."""
    key = (width, name, transpose)
    if key in _noticed:
        return _noticed[key]
    c = R.width_inputs(width, name, transpose)
    g, ints, gauss, gout = c["g"], c["integers"], c["gaussian"], c["gout"]
    csrs = {"in": (g.indptr, g.indices), "out": (g.t_indptr, g.t_indices)}
    out = {"tie <=": not np.array_equal(_max_with_last_maximum(g, ints), R.max_ref(g, ints)[1])}
    # the last edge of a row of degree 8k + 1 dropped
    ptr, idx = _rows_edited(*csrs["in"], _drop_last_of_8k_plus_1)
    short = SimpleNamespace(n=g.n, indptr=ptr, indices=idx)
    out["dropped edge, max"] = not R.same_bits(R.max_ref(short, gauss)[0], R.max_ref(g, gauss)[0])
    for which, (ip, ix) in csrs.items():
        ptr, idx = _rows_edited(ip, ix, _drop_last_of_8k_plus_1)
        out["dropped edge, sum " + which] = not R.same_bits(R.sum_ref(ptr, idx, gauss), R.sum_ref(ip, ix, gauss))
        out["8k+1 rows " + which] = bool((np.diff(ip) % 8 == 1).any())
        # a clamped, out-of-row edge read as valid: the last edge counts again
        ptr, idx = _rows_edited(ip, ix, _clamped_tail_read_as_valid)
        out["clamped edge, sum " + which] = all(not R.same_bits(R.sum_ref(ptr, idx, x), R.sum_ref(ip, ix, x)) for x in (ints, gauss))
    # ... which the maximum is blind to (the repeated value is never strictly greater) and K2 is not
    ptr, idx = _rows_edited(*csrs["in"], _clamped_tail_read_as_valid)
    padded = SimpleNamespace(n=g.n, indptr=ptr, indices=idx)
    assert all(np.array_equal(a, b) for a, b in zip(R.max_ref(padded, ints), R.max_ref(g, ints)))
    tp, ti, ts = _rows_edited(*csrs["out"], _clamped_tail_read_as_valid, g.t_slot)
    padded = SimpleNamespace(n=g.n, t_indptr=tp, t_indices=ti, t_slot=ts)
    slots = R.max_ref(g, gauss, slots=True)[1]
    out["clamped edge, max bwd"] = not R.same_bits(R.max_bwd_ref(padded, gout, slots), R.max_bwd_ref(g, gout, slots))
    # the self term before the neighbours instead of after them
    ip, ix = csrs["in"]
    ptr, idx = _rows_edited(ip, ix, _self_first)
    out["self first"] = all(not R.same_bits(R.sum_ref(ptr, idx, gauss, div_in=div), R.sum_ref(ip, ix, gauss, div_in=div, add_self=True))
                            for div in (None, c["divisors"]["random"]))
    # the sum divided once instead of each term by its own div_in
    out["divided once"] = all(not R.same_bits(R.sum_ref(ip, ix, gauss) / div[:, None], R.sum_ref(ip, ix, gauss, div_in=div))
                              for div in c["divisors"].values())
    _noticed[key] = out
    return out


@pytest.mark.parametrize("width,name,transpose", WRONG_CASES)
def test_inputs_notice_a_wrong_kernel(width, name, transpose):
    """Each deliberately wrong variant differs from the true reference on the inputs the GPU test uses: in every case
    where the inputs make it differ by construction (a dropped edge needs a row of degree 8k + 1 to drop it from)."""
    got = _notices(width, name, transpose)
    for variant in ("tie <=", "clamped edge, sum in", "clamped edge, sum out", "self first", "divided once"):
        assert got[variant], variant
    for which in ("in", "out"):
        assert got["dropped edge, sum " + which] == got["8k+1 rows " + which], which
    assert got["8k+1 rows out" if transpose else "8k+1 rows in"] or R.geometry(1, width, 0)[1] == 64


def test_variants_that_need_a_winner_in_the_right_place_are_noticed_in_every_lane_class():
    """A dropped last edge changes a maximum, and a repeated last edge a routed gradient, only where that edge wins: not in
    every case, but at wave-per-row widths and at shared-wave widths alike (the clamped read exists only at the latter)."""
    for wide in (False, True):
        cases = [c for c in WRONG_CASES if (R.geometry(1, c[0], 0)[1] == 64) == wide]
        assert sum(_notices(*c)["dropped edge, max"] for c in cases) >= 1
        assert sum(_notices(*c)["8k+1 rows in"] for c in cases) >= 1
        if not wide:
            assert sum(_notices(*c)["clamped edge, max bwd"] for c in cases) >= 1


def test_inputs_notice_a_wrong_winner_width_and_a_lost_zero_sign():
    # the uint8 sentinel's neighbour applied to an int32 record: slot 254 of the 255-edge row read as "no winner"
    for f in R.HUB_WIDTHS:
        g, x = R.hub_graph(255), R.hub_features(255, f)
        slot = R.max_ref(g, x, slots=True)[1]
        wrong = np.where(slot == 254, -1, slot)
        assert not np.array_equal(wrong, slot)
        gout = R.gaussian(g.n, f, 9)
        assert not R.same_bits(R.max_bwd_ref(g, gout, wrong), R.max_bwd_ref(g, gout, slot))
        # 0xFF itself is a real slot of the 256-edge row
        g, x = R.hub_graph(256), R.hub_features(256, f)
        assert (R.max_ref(g, x, slots=True)[1][0] == 255).any()
    # -0.0 written as +0.0
    g = R.ladder(R.VALUE_ROWS, "u8", seed=3)
    for f in R.VALUE_WIDTHS:
        out = R.max_ref(g, R.signed_zeros(g, f, 5)[0])[0]
        assert not R.same_bits(out + np.float32(0), out) and np.array_equal(out + np.float32(0), out)
