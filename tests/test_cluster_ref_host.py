"""The hand-made cluster schedules of tests/cluster_ref.py, proven on the CPU before tests/test_gpu_cluster_edges.py sends
them to the clustered K1 / K2 kernels (csrc/gts_spmm_cluster.hip, which stores to out + row * 256 unguarded): the packer
writes byte for byte what the greedy builder writes for the builder's own partitions, every case is an exact cover within
its limits with every id in range, every case contains the wave slots, chunk counts, record sizes, neighbour counts and
cluster counts it claims, the kernels' walk restated over the records equals the per-row references of tests/spmm_ref.py
bit for bit, and every deliberately wrong walk changes a bit of the case that targets it."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import gts
from gts import schedule, synth
from tests import cluster_ref as C
from tests import spmm_ref as R
from tests.helpers import random_coo
from tests.test_cluster_schedule import _check_cover


@pytest.fixture(scope="module", autouse=True)
def lib(hip_lib):
    return hip_lib


# ---------------------------------------------------------------- the packer writes what the builder writes
def _build(g, which, lim):
    ip, ix, tp, tx = (g.indptr, g.indices, g.t_indptr, g.t_indices) if which == "in" else \
        (g.t_indptr, g.t_indices, g.indptr, g.indices)
    return schedule.ClusterSchedule.build(ip, ix, tp, tx, g.t_slot if which == "out" else None, lim)


def _same_as_builder(g, which, lim):
    s = _build(g, which, lim)
    if s is None:
        return False
    groups, orders = C.partition_of(s)
    mine = C.pack(g, which, groups, lim, srcs=orders)
    assert mine.loc_words == s.loc_words and mine.tagged == s.tagged and mine.limits == s.limits
    assert (mine.n_rows, mine.n_edges, mine.staged_rows) == (s.n_rows, s.n_edges, s.staged_rows)
    assert mine.rec.shape == s.rec.shape and mine.rec.tobytes() == s.rec.tobytes()
    return True


@pytest.mark.parametrize("which", ["in", "out"])
def test_packer_equals_builder_on_the_lattice_and_the_geometric_graph_with_holes(which):
    assert _same_as_builder(synth.lattice_graph((9, 8, 7)), which, C.DEFAULT_LIMITS[which])
    base = synth.geometric_graph(n=1500, k=8, seed=3, self_loops=True)
    keep = base.dst % 97 != 5
    holes = gts.Graph(base.src[keep], base.dst[keep], base.n)
    assert holes.min_in_degree == 0
    assert _same_as_builder(holes, which, C.DEFAULT_LIMITS[which])
    assert _same_as_builder(holes, which, (16, 40, 128))


@settings(max_examples=40, deadline=None)
@given(n=st.integers(1, 120), e=st.integers(0, 500), seed=st.integers(0, 10 ** 6),
       rows=st.integers(1, 20), srcs=st.integers(30, 60))
def test_packer_equals_builder_on_any_graph_at_any_limits(n, e, seed, rows, srcs):
    src, dst = random_coo(n, e, seed)
    g = gts.Graph(src, dst, n)
    for which in ("in", "out"):
        if not _same_as_builder(g, which, (rows, srcs, 400)):
            deg = np.diff(C.csr(g, which)[0])
            assert deg.max() > srcs or (which == "out" and g.t_slot.max() > 255)


def test_first_use_order_is_the_default_and_any_order_decodes_to_the_same_rows():
    g = synth.lattice_graph((5, 6, 7))
    groups = C.greedy_groups(g, "out", (32, 60, 512))
    a = C.pack(g, "out", groups, (32, 60, 512))
    _check_cover(g, "out", a)
    orders = [list(reversed(o)) for o in C.partition_of(a)[1]]
    b = C.pack(g, "out", groups, (32, 60, 512), srcs=orders)
    _check_cover(g, "out", b)
    assert a.rec.tobytes() != b.rec.tobytes()
    for (_, sa, _), rows in zip(a.decode(), groups):      # first use over the rows ascending
        seen = []
        for v in rows:
            seen += [u for u in g.t_indices[g.t_indptr[v]:g.t_indptr[v + 1]].tolist() if u not in seen]
        assert sa.tolist() == seen


def test_packer_refuses_what_a_kernel_must_never_see():
    g = synth.lattice_graph((4, 4, 4))
    lim = (32, 60, 512)
    groups = C.greedy_groups(g, "in", lim)
    C.pack(g, "in", groups, lim)
    with pytest.raises(ValueError):
        C.pack(g, "in", groups[:-1], lim)                              # a row in no cluster
    with pytest.raises(ValueError):
        C.pack(g, "in", groups + [groups[0]], lim)                     # a row in two
    with pytest.raises(ValueError):
        C.pack(g, "in", groups[:-1] + [groups[-1] + [g.n]], lim)       # a row id past the graph
    with pytest.raises(ValueError):
        C.pack(g, "in", groups[:-1] + [groups[-1] + [-1]], lim)
    with pytest.raises(ValueError):
        C.pack(g, "in", [list(range(g.n))], lim)                       # more rows than the limit
    with pytest.raises(ValueError):
        C.pack(g, "in", [list(range(g.n))], (g.n, 8, 65535))           # more neighbours than the limit
    with pytest.raises(ValueError):
        C.pack(g, "in", [[v] for v in range(g.n)], (1, 3, 512))        # rows of up to 6 distinct neighbours
    with pytest.raises(ValueError):
        C.pack(g, "in", groups, (32, 60, 16))                          # padded edges
    with pytest.raises(ValueError):
        C.pack(g, "in", groups, (32, 300, 512))                        # byte-indexed neighbours
    # a tag that does not fit a byte: one destination with 300 in-edges
    n = 301
    hub = gts.Graph(np.arange(1, n), np.zeros(n - 1, dtype=np.int64), n)
    assert hub.t_slot.max() == 299
    with pytest.raises(ValueError):
        C.pack(hub, "out", [[v] for v in range(n)], (1, 4, 8))
    # records above 512 words
    with pytest.raises(ValueError, match="words"):
        C.make_case("in", [[64] * 32], (32, 256, 2048), 0)


# ---------------------------------------------------------------- the cases
_cases = {}


largest_max_srcs = C.largest_max_srcs


def cases(lib):
    """name -> case: every hand-made schedule the GPU test launches (the dealing cases of thousands of one-row clusters are
    made the same way, by count_case, and checked by the GPU test's own asserts on the counts)."""
    if _cases:
        return _cases
    for which in ("in", "out"):
        _cases[f"pairs-{which}"] = C.pair_case(which)
        top = largest_max_srcs(lib, which)
        for s in (C.DEFAULT_LIMITS[which][1], top, top + 1):
            _cases[f"long-{which}-{s}"] = C.long_case(which, s)
        _cases[f"long-{which}-64-one-piece"] = C.long_case(which, 64, max_edges=256, max_rows=8)
        for words in ((252, 256, 260, 512) if which == "in" else (248, 256, 264, 512)):
            _cases[f"records-{which}-{words}"] = C.record_case(which, words)
        for count in (1, 2, 3, 4, 5, 7, 8, 9):
            _cases[f"count-{which}-{count}"] = C.count_case(which, count)
        _cases[f"one-row-{which}-300"] = C.count_case(which, 300, rows_per_cluster=1)
    return _cases


def test_largest_neighbour_limit_is_about_what_the_launch_arithmetic_says(lib):
    k1, k2 = largest_max_srcs(lib, "in"), largest_max_srcs(lib, "out")
    assert 140 <= k1 <= 160 and 110 <= k2 <= 130 and k1 % 2 == 0


def test_every_case_is_an_exact_cover_with_every_id_in_range(lib):
    for name, c in cases(lib).items():
        g, s = c["g"], c["sched"]
        _check_cover(g, c["which"], s)
        lay = s.layout
        assert lay.words <= 512 and s.rec.shape == (len(c["clusters"]), lay.words), name
        ids = s.rec[:, lay.rows:lay.eoff]
        assert ids.min() >= 0 and ids.max() < g.n, name
        assert C.rows_of(s) == [len(d) for d in c["clusters"]], name
        assert [d for slots in C.wave_slots(s) for p in slots for d in p if d is not None] == [d for k in c["clusters"] for d in k]
        assert g.arg_bytes == 1, name
        # ... and so is the schedule of the other CSR, which the GPU test packs greedily at the default limits
        other = "out" if c["which"] == "in" else "in"
        _check_cover(g, other, C.other_schedule(g, other))


def test_pair_cases_hold_every_ordered_pair_every_cluster_size_and_the_zero_row_past_the_section(lib):
    for which in ("in", "out"):
        c = cases(lib)[f"pairs-{which}"]
        s = c["sched"]
        slots = [p for cl in C.wave_slots(s) for p in cl]
        want = [(a, b) for a in C.PAIR_DEGREES for b in C.PAIR_DEGREES]
        assert len(want) == 225 and slots[:225] == want == c["pairs"]
        assert (8, 8) in slots and (9, 9) in slots and (8, 9) in slots and (9, 8) in slots
        sizes = C.rows_of(s)
        assert sizes[38:44] == [1, 1, 2, 3, 31, 32] == c["sizes"] and sizes[:38] == [12] * 37 + [6]
        odd = [cl[-1] for cl in C.wave_slots(s) if cl[-1][1] is None]
        assert odd == [(0, None), (7, None), (7, None), (7, None)]               # an odd last row: clusters of 1, 1, 3 and 31 rows
        assert C.n_srcs_of(s)[38] == 0 and min(C.n_srcs_of(s)[:38] + C.n_srcs_of(s)[39:]) > 0      # one cluster stages nothing
        # the fullest cluster: 400 padded edges = 100 loc words exactly, last row without an edge and first chunk 50 = one past
        at, edges = c["full"]
        lay = s.layout
        assert C.padded_edges_of(s)[at] == edges == 400 == max(C.padded_edges_of(s)) and s.loc_words == 100
        info = s.rec[at, lay.eoff:lay.eoff + sizes[at]].view(np.uint32)
        assert int(info[-1] >> 16) == 0 and int(info[-1] & 0xFFFF) == 8 * s.loc_words // 8 // 2 == 50
        assert C.wave_slots(s)[at][-1] == (16, 0)
        # chunk counts: rows of 1, 2, 3 and 4 chunks, every count 1 .. 8 in a last chunk
        degs = [d for cl in c["clusters"] for d in cl]
        assert {(d + 7) // 8 for d in degs} == {0, 1, 2, 3, 4} and {d % 8 for d in degs} == set(range(8))
        assert s.limits == C.DEFAULT_LIMITS[which] and max(C.n_srcs_of(s)) <= 40


def test_long_cases_hold_the_full_list_the_neighbour_counts_and_the_full_edge_section(lib):
    for which in ("in", "out"):
        top = largest_max_srcs(lib, which)
        for name, limit, rows, edges in [(f"long-{which}-{s}", s, 32, 512) for s in (C.DEFAULT_LIMITS[which][1], top, top + 1)] + \
                                        [(f"long-{which}-64-one-piece", 64, 8, 256)]:
            c = cases(lib)[name]
            s = c["sched"]
            assert s.limits == (rows, limit, edges)
            counts = C.n_srcs_of(s)
            odd = limit if limit % 2 else limit - 1
            assert counts[0] == limit and C.wave_slots(s)[0] == [(limit, None)]
            assert counts[1:8] == [1, 2, 3, 7, 8, 9, odd] == c["n_srcs"][1:]
            at, full = c["full"]
            assert C.padded_edges_of(s)[at] == full == edges and C.rows_of(s)[at] == rows and s.loc_words == edges // 4
            ip, ix, _ = C.csr(c["g"], which)
            for v in c["hubs"]:
                u = ix[ip[v]:ip[v + 1]]
                assert np.unique(u).size == u.size
        one = cases(lib)[f"long-{which}-64-one-piece"]["sched"]
        assert one.layout.words <= 256 and cases(lib)[f"long-{which}-{top}"]["sched"].layout.words > 256


def test_record_cases_have_exactly_the_words_they_name(lib):
    for which, sizes in (("in", (252, 256, 260, 512)), ("out", (248, 256, 264, 512))):
        for words in sizes:
            c = cases(lib)[f"records-{which}-{words}"]
            s = c["sched"]
            assert s.layout.words == words == c["words"] and s.tagged == (which == "out")
            assert (words + 255) // 256 == (1 if words <= 256 else 2)
            assert max(C.padded_edges_of(s)) == 4 * s.loc_words == C.padded_edges_of(s)[1]
            wide = s.with_loc_words(s.loc_words + 8)
            _check_cover(c["g"], which, wide)
    # no limits give a record of 255 or 257 words: every section is padded to 4 words
    for r in range(1, 40):
        for e in range(0, 64, 4):
            assert schedule._Layout(r, 76, e, False).words % 4 == 0 and schedule._Layout(r, 60, e, True).words % 4 == 0


def test_count_cases_have_the_cluster_counts_they_name(lib):
    for which in ("in", "out"):
        for count in (1, 2, 3, 4, 5, 7, 8, 9):
            s = cases(lib)[f"count-{which}-{count}"]["sched"]
            assert s.n_clusters == count and C.rows_of(s) == [3] * count
        s = cases(lib)[f"one-row-{which}-300"]["sched"]
        assert s.n_clusters == 300 == s.n_rows and C.rows_of(s) == [1] * 300


def test_gat_cases_are_untagged_exact_covers_with_their_pairs_in_one_wave_slot():
    """The schedules tests/test_gpu_gat_cluster_edges.py injects: at the limits of gts/schedule.py, every id in range."""
    for kind, lim in C.GAT_LIMITS.items():
        assert schedule.limits(kind) == lim
        which = "out" if kind == "gat_out" else "in"
        for c in [C.gat_pair_case(kind)] + [C.gat_count_case(kind, k) for k in (1, 3, 8, 9)]:
            g, s = c["g"], c["sched"]
            assert not s.tagged and s.limits == lim and s.loc_words >= 2 and s.layout.words <= 512
            ip, ix, _ = C.csr(g, which)
            seen = np.zeros(g.n, dtype=np.int64)
            for rows, srcs, per_row in s.decode():
                assert len(rows) <= lim[0] and len(srcs) <= lim[1] and len(set(srcs.tolist())) == len(srcs)
                assert sum((len(nb) + 7) // 8 * 8 for _, nb, _ in per_row) <= lim[2]
                for r, nb, _ in per_row:
                    seen[r] += 1
                    assert nb == ix[ip[r]:ip[r + 1]].tolist()
            assert (seen == 1).all()
            ids = s.rec[:, s.layout.rows:s.layout.eoff]
            assert ids.min() >= 0 and ids.max() < g.n and g.max_in_degree <= 64
        c = C.gat_pair_case(kind)
        degs = C.GAT_EDGE_DEGREES if kind == "gat_edge_in" else C.GAT_DEGREES
        slots = [p for cl in C.wave_slots(c["sched"]) for p in cl]
        assert slots[:64] == [(a, b) for a in degs for b in degs] == c["pairs"]
        assert {1, 3} <= set(C.rows_of(c["sched"]))
        if kind == "gat_edge_in":
            assert c["g"].max_in_degree == 8
        if kind == "gat_out":
            assert (np.diff(c["g"].t_indptr) == 0).sum() == 4 and (5, 0) not in slots and (0, 7) in slots and (0, None) in slots


# ---------------------------------------------------------------- the walk over the records equals the references
def _inputs(g, seed):
    return R.integers(g.n, C.F, seed), R.gaussian(g.n, C.F, seed + 1), R.gaussian(g.n, C.F, seed + 2)


def _same_u8(a, b):
    return np.array_equal(np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8))


EMULATED = ["pairs-in", "pairs-out", "records-in-260", "records-out-264", "records-in-512", "records-out-512", "count-in-3",
            "count-out-9", "long-in-64-one-piece", "long-out-64-one-piece"]


@pytest.mark.parametrize("name", EMULATED)
def test_the_restated_walk_equals_the_per_row_references_bit_for_bit(lib, name):
    c = cases(lib)[name]
    g, which = c["g"], c["which"]
    s_in = c["sched"] if which == "in" else C.other_schedule(g, "in")
    s_out = c["sched"] if which == "out" else C.other_schedule(g, "out")
    ints, gauss, gout = _inputs(g, 7)
    for x in (ints, gauss):
        for relu in (False, True):
            want, _, slot = R.max_ref_full(g, x, relu)
            out, arg = C.emulate_k1(s_in, x, relu)
            assert R.same_bits(out, want) and _same_u8(arg, C.winner_bytes(slot)), (name, relu)
            gx = C.emulate_k2(s_out, gout, arg)
            assert R.same_bits(gx, R.max_bwd_ref(g, gout, slot)), (name, relu)


def test_value_classes_are_where_the_builders_say_on_the_pair_case(lib):
    g = cases(lib)["pairs-in"]["g"]
    x, rows = C.nonfinite_in(g, 6)
    out, _, slot = R.max_ref_full(g, x)
    _, _, slot_relu = R.max_ref_full(g, x, True)
    assert not np.isnan(out).any() and not np.isinf(out).any()
    for k in ("nan_only", "pos_inf", "neg_inf_all"):
        assert (out[rows[k]].view(np.int32) == 0).all() and (slot[rows[k]] == -1).all(), k
    assert (slot[rows["nan_among"]] != 1).all() and (slot[rows["nan_among"]] >= 0).all()
    top = int(np.diff(g.indptr).max())
    assert top == 25 and (slot[rows["last_slot"]] == top - 1).all() and (slot_relu[rows["last_slot"]] == top - 1).all()
    bits = out.view(np.int32)
    assert (out[rows["neg_denormal"]] == np.float32(-1e-40)).all() and np.float32(-1e-40) < 0
    assert (bits[rows["pos_zero"]] == 0).all() and (bits[rows["neg_zero"]] == np.int32(-2 ** 31)).all()
    for k in ("neg_denormal", "pos_zero", "neg_zero"):
        assert (slot[rows[k]] == 1).all() and (slot_relu[rows[k]] == -1).all(), k
    got, arg = C.emulate_k1(cases(lib)["pairs-in"]["sched"], x)
    assert R.same_bits(got, out) and _same_u8(arg, C.winner_bytes(slot))
    z, zrows = R.signed_zeros(g, C.F, 5)
    out = R.max_ref_full(g, z)[0].view(np.int32)
    assert (out[zrows["neg"]] == np.int32(-2 ** 31)).all() and (out[zrows["pos_then_neg"]] == 0).all()


def test_hub_columns_put_the_winner_in_the_first_and_in_the_last_slot_of_the_longest_rows(lib):
    for which in ("in", "out"):
        c = cases(lib)[f"long-{which}-{C.DEFAULT_LIMITS[which][1]}"]
        g = c["g"]
        if which == "out":
            continue                      # the hubs of an out-case are sources: their columns are K2's tags, not K1's slots
        x = C.hub_columns(R.integers(g.n, C.F, 3), g, "in", c["hubs"][:1])
        slot = R.max_ref_full(g, x)[2]
        cols = np.arange(C.F) % 3
        deg = c["n_srcs"][0]
        assert (slot[0, cols == 0] == 0).all() and (slot[0, cols == 1] == deg - 1).all() and (slot[0, cols == 2] == 0).all()
        assert (deg - 1) % 8 == 3 and deg == 76                                   # the last chunk holds four edges


# ---------------------------------------------------------------- every wrong walk changes a bit of its case
def test_a_wrong_walk_changes_a_bit_of_the_case_that_targets_it(lib):
    pin, pout = cases(lib)["pairs-in"], cases(lib)["pairs-out"]
    ints, gauss, gout = _inputs(pin["g"], 7)
    right = C.emulate_k1(pin["sched"], gauss)
    wrong = C.emulate_k1(pin["sched"], gauss, unmasked=True)
    assert not R.same_bits(right[0], wrong[0]), "K1: a shorter row that is not masked"
    right = C.emulate_k1(pin["sched"], ints)
    wrong = C.emulate_k1(pin["sched"], ints, tie_last=True)
    assert R.same_bits(right[0], wrong[0]) and not _same_u8(right[1], wrong[1]), "K1: '<=' moves winners, not values"

    g = pout["g"]
    ints, gauss, gout = _inputs(g, 7)
    arg = C.winner_bytes(R.max_ref_full(g, ints)[2])
    right = C.emulate_k2(pout["sched"], gout, arg)
    assert not R.same_bits(right, C.emulate_k2(pout["sched"], gout, arg, unmasked=True)), "K2: pads that count"
    fast = C.emulate_k2(pout["sched"], gout, arg, fast_unequal=True)
    assert not R.same_bits(right, fast), "K2: the fast path for unequal degrees"
    # ... and exactly in slots of unequal degrees of at most 8
    deg = np.diff(g.t_indptr)
    mate = np.concatenate([[k[j ^ 1] if (j ^ 1) < len(k) else 0 for j in range(len(k))] for k in pout["clusters"]])
    changed = np.flatnonzero((right.view(np.int32) != fast.view(np.int32)).any(axis=1))
    assert changed.size and (deg[changed] < mate[changed]).all() and (mate[changed] <= 8).all()

    for name in ("records-in-260", "records-in-512"):
        c = cases(lib)[name]
        x = _inputs(c["g"], 7)[1]
        assert not R.same_bits(C.emulate_k1(c["sched"], x)[0], C.emulate_k1(c["sched"], x, zero_second_piece=True)[0]), name
    for name in ("records-out-264", "records-out-512"):
        c = cases(lib)[name]
        ints, _, gout = _inputs(c["g"], 7)
        arg = C.winner_bytes(R.max_ref_full(c["g"], ints)[2])
        assert not R.same_bits(C.emulate_k2(c["sched"], gout, arg), C.emulate_k2(c["sched"], gout, arg, zero_second_piece=True)), name
    # one piece holds the whole record of 256 words: nothing to lose
    c = cases(lib)["records-in-256"]
    x = _inputs(c["g"], 7)[1]
    assert R.same_bits(C.emulate_k1(c["sched"], x)[0], C.emulate_k1(c["sched"], x, zero_second_piece=True)[0])
