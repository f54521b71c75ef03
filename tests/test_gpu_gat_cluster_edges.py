"""The clustered GAT kernels (csrc/gts_gat_cluster.hip) on schedules made by hand (tests/cluster_ref.py: pack), injected into
Graph._sched: chosen degree pairs in one wave slot, clusters of one row and of an odd number of rows, rows without out-edges
in the source pass, 1 / 3 / 4 heads, 1 / 3 / 8 / 9 clusters, both dealing modes.  Bar: the plain kernels' bits (csrc/gts_gat.hip,
held to fp64 by tests/test_gpu_gat_edges.py), through ops._gat_fwd / ops._gat_bwd as tests/test_gpu_gat_cluster.py compares
them on graph families.  One parametrised test per pass."""
import numpy as np
import pytest
import torch

from gts import _lib, ops, schedule
from tests import cluster_ref as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAT_DEALING = _lib.const("GTS_OPT_GAT_CLUSTER_DEALING")
ENTRY = {"gat_in": "gts_gat_fwd_cluster_f32", "gat_edge_in": "gts_gat_bwd_edge_cluster_f32", "gat_out": "gts_gat_bwd_src_cluster_f32"}


@pytest.fixture(scope="module", autouse=True)
def _lib_and_rules(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    old = schedule.MIN_ROWS_GAT, schedule.MAX_DEGREE_GAT, schedule.WORTHWHILE
    schedule.MIN_ROWS_GAT, schedule.MAX_DEGREE_GAT, schedule.WORTHWHILE = 0, 10 ** 9, 10.0
    yield hip_lib
    schedule.MIN_ROWS_GAT, schedule.MAX_DEGREE_GAT, schedule.WORTHWHILE = old


def _plain(fn):
    old = schedule.ENABLED_GAT
    schedule.ENABLED_GAT = False
    try:
        return fn()
    finally:
        schedule.ENABLED_GAT = old


def _cases(kind):
    cases = [C.gat_pair_case(kind)] + [C.gat_count_case(kind, k) for k in (1, 3, 8, 9)]
    for c in cases:
        slots = [p for cl in C.wave_slots(c["sched"]) for p in cl]
        assert not c["sched"].tagged and c["sched"].limits == C.GAT_LIMITS[kind]
        if "pairs" in c:
            assert slots[:len(c["pairs"])] == c["pairs"] and len(c["pairs"]) == 64
            assert 1 in C.rows_of(c["sched"]) and 3 in C.rows_of(c["sched"])
        c["g"]._sched[kind] = c["sched"]              # shared by every view of the graph
    assert [c["sched"].n_clusters for c in cases[1:]] == [1, 3, 8, 9]
    return cases


def _inputs(g, heads, seed):
    gen = torch.Generator().manual_seed(seed)
    ft = torch.randn(g.n, heads, 256, generator=gen)
    el, er = torch.randn(g.n, heads, generator=gen) * 2, torch.randn(g.n, heads, generator=gen) * 2
    gout = torch.randn(g.n, heads, 256, generator=gen)
    al, ar = torch.randn(heads, 256, generator=gen), torch.randn(heads, 256, generator=gen)
    bias = torch.randn(heads * 256, generator=gen)
    return [t.to(DEV) for t in (ft, el, er, gout, al, ar, bias)]


def _run(kind, heads, dealing, check):
    """`check(case, graph on the device, inputs)` on every case of `kind` under one dealing mode, the clustered entry point of
    the pass counted: it ran once per clustered call."""
    lib = _lib.load()
    real = getattr(lib, ENTRY[kind])
    ran = []
    assert lib.gts_get_option(GAT_DEALING) == 0
    try:
        assert lib.gts_set_option(GAT_DEALING, dealing) == 0
        setattr(lib, ENTRY[kind], lambda *a: (ran.append(1), real(*a))[1])
        for c in _cases(kind):
            before = len(ran)
            gd = c["g"].to(DEV)
            assert gd.cluster_schedule(kind) is c["sched"]
            check(c, gd, _inputs(c["g"], heads, c["g"].n))
            assert len(ran) > before, "the clustered kernel did not run"
    finally:
        setattr(lib, ENTRY[kind], real)
        lib.gts_set_option(GAT_DEALING, 0)


@pytest.mark.parametrize("dealing", [0, 1])
@pytest.mark.parametrize("heads", [1, 3, 4])
def test_forward_on_hand_made_partitions_equals_the_plain_kernel(heads, dealing):
    """In-degree pairs from {1, 7, 8, 9, 16, 17, 63, 64} in one wave slot; with and without bias + ELU."""
    def check(c, gd, inputs):
        ft, el, er, _, _, _, bias = inputs
        assert c["g"].max_in_degree == 64 or "pairs" not in c
        for b, act in ((bias, 1), (None, 0)):
            out, attn = ops._gat_fwd(gd, ft, el, er, 0.2, bias=b, activation=act)
            out_p, attn_p = _plain(lambda: ops._gat_fwd(gd, ft, el, er, 0.2, bias=b, activation=act))
            assert torch.equal(attn, attn_p) and torch.equal(out, out_p) and not torch.isnan(out).any()
    _run("gat_in", heads, dealing, check)


def _check_bwd(c, gd, inputs):
    ft, el, er, gout, al, ar, _ = inputs
    _, attn = _plain(lambda: ops._gat_fwd(gd, ft, el, er, 0.2))
    for vecs in ((al, ar), (None, None)):
        got = ops._gat_bwd(gd, ft, el, er, attn, gout, 0.2, *vecs)
        want = _plain(lambda: ops._gat_bwd(gd, ft, el, er, attn, gout, 0.2, *vecs))
        for a, w, what in zip(got, want, ("gft", "gel", "ger")):
            assert torch.equal(a, w) and not torch.isnan(a).any(), what


@pytest.mark.parametrize("dealing", [0, 1])
@pytest.mark.parametrize("heads", [1, 3, 4])
def test_source_pass_on_hand_made_partitions_equals_the_plain_kernel(heads, dealing):
    """Out-degree pairs from {1, 7, 8, 9, 16, 17, 63, 64} in one wave slot, rows without out-edges beside rows with some."""
    def check(c, gd, inputs):
        if "pairs" in c:
            deg = np.diff(c["g"].t_indptr)
            assert deg.max() == 64 and (deg == 0).sum() == 4
        _check_bwd(c, gd, inputs)
    _run("gat_out", heads, dealing, check)


@pytest.mark.parametrize("dealing", [0, 1])
@pytest.mark.parametrize("heads", [1, 3, 4])
def test_edge_pass_on_hand_made_partitions_equals_the_plain_kernel(heads, dealing):
    """In-degree pairs from 1 .. 8 in one wave slot: rows of one 8-edge chunk, which the clustered edge pass takes."""
    def check(c, gd, inputs):
        assert c["g"].max_in_degree <= 8 and (c["g"].max_in_degree == 8 or "pairs" not in c)
        _check_bwd(c, gd, inputs)
    _run("gat_edge_in", heads, dealing, check)
