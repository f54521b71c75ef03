"""The GATConv attention kernels (csrc/gts_gat.hip: fused edge softmax + aggregation, backward edge pass, backward source
pass) against the float64 reference of tests/gat_ref.py under its derived bounds, on a real MI355X, at the degree, geometry
and score edges where they can go wrong: in- and out-degrees on both sides of every chunk remainder and of the 64-edge
wave-per-row paths (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200), every (VEC, LPR) geometry, scores whose
weights underflow to zero, scores with pre == 0 and ties of the row maximum.  No element is left out of a comparison.
Then the clustered kernels (csrc/gts_gat_cluster.hip) under the same scores: bit-equal to the plain kernels wherever the
schedule builder takes the graph.  The bounds and their constants are validated on the CPU in tests/test_gat_ref_host.py."""
import numpy as np
import pytest
import torch

import gts
from gts import _lib, ops, schedule, synth
from gts.ops import current_stream, ptr
from tests import gat_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPT_GAT_WALK = 14       # include/gts_hip.h: GTS_OPT_GAT_WALK


@pytest.fixture(scope="module", autouse=True)
def _plain_kernels_and_forced_rules(hip_lib):
    """The plain kernels for the whole module (the clustered tests switch the clustered ones on for their own calls), and
    the speed rules of the schedule out of the way, as in tests/test_gpu_gat_cluster.py."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    old = schedule.ENABLED_GAT, schedule.MIN_ROWS_GAT, schedule.MAX_DEGREE_GAT, schedule.WORTHWHILE
    schedule.ENABLED_GAT, schedule.MIN_ROWS_GAT, schedule.MAX_DEGREE_GAT, schedule.WORTHWHILE = False, 0, 10 ** 9, 10.0
    yield hip_lib
    schedule.ENABLED_GAT, schedule.MIN_ROWS_GAT, schedule.MAX_DEGREE_GAT, schedule.WORTHWHILE = old


def _clustered(fn):
    schedule.ENABLED_GAT = True
    try:
        return fn()
    finally:
        schedule.ENABLED_GAT = False


_device_graphs = {}


def _graph(rg):
    """The product graph of a reference graph, on the device: same in-CSR order."""
    g = _device_graphs.get(id(rg))
    if g is None:
        host = gts.Graph(rg.src, rg.dst, rg.n)
        assert np.array_equal(host.indices, rg.src) and np.array_equal(host.indptr, rg.indptr)
        g = _device_graphs[id(rg)] = (rg, host.to(DEV))
    return g[1]


def _dev(x, *names):
    return [x[k].to(DEV) for k in names]


def _hold(what, got, want, bound):
    """Prints the figure before it asserts: profiles/gat_edges/README.md records the worst of them per output and regime."""
    ratio = R.worst_ratio(got, want, bound)
    print(f"{what}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: worst error / bound = {ratio}"


def _run_and_hold(ref, slope):
    """Forward and both backwards of one reference case on the device, every output under its bound."""
    gd = _graph(ref["g"])
    ft, el, er, gout, al, ar = _dev(ref["x"], "ft", "el", "er", "gout", "attn_l", "attn_r")
    out, attn = ops._gat_fwd(gd, ft, el, er, slope)
    _hold("attn", attn, ref["fwd"]["a"], ref["fb"]["a"])
    _hold("out", out, ref["fwd"]["out"], ref["fb"]["out"])
    gft, gel, ger = ops._gat_bwd(gd, ft, el, er, attn, gout, slope)
    for what, got in (("gft", gft), ("gel", gel), ("ger", ger)):
        _hold(what, got, ref["bwd"][what], ref["bb"][what])
    gft_f, gel_f, ger_f = ops._gat_bwd(gd, ft, el, er, attn, gout, slope, al, ar)
    _hold("gft_folded", gft_f, ref["bwd"]["gft_folded"], ref["bb"]["gft_folded"])
    assert torch.equal(gel_f, gel) and torch.equal(ger_f, ger)
    return dict(out=out, attn=attn, gft=gft, gel=gel, ger=ger, gft_folded=gft_f)


# ---------------------------------------------------------------- plain kernels: degrees x geometry x regime
@pytest.mark.parametrize("kind,heads,dim,regime", R.cases())
def test_every_output_is_inside_its_fp64_bound(kind, heads, dim, regime):
    ref = R.reference_case(kind, heads, dim, regime)
    got = _run_and_hold(ref, 0.2)
    if regime == "underflow":       # the regime is what it says on the device too, and nothing in it is lost to a NaN
        assert float((got["attn"] == 0).float().mean()) > 0.30
    for t in got.values():
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("heads,dim", [(4, 256), (3, 64)])
@pytest.mark.parametrize("kind", ["in", "out"])
def test_slope_zero_blocks_every_edge_with_pre_not_above_zero(kind, heads, dim):
    """The bound of whatever flows through an edge with pre <= 0 is exactly 0 (tests/gat_ref.py): `>=` at pre == 0 fails."""
    ref = R.reference_case(kind, heads, dim, "integer", 0.0)
    assert float((ref["fwd"]["pre"] == 0).float().mean()) > 0.05
    _run_and_hold(ref, 0.0)
    g, x = ref["g"], ref["x"]
    gd = _graph(g)
    ft, gout = _dev(x, "ft", "gout")
    el, er = -x["el"].abs() - 1, -x["er"].abs()                                    # every pre < 0
    out, attn = ops._gat_fwd(gd, ft, el.to(DEV), er.to(DEV), 0.0)
    want = R.forward64(g, x["ft"], el, er, 0.0)
    _hold("attn", attn, want["a"], R.forward_bounds(g, want, x["ft"])["a"])
    gft, gel, ger = ops._gat_bwd(gd, ft, el.to(DEV), er.to(DEV), attn, gout, 0.0)
    assert bool((gel == 0).all()) and bool((ger == 0).all()) and bool(torch.isfinite(gft).all())


@pytest.mark.parametrize("heads,dim", [(4, 256), (3, 64)])
@pytest.mark.parametrize("kind", ["in", "out"])
def test_slope_one_is_the_reference_without_leaky(kind, heads, dim):
    _run_and_hold(R.reference_case(kind, heads, dim, "integer", 1.0, False), 1.0)


# ---------------------------------------------------------------- rows without edges
def _self_loops_elu(x):
    """elu(x) in the kernels' own arithmetic: a graph of self-loops only has weights of exactly 1.  Computed by the kernel
    under test, so it shows that a row without edges takes the same epilogue as any other row, not that the ELU is right:
    that rests on test_epilogue_combinations_are_inside_the_forward_bound and on the 4-ulp test of tests/test_gpu_kernels.py."""
    n, heads, dim = x.shape
    idx = np.arange(n)
    g = gts.Graph(idx, idx, n).to(DEV)
    zero = torch.zeros(n, heads, device=DEV)
    return ops._gat_fwd(g, x.contiguous(), zero, zero, 0.2, activation=1)[0]


@pytest.mark.parametrize("heads,dim", [(4, 256), (2, 65), (3, 64), (4, 3)])
def test_rows_without_in_edges(heads, dim):
    ref = R.reference_case("in", heads, dim, "unit")
    g, x = ref["g"], ref["x"]
    empty = torch.from_numpy(g.in_deg == 0).to(DEV)
    assert int(empty.sum()) == 14
    gd = _graph(g)
    ft, el, er, gout = _dev(x, "ft", "el", "er", "gout")
    gen = torch.Generator().manual_seed(dim)
    bias = torch.randn(heads * dim, generator=gen).to(DEV)
    res = torch.randn(g.n, heads * dim, generator=gen).to(DEV)
    out, attn = ops._gat_fwd(gd, ft, el, er, 0.2)
    assert bool((out[empty] == 0).all())
    pre = res.view(g.n, heads, dim) + bias.view(1, heads, dim)
    out_e, attn_e = ops._gat_fwd(gd, ft, el, er, 0.2, bias, res, 0)
    assert torch.equal(out_e[empty], pre[empty]) and torch.equal(attn_e, attn)
    out_a, _ = ops._gat_fwd(gd, ft, el, er, 0.2, bias, res, 1)
    assert torch.equal(out_a[empty], _self_loops_elu(pre[empty]))
    out_b, _ = ops._gat_fwd(gd, ft, el, er, 0.2, bias, None, 1)
    assert torch.equal(out_b[empty], _self_loops_elu(bias.view(1, heads, dim).expand(14, -1, -1)))
    gft, gel, ger = ops._gat_bwd(gd, ft, el, er, attn, gout, 0.2)
    assert bool((ger[empty] == 0).all())
    for t in (out, attn, out_e, out_a, out_b, gft, gel, ger):
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("heads,dim", [(4, 256), (2, 65), (3, 64), (4, 3)])
def test_rows_without_out_edges(heads, dim):
    ref = R.reference_case("out", heads, dim, "unit")
    g, x = ref["g"], ref["x"]
    empty = torch.from_numpy(g.out_deg == 0).to(DEV)
    assert int(empty.sum()) == 14
    gd = _graph(g)
    ft, el, er, gout, al, ar = _dev(x, "ft", "el", "er", "gout", "attn_l", "attn_r")
    _, attn = ops._gat_fwd(gd, ft, el, er, 0.2)
    gft, gel, ger = ops._gat_bwd(gd, ft, el, er, attn, gout, 0.2)
    assert bool((gel[empty] == 0).all()) and bool((gft[empty] == 0).all())
    gft_f, gel_f, ger_f = ops._gat_bwd(gd, ft, el, er, attn, gout, 0.2, al, ar)
    assert bool((gel_f[empty] == 0).all())
    assert torch.equal(gft_f[empty], ger_f[empty][:, :, None] * ar[None])           # the folded term alone, one rounding
    for t in (gft, gel, ger, gft_f):
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("kind", ["in", "out"])
def test_c_abi_writes_every_element(kind):
    """Through the C ABI with every output NaN beforehand: no NaN is left, attn and ge of every edge included."""
    heads, dim = 2, 65
    ref = R.reference_case(kind, heads, dim, "unit")
    g, x = ref["g"], ref["x"]
    gd = _graph(g)
    d = gd.dev()
    lib = _lib.load()
    ft, el, er, gout, al, ar = _dev(x, "ft", "el", "er", "gout", "attn_l", "attn_r")
    e = g.number_of_edges()

    def nan(*shape):
        return torch.full(shape, float("nan"), device=DEV)
    out, attn, ge, ger, gft, gel = nan(g.n, heads, dim), nan(e, heads), nan(e, heads), nan(g.n, heads), nan(g.n, heads, dim), nan(g.n, heads)
    _lib.check(lib.gts_gat_fwd_f32(ptr(d.indptr), ptr(d.indices), ptr(ft), ptr(el), ptr(er), 0.2, None, None, 0, ptr(out),
                                   ptr(attn), g.n, heads, dim, current_stream()), "gts_gat_fwd_f32")
    _lib.check(lib.gts_gat_bwd_edge_f32(ptr(d.indptr), ptr(d.indices), ptr(ft), ptr(el), ptr(er), ptr(attn), ptr(gout), 0.2,
                                        ptr(ge), ptr(ger), g.n, heads, dim, current_stream()), "gts_gat_bwd_edge_f32")
    _lib.check(lib.gts_gat_bwd_src_f32(ptr(d.t_indptr), ptr(d.t_indices), ptr(d.t_pos), ptr(attn), ptr(ge), ptr(gout), ptr(al),
                                       ptr(ar), ptr(ger), ptr(gft), ptr(gel), g.n, heads, dim, current_stream()),
               "gts_gat_bwd_src_f32")
    for what, t in (("out", out), ("attn", attn), ("ge", ge), ("ger", ger), ("gft", gft), ("gel", gel)):
        assert not bool(torch.isnan(t).any()), what
    _hold("attn", attn, ref["fwd"]["a"], ref["fb"]["a"])
    _hold("gft_folded", gft, ref["bwd"]["gft_folded"], ref["bb"]["gft_folded"])
    # ge is what gel and ger are sums of
    _hold("ger", torch.zeros_like(ger).index_add(0, g.dst_of_slot.to(DEV), ge), ref["bwd"]["ger"], ref["bb"]["ger"])


# ---------------------------------------------------------------- epilogue
@pytest.mark.parametrize("heads,dim", [(4, 256), (2, 65)])
@pytest.mark.parametrize("bias,residual,elu", [(b, r, e) for b in (0, 1) for r in (0, 1) for e in (0, 1)])
def test_epilogue_combinations_are_inside_the_forward_bound(bias, residual, elu, heads, dim):
    ref = R.reference_case("in", heads, dim, "unit")
    g, x = ref["g"], ref["x"]
    gen = torch.Generator().manual_seed(7)
    b = torch.randn(heads * dim, generator=gen) if bias else None
    r = torch.randn(g.n, heads * dim, generator=gen) if residual else None
    ft, el, er = _dev(x, "ft", "el", "er")
    out, _ = ops._gat_fwd(_graph(g), ft, el, er, 0.2, b.to(DEV) if bias else None, r.to(DEV) if residual else None, elu)
    fwd = dict(ref["fwd"], out=R.epilogue64(ref["fwd"]["agg"], b, r, bool(elu)))
    _hold("out", out, fwd["out"], R.forward_bounds(g, fwd, x["ft"], None, b, r, bool(elu))["out"])


# ---------------------------------------------------------------- exact cases, determinism, walk order, strided operands
@pytest.mark.parametrize("heads,dim", [(2, 256), (3, 20), (2, 65)])
def test_uniform_rows_of_power_of_two_degree_weigh_exactly_one_over_deg(heads, dim):
    """Equal scores: expf(0) = 1 and the denominator is an exact sum of ones."""
    g = R.graph_ladder(60, (1, 2, 4, 8, 64, 128), seed=9)
    gen = torch.Generator().manual_seed(3)
    el = torch.full((g.n, heads), 0.75)
    er = torch.randn(g.n, heads, generator=gen) * 10
    ft = torch.randn(g.n, heads, dim, generator=gen)
    out, attn = ops._gat_fwd(_graph(g), ft.to(DEV), el.to(DEV), er.to(DEV), 0.2)
    want = R.forward64(g, ft, el, er, 0.2)
    assert torch.equal(attn.cpu().double(), want["a"])
    assert torch.equal(want["a"][:, 0], 1.0 / torch.from_numpy(g.in_deg).double()[g.dst_of_slot])
    _hold("out", out, want["out"], R.forward_bounds(g, want, ft)["out"])


def _all_outputs(gd, ft, el, er, gout, al, ar):
    out, attn = ops._gat_fwd(gd, ft, el, er, 0.2)
    return (out, attn) + tuple(ops._gat_bwd(gd, ft, el, er, attn, gout, 0.2)) + tuple(ops._gat_bwd(gd, ft, el, er, attn, gout, 0.2, al, ar))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("heads,dim", [(4, 256), (3, 64)])
@pytest.mark.parametrize("kind", ["in", "out"])
def test_two_launches_give_the_same_bits_in_the_underflow_regime(kind, heads, dim):
    ref = R.reference_case(kind, heads, dim, "underflow")
    args = [_graph(ref["g"])] + _dev(ref["x"], "ft", "el", "er", "gout", "attn_l", "attn_r")
    first, second = _all_outputs(*args), _all_outputs(*args)
    for a, b in zip(first, second):
        assert _same_bits(a, b)


@pytest.mark.parametrize("heads,dim", [(4, 256), (3, 64), (2, 65)])
@pytest.mark.parametrize("kind", ["in", "out"])
def test_node_major_and_head_major_walks_give_the_same_bits(kind, heads, dim):
    """GTS_OPT_GAT_WALK only changes which wave computes a row."""
    lib = _lib.load()
    ref = R.reference_case(kind, heads, dim, "large")
    args = [_graph(ref["g"])] + _dev(ref["x"], "ft", "el", "er", "gout", "attn_l", "attn_r")
    assert lib.gts_get_option(OPT_GAT_WALK) == 1
    head_major = _all_outputs(*args)
    try:
        assert lib.gts_set_option(OPT_GAT_WALK, 0) == 0
        node_major = _all_outputs(*args)
    finally:
        lib.gts_set_option(OPT_GAT_WALK, 1)
    for a, b in zip(head_major, node_major):
        assert _same_bits(a, b)


def test_strided_operands_are_copied():
    ref = R.reference_case("in", 3, 64, "unit")
    gd = _graph(ref["g"])
    ft, el, er, gout, al, ar = _dev(ref["x"], "ft", "el", "er", "gout", "attn_l", "attn_r")
    want = _all_outputs(gd, ft, el, er, gout, al, ar)

    def strided(t):
        wide = torch.stack([t, t + 1], dim=-1)
        view = wide[..., 0]
        assert not view.is_contiguous() and torch.equal(view, t)
        return view
    got = _all_outputs(gd, *(strided(t) for t in (ft, el, er, gout, al, ar)))
    for a, b in zip(got, want):
        assert _same_bits(a, b)
    with pytest.raises(gts.GtsError):
        ops._gat_fwd(gd, ft.double(), el, er, 0.2)
    with pytest.raises(gts.GtsError):
        ops._gat_bwd(gd, ft, el, er, want[1], gout.cpu(), 0.2)


# ---------------------------------------------------------------- clustered kernels under the same scores
_CLUSTER_KERNELS = ("gts_gat_fwd_cluster_f32", "gts_gat_bwd_edge_cluster_f32", "gts_gat_bwd_src_cluster_f32")


def _cluster_graphs():
    lat = synth.lattice_graph((9, 8, 7))
    return {"lattice": R.RefGraph(lat.src.astype(np.int64), lat.dst.astype(np.int64), lat.n),
            "ladder64": R.graph_ladder(R.N_NODES, tuple(d for d in R.LADDER if d <= 64), seed=4),
            "out200": R.graph_ladder(2 * R.N_NODES, R.LADDER + (1,) * 15, seed=3, transpose=True, cap_other=64)}


# which schedules the builder takes (forward, edge pass, source pass); what it declines it declines for a reason of its own:
#   ladder64 'gat_edge_in': a row of 64 distinct sources is beyond the 50 neighbour slices of an edge-pass cluster
#   out200   'gat_out':     a row of 200 out-edges is beyond a cluster of the source pass (64 neighbours, 256 padded edges)
# and ops._gat_bwd only takes the clustered edge pass on rows of one 8-edge chunk (max in-degree <= 8).
_SCHEDULES = {"lattice": (True, True, True), "ladder64": (True, False, True), "out200": (True, True, False)}
_RAN = {"lattice": (True, True, True), "ladder64": (True, False, True), "out200": (True, False, False)}


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("name", ["lattice", "ladder64", "out200"])
def test_clustered_kernels_equal_the_plain_ones_bit_for_bit_in_every_regime(name, regime):
    rg = _cluster_graphs()[name]
    heads, dim = 4, 256
    gd = _graph(rg)
    assert gd.max_in_degree <= 64 and (name != "out200" or gd.max_out_degree == 200)
    for which, there in zip(("gat_in", "gat_edge_in", "gat_out"), _SCHEDULES[name]):
        sched = _clustered(lambda: ops._gat_cluster_schedule(gd, which, rg.n, heads, dim))
        assert (sched is not None) == there, which
        if not there:
            assert sched is None and gd.cluster_schedule(which) is None
    x = R.inputs(rg, heads, dim, regime, seed=len(name))
    args = [gd] + _dev(x, "ft", "el", "er", "gout", "attn_l", "attn_r")
    plain = _all_outputs(*args)
    ran = set()
    lib = _lib.load()
    real = {k: getattr(lib, k) for k in _CLUSTER_KERNELS}
    try:
        for k, fn in real.items():
            setattr(lib, k, (lambda k_, fn_: (lambda *a: (ran.add(k_), fn_(*a))[1]))(k, fn))
        clustered = _clustered(lambda: _all_outputs(*args))
    finally:
        for k, fn in real.items():
            setattr(lib, k, fn)
    assert ran == {k for k, on in zip(_CLUSTER_KERNELS, _RAN[name]) if on}
    for what, a, b in zip(("out", "attn", "gft", "gel", "ger", "gft_folded", "gel", "ger"), clustered, plain):
        assert _same_bits(a, b), what
    # the plain kernels on this graph, and with them the clustered ones, are inside the fp64 bounds
    fwd = R.forward64(rg, x["ft"], x["el"], x["er"], 0.2)
    fb = R.forward_bounds(rg, fwd, x["ft"])
    _hold("attn", clustered[1], fwd["a"], fb["a"])
    _hold("out", clustered[0], fwd["out"], fb["out"])
    bwd = R.backward64(rg, x["ft"], x["el"], x["er"], x["gout"], 0.2, x["attn_l"], x["attn_r"])
    bb = R.backward_bounds(rg, fwd, bwd, x["ft"], x["gout"], 0.2, attn_l=x["attn_l"], attn_r=x["attn_r"])
    for what, got in zip(("gft", "gel", "ger", "gft_folded"), clustered[2:6]):
        _hold(what, got, bwd[what], bb[what])
