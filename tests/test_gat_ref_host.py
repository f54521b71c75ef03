"""The float64 reference and the bounds of tests/test_gpu_gat_edges.py, validated on the CPU (tests/gat_ref.py), and the
host-side refusals of ops._gat_fwd / ops._gat_bwd, which need no device: they come before the library is loaded."""
import numpy as np
import pytest
import torch

import gts
from gts import _lib, ops
from oracle import torch_ref
from tests import gat_ref as R


# ---------------------------------------------------------------- graphs
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("n", [15, 203, 40])
def test_ladder_graph_has_exactly_the_stated_degrees(n, transpose):
    g = R.graph_ladder(n, R.LADDER, seed=n, transpose=transpose)
    want = np.array([R.LADDER[v % len(R.LADDER)] for v in range(n)])
    assert np.array_equal(g.out_deg if transpose else g.in_deg, want)
    assert g.number_of_edges() == want.sum()
    assert np.all(np.diff(g.dst) >= 0)                                      # in-CSR order
    assert np.array_equal(np.diff(g.indptr), g.in_deg)
    assert 0 <= g.src.min() and g.src.max() < n and 0 <= g.dst.min() and g.dst.max() < n
    if n >= len(R.LADDER):
        assert set(want) == set(R.LADDER)
        assert np.all(want[:-1] != want[1:])                                # neighbouring rows differ in degree


def test_the_graphs_of_the_device_test():
    for kind in ("in", "out"):
        g = R.ladder(kind)
        deg = g.in_deg if kind == "in" else g.out_deg
        assert g.n == 203 and {0, 7, 8, 9, 63, 64, 65, 128, 200} <= set(deg)
    capped = R.graph_ladder(406, R.LADDER + (1,) * 15, seed=3, transpose=True, cap_other=64)
    assert capped.in_deg.max() <= 64 and capped.out_deg.max() == 200
    with pytest.raises(ValueError):
        R.graph_ladder(30, R.LADDER, seed=3, transpose=True, cap_other=8)


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("kind", ["in", "out"])
def test_fp64_forward_is_the_oracle_on_doubles(kind):
    """Integer scores and slope 0.5: the fp32 score is exact, so the two agree to float64 rounding.  Random scores: they
    differ by the rounding of the fp32 score alone."""
    g = R.ladder(kind)
    for regime, slope, tol in (("integer", 0.5, 1e-13), ("unit", 0.2, 2e-6)):
        x = R.inputs(g, 2, 20, regime, seed=4)
        fwd = R.forward64(g, x["ft"], x["el"], x["er"], slope)
        out, a = torch_ref.gat_aggregate(g, x["ft"].double(), x["el"].double(), x["er"].double(), slope)
        assert torch.allclose(fwd["a"], a, rtol=tol, atol=0) and torch.allclose(fwd["out"], out, rtol=0, atol=tol * 10)
        assert torch.equal(fwd["out"], fwd["agg"])
        rows = torch.from_numpy(g.in_deg > 0)
        assert torch.allclose(R._row_sum(g, fwd["a"])[rows], torch.ones(1, dtype=torch.float64))
        assert torch.equal(fwd["s"].float(), R.score_f32(fwd["pre"], slope)) and fwd["s"].dtype == torch.float64
        assert bool((fwd["s"] <= fwd["m"][g.dst_of_slot]).all())
        assert bool(torch.isinf(fwd["m"][~rows]).all()) and bool((fwd["out"][~rows] == 0).all())


def test_fp64_backward_is_the_oracles_autograd_on_doubles_and_folds():
    g = R.ladder("in")
    x = R.inputs(g, 2, 20, "integer", seed=5)
    bwd = R.backward64(g, x["ft"], x["el"], x["er"], x["gout"], 0.5, x["attn_l"], x["attn_r"])
    leaves = [x[k].double().requires_grad_(True) for k in ("ft", "el", "er")]
    # integer scores: pre == 0 on many edges, where torch's leaky_relu' is the slope too
    torch_ref.gat_aggregate(g, *leaves, 0.5)[0].backward(x["gout"].double())
    for name, leaf in zip(("gft", "gel", "ger"), leaves):
        assert torch.allclose(bwd[name], leaf.grad, rtol=1e-12, atol=1e-12), name
    folded = bwd["gft"] + bwd["gel"][:, :, None] * x["attn_l"].double() + bwd["ger"][:, :, None] * x["attn_r"].double()
    assert torch.equal(bwd["gft_folded"], folded)
    plain = R.backward64(g, x["ft"], x["el"], x["er"], x["gout"], 1.0, leaky=False)
    slope1 = R.backward64(g, x["ft"], x["el"], x["er"], x["gout"], 1.0)
    for name in ("gft", "gel", "ger"):
        assert torch.equal(plain[name], slope1[name])


@pytest.mark.parametrize("deg", [1, 2, 4, 8, 64, 128])
def test_equal_scores_and_power_of_two_degree_give_exactly_one_over_deg(deg):
    g = R.graph_ladder(40, (deg,), seed=deg)
    el = torch.full((40, 3), 0.75)
    er = torch.randn(40, 3, generator=torch.Generator().manual_seed(1)) * 10
    fwd = R.forward64(g, torch.ones(40, 3, 4), el, er, 0.2)
    assert torch.equal(fwd["a"], torch.full_like(fwd["a"], 1.0 / deg))
    _, a32 = torch_ref.gat_aggregate(g, torch.ones(40, 3, 4), el, er, 0.2)
    assert torch.equal(a32, torch.full_like(a32, 1.0 / deg))


# ---------------------------------------------------------------- constants and bounds
def test_constants_are_four_times_the_measured_ratios():
    assert R.C0 == 4.0 * R.MEASURED_FWD_AT_C0_1 and R.CB == 4.0 * R.MEASURED_BWD_AT_CB_1
    assert R.U == 2.0 ** -24 and R.FLOOR == 2.0 ** -126


@pytest.mark.parametrize("kind,heads,dim,regime", R.cases())
def test_fp32_oracle_is_inside_every_bound_with_the_constants_and_with_half_of_them(kind, heads, dim, regime):
    """Keeps the constants honest: the oracle they were measured on stays inside, and still does with both halved — the
    4x margin is there for the device and is not consumed by the oracle."""
    full = R.oracle_ratios(kind, heads, dim, regime, R.C0, R.CB)
    half = R.oracle_ratios(kind, heads, dim, regime, R.C0 / 2, R.CB / 2)
    for name in ("a", "out", "gft", "gel", "ger"):
        assert full[name] <= 1.0 and half[name] <= 1.0, (name, full[name], half[name])


@pytest.mark.parametrize("bias,residual,elu", [(b, r, e) for b in (0, 1) for r in (0, 1) for e in (0, 1)])
def test_fp32_epilogue_is_inside_the_forward_bound(bias, residual, elu):
    g = R.ladder("in")
    x = R.inputs(g, 2, 65, "unit", seed=6)
    gen = torch.Generator().manual_seed(7)
    b = torch.randn(2 * 65, generator=gen) if bias else None
    r = torch.randn(g.n, 2 * 65, generator=gen) if residual else None
    fwd = R.forward64(g, x["ft"], x["el"], x["er"], 0.2, b, r, bool(elu))
    got, _ = torch_ref.gat_aggregate(g, x["ft"], x["el"], x["er"], 0.2)
    if r is not None:
        got = got + r.reshape(got.shape)
    if b is not None:
        got = got + b.reshape(1, 2, 65)
    if elu:
        got = torch.nn.functional.elu(got)
    for c0 in (R.C0, R.C0 / 2):
        bound = R.forward_bounds(g, fwd, x["ft"], c0, b, r, bool(elu))["out"]
        assert R.worst_ratio(got, fwd["out"], bound) <= 1.0
    assert bool((fwd["out"][torch.from_numpy(g.in_deg == 0)]
                 == R.epilogue64(torch.zeros_like(fwd["agg"]), b, r, bool(elu))[torch.from_numpy(g.in_deg == 0)]).all())


def test_bounds_notice_a_wrong_kernel():
    """The bars are tight enough to fail the mistakes they are there for, restated on the CPU in fp32: no maximum
    subtracted (weights overflow or lose their small terms), `>=` in leaky', one edge dropped from a sum."""
    g = R.ladder("in")
    ref = R.reference_case("in", 3, 64, "integer")
    x, fwd, bwd = ref["x"], ref["fwd"], ref["bwd"]
    pre = R.pre_f32(g, x["el"], x["er"])
    assert float((pre == 0).float().mean()) > 0.05
    s = R.score_f32(pre, 0.2).double().requires_grad_(True)
    R._aggregate(g, x["ft"].double(), s)[0].backward(x["gout"].double())
    slope = float(torch.tensor(0.2, dtype=torch.float32))
    for at_zero, wrong in ((slope, False), (1.0, True)):                       # `>` (right) and `>=` (wrong) at pre == 0
        ge = s.grad * torch.where(pre > 0, 1.0, torch.where(pre == 0, at_zero, slope)).double()
        ratio = R.worst_ratio(R._row_sum(g, ge, "dst"), bwd["ger"], ref["bb"]["ger"])
        assert ratio > 100 if wrong else ratio == 0.0
    # a dropped edge
    msg = x["ft"][g.indices] * fwd["a"].float()[:, :, None]
    msg[g.indptr[8 + 1] - 1] = 0                                              # the last edge of a 63-edge row
    out = torch.zeros_like(x["ft"]).index_add(0, g.dst_of_slot, msg)
    assert R.worst_ratio(out, fwd["out"], ref["fb"]["out"]) > 100
    # exp without the maximum: harmless while exp(score) is finite (the large regime), inf / inf in the underflow regime
    big = R.reference_case("in", 3, 64, "underflow")
    e = torch.exp(big["fwd"]["s"].float())
    a = e / torch.zeros(g.n, 3).index_add(0, g.dst_of_slot, e)[g.dst_of_slot]
    assert R.worst_ratio(a, big["fwd"]["a"], big["fb"]["a"]) > 1.0


# ---------------------------------------------------------------- regime facts the device tests rely on
def test_regime_facts():
    g = R.ladder("in")
    x = R.inputs(g, 4, 8, "underflow", seed=8)
    o = R.oracle32(g, x["ft"], x["el"], x["er"], x["gout"], 0.2)
    assert float((o["a"] == 0).float().mean()) > 0.30
    for t in o.values():
        assert bool(torch.isfinite(t).all())
    ref = R.forward64(g, x["ft"], x["el"], x["er"], 0.2)
    assert bool(torch.isfinite(ref["out"]).all()) and float((ref["s"] - ref["m"][g.dst_of_slot]).abs().max()) > 104
    x = R.inputs(g, 4, 8, "large", seed=8)
    o = R.oracle32(g, x["ft"], x["el"], x["er"], x["gout"], 0.2)
    assert bool((o["a"] > 0).all()) and 30 < float(R.pre_f32(g, x["el"], x["er"]).abs().max()) < 90
    x = R.inputs(g, 4, 8, "integer", seed=8)
    pre = R.pre_f32(g, x["el"], x["er"])
    assert float((pre == 0).float().mean()) > 0.05
    s = R.forward64(g, x["ft"], x["el"], x["er"], 0.2)
    ties = (s["s"] == s["m"][g.dst_of_slot]).double()
    assert float(R._row_sum(g, ties).max()) > 1                                # the row maximum is attained more than once


def test_worst_ratio_leaves_nothing_out():
    want, bound = torch.zeros(4, dtype=torch.float64), torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64)
    assert R.worst_ratio(torch.zeros(4), want, bound) == 0.0
    assert R.worst_ratio(torch.tensor([0.0, 0.5, 0.0, 0.0]), want, bound) == 0.5
    assert R.worst_ratio(torch.tensor([0.0, 0.0, 0.0, 1e-30]), want, bound) == float("inf")     # error over a zero bound
    assert R.worst_ratio(torch.tensor([float("nan"), 0.0, 0.0, 0.0]), want, bound) == float("inf")


# ---------------------------------------------------------------- wrapper refusals that need no device
@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to reach the library fails the test: the refusals below are decided on the host before that."""
    def load():
        raise AssertionError("the wrapper reached _lib.load() with operands it must refuse")
    monkeypatch.setattr(_lib, "load", load)


def _tiny_graph():
    return gts.Graph(np.array([0, 1, 2, 2]), np.array([1, 2, 0, 1]), 3)


def test_gat_fwd_refuses_on_the_host(no_library):
    g = _tiny_graph()
    ft, e = torch.zeros(3, 2, 4), torch.zeros(3, 2)
    b, r = torch.zeros(8), torch.zeros(3, 8)
    for args, kw in [((ft.reshape(3, 8), e, e), {}), ((ft[:2], e[:2], e[:2]), {}), ((ft, e[:, :1], e), {}), ((ft, e, e.t()), {}),
                     ((ft, e, e), dict(bias=b[:4])), ((ft, e, e), dict(residual=r[:2])), ((ft, e, e), dict(activation=2)),
                     ((ft.double(), e, e), {}), ((ft, e.double(), e), {}), ((ft, e, e.half()), {}),       # dtype
                     ((ft, e, e), dict(bias=b.double())), ((ft, e, e), dict(residual=r.double())),
                     ((ft, e, e), {}), ((ft, e, e), dict(bias=b, residual=r, activation=1))]:            # CPU tensors
        with pytest.raises(gts.GtsError):
            ops._gat_fwd(g, *args, 0.2, **kw)


def test_gat_bwd_refuses_on_the_host(no_library):
    g = _tiny_graph()
    ft, e, a = torch.zeros(3, 2, 4), torch.zeros(3, 2), torch.zeros(4, 2)
    v = torch.zeros(2, 4)
    for args in [(ft.reshape(3, 8), e, e, a, ft), (ft, e[:2], e, a, ft), (ft, e, e, a[:3], ft), (ft, e, e, a, ft[:, :1]),
                 (ft, e, e, a, ft, v[:1], v), (ft, e, e, a, ft, v, None), (ft, e, e, a, ft, None, v),
                 (ft.double(), e, e, a, ft), (ft, e, e.double(), a, ft), (ft, e, e, a.double(), ft), (ft, e, e, a, ft.double()),
                 (ft, e, e, a, ft, v.double(), v), (ft, e, e, a, ft, v, v.double()),
                 (ft, e, e, a, ft), (ft, e, e, a, ft, v, v)]:                                             # CPU tensors
        with pytest.raises(gts.GtsError):
            ops._gat_bwd(g, *args[:5], 0.2, *args[5:])
