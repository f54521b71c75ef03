"""The 4-wide first layer of a SAGEConv('pool') stack, backward (reference call sites: /root/reference/model/networks.py:25-30,
SAGEConv(in_feats, 256, 'pool') under autograd): gts_sage_first_layer_bwd_f32 streams the 256-wide gradient once where three
launches streamed it three times, and must give THE SAME BITS as those launches, which stay in the library and are the
oracle here: gts_linear_bwd_input_f32 for g @ W_neigh, gts_linear_bwd_weight_f32 (single problems (256, 4), with and
without bias) for the weight gradients.  Every comparison is torch.equal on int32 views (so -0.0 != 0.0 and no NaN games).

Row counts: 1 and 3 (fewer rows than the four row lanes of a chunk), 511 / 512 / 513 (one row per chunk; the step to two
rows per chunk with a short last chunk), 1 501 (three rows per chunk, a row count that is no multiple of four).

The 4-class top layer: gts_spmm_max_bwd_lowrank_f32 forms the rows of g @ W_neigh in registers where a panel GEMM stored
[N, 256] and K2 read it back; the oracle is those two steps as the stack issues them (gts_linear_bwd_input_t_f32 on the
transposed, packed weights, then K2).  Graphs of 1 .. 1 500 rows whose out-degrees cycle through 0, 1, 8 and 9 (no edge, one
edge, a whole chunk of K2's walk, a chunk and one more), and one of 27 700 rows, the smallest size at which the product
comes from the 16x16x4 panel kernel as at the headline shape (below that the 32x32x2 tiles make it); rows whose every
winner is "none"; finite g from 1e-30 to 1e30 and exact zeros of both signs.

The whole stack: 4 -> 256 -> 256 -> 4 at 1 500 rows, every gradient through the new plan (issued from Python and by
gts_sage_pool_stack_bwd_f32) against the old plan, assembled from the retained entry points."""
import numpy as np
import pytest
import torch

import gts
from gts import dense, ops, synth
from gts import nn as gnn

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    assert torch.equal(_bits(got), _bits(want)), what


def _operands(m, seed, zero_m0=False):
    gen = torch.Generator().manual_seed(seed)
    # magnitudes over many binades, both signs, exact zeros of both signs: sums whose rounding depends on their order
    g = torch.randn(m, 256, generator=gen) * torch.exp2(torch.randint(-20, 20, (m, 256), generator=gen).float())
    g[torch.rand(m, 256, generator=gen) < 0.05] = 0.0
    g[torch.rand(m, 256, generator=gen) < 0.05] = -0.0
    x = torch.randn(m, 4, generator=gen)
    m0 = torch.zeros(m, 4) if zero_m0 else torch.relu(torch.randn(m, 4, generator=gen))   # max-pooled ReLU outputs
    w_neigh = torch.randn(256, 4, generator=gen) * 0.1
    return [t.to(DEV) for t in (g, x, m0, w_neigh)]


@pytest.mark.parametrize("m,zero_m0", [(1, False), (3, False), (511, False), (512, False), (513, False), (1501, False),
                                       (1501, True)])
def test_first_layer_backward_in_one_pass_equals_its_three_launches_bit_for_bit(m, zero_m0):
    g, x, m0, w_neigh = _operands(m, seed=m + int(zero_m0), zero_m0=zero_m0)
    want_gm = dense.linear_bwd_input(g, w_neigh)
    want_ws, want_b = dense.linear_bwd_weight(g, x, want_bias_grad=True)
    want_wn, none = dense.linear_bwd_weight(g, m0)
    assert none is None
    gm, gw_self, g_bias, gw_neigh = dense.sage_first_layer_bwd(g, x, m0, w_neigh)
    _same_bits(gm, want_gm, "g @ W_neigh")
    _same_bits(gw_self, want_ws, "fc_self.weight gradient")
    _same_bits(g_bias, want_b, "bias gradient")
    _same_bits(gw_neigh, want_wn, "fc_neigh.weight gradient")
    if zero_m0:
        assert not gw_neigh.any()
    # not vacuous: the oracle's values are the products they stand for
    assert torch.allclose(want_gm.double(), g.double() @ w_neigh.double(), rtol=1e-4, atol=1e-3 * float(g.abs().max()))
    assert torch.allclose(want_b.double(), g.double().sum(0), rtol=1e-4, atol=1e-3 * float(g.abs().max()))


def test_first_layer_entry_point_takes_its_shape_only():
    lib = gts._lib.load()
    assert lib.gts_sage_first_layer_bwd_workspace(1000, 256, 4, 4) == 512 * 9 * 256 * 4
    for m, w, s0, s1 in ((0, 256, 4, 4), (1000, 128, 4, 4), (1000, 256, 8, 4), (1000, 256, 4, 8), (1 << 31, 256, 4, 4)):
        assert lib.gts_sage_first_layer_bwd_workspace(m, w, s0, s1) == 0
    t = torch.zeros(1000, 256, device=DEV)
    p = t.data_ptr()
    assert lib.gts_sage_first_layer_bwd_f32(p, p, p, p, p, p, p, p, p, 1 << 30, 1000, 128, 4, 4, None) == -2
    assert lib.gts_sage_first_layer_bwd_f32(p, p, p, p, p, p, p, p, p, 16, 1000, 256, 4, 4, None) == -2     # workspace too small
    assert lib.gts_sage_first_layer_bwd_f32(p, p, None, p, p, p, p, p, p, 1 << 30, 1000, 256, 4, 4, None) == -1
    x = torch.zeros(1000, 8, device=DEV)
    assert not dense.first_layer_bwd_applies(t, x, x, torch.zeros(256, 8, device=DEV))
    with pytest.raises(gts.GtsError):
        dense.sage_first_layer_bwd(t, x, x, torch.zeros(256, 8, device=DEV))


def _degree_cycle_graph(n):
    """Source u has out-degree (0, 1, 8, 9)[u % 4]; destinations spread over the rows (multi-edges and loops allowed)."""
    deg = np.array([0, 1, 8, 9])[np.arange(n) % 4]
    src = np.repeat(np.arange(n), deg)
    j = np.arange(src.size) - np.repeat(np.cumsum(deg) - deg, deg)
    dst = (src * 7 + j * 3 + 1) % n
    return gts.Graph(src, dst, n)


def _top_layer_operands(g, seed):
    gen = torch.Generator().manual_seed(seed)
    n = g.n
    mag = torch.pow(10.0, torch.rand(n, 4, generator=gen) * 60 - 30)
    grad = mag * torch.where(torch.rand(n, 4, generator=gen) < 0.5, -1.0, 1.0)
    grad[torch.rand(n, 4, generator=gen) < 0.1] = 0.0
    grad[torch.rand(n, 4, generator=gen) < 0.1] = -0.0
    w = torch.randn(4, 256, generator=gen) * 0.1
    w[torch.rand(4, 256, generator=gen) < 0.05] = 0.0
    w[torch.rand(4, 256, generator=gen) < 0.05] = -0.0
    # winners: a slot of the row's in-edges or "none" (0xFF); every fifth row has no winner at all
    in_deg = torch.from_numpy(np.diff(g.indptr).astype(np.int64))
    assert int(in_deg.max()) <= 254
    slot = (torch.rand(n, 256, generator=gen) * in_deg[:, None].float()).long().clamp(max=254)
    none = (torch.rand(n, 256, generator=gen) < 0.3) | (in_deg[:, None] == 0) | (torch.arange(n)[:, None] % 5 == 4)
    arg = torch.where(none, torch.full_like(slot, 255), slot).to(torch.uint8)
    return grad.to(DEV), w.to(DEV), arg.to(DEV)


@pytest.mark.parametrize("n", [1, 2, 37, 1500, 27700])
def test_top_layer_k2_from_the_rank_4_gradient_equals_gemm_then_k2_bit_for_bit(n):
    g = _degree_cycle_graph(n)
    grad, w, arg = _top_layer_operands(g, seed=n)
    g = g.to(DEV)
    assert ops.lowrank_bwd_applies(grad, w, arg)
    (wt,), (wtp,) = dense.pack_weights([w], transposed=True, want_plain=True)     # as the stack's backward turns its weights
    gm = dense.linear_bwd_input_t(grad, wt, packed=(wtp, None))
    want = ops.spmm_max_bwd(g, gm, arg)
    got = ops.spmm_max_bwd_lowrank(g, grad, w, arg)
    _same_bits(got, want, "gradient w.r.t. fc_pool's output")
    # not vacuous: rows without out-edges are zero, the others mostly are not, and the product is the product
    out_deg = torch.from_numpy(np.diff(g.t_indptr)).to(DEV)
    assert not want[out_deg == 0].any()
    if n >= 37:
        assert want[out_deg > 0].count_nonzero() > want[out_deg > 0].numel() // 8
    ref = grad.double() @ w.double()
    assert torch.allclose(gm.double(), ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max()))


def test_top_layer_entry_point_takes_its_shape_only():
    lib = gts._lib.load()
    p = torch.zeros(1024, device=DEV).data_ptr()
    assert lib.gts_spmm_max_bwd_lowrank_f32(p, p, p, p, p, p, 1, p, 4, 128, 4, None) == -2
    assert lib.gts_spmm_max_bwd_lowrank_f32(p, p, p, p, p, p, 1, p, 4, 256, 8, None) == -2
    assert lib.gts_spmm_max_bwd_lowrank_f32(p, p, p, p, p, p, 2, p, 4, 256, 4, None) == -3
    assert lib.gts_spmm_max_bwd_lowrank_f32(p, p, p, None, p, p, 1, p, 4, 256, 4, None) == -1
    assert lib.gts_spmm_max_bwd_lowrank_f32(p, p, p, p, p, p, 1, p, 0, 256, 4, None) == 0


def _gradients(net, g, x, y, one_call):
    old = gnn.STACK_IN_ONE_CALL
    gnn.STACK_IN_ONE_CALL = one_call
    try:
        net.zero_grad(set_to_none=True)
        x = x.clone().requires_grad_(True)
        logits = net(g, x)
        ops.weighted_cross_entropy(logits, y, torch.tensor([0.1, 1.0, 2.0, 2.0], device=DEV)).backward()
        return [logits.detach(), x.grad] + [p.grad.clone() for p in net.parameters()]
    finally:
        gnn.STACK_IN_ONE_CALL = old


def test_stack_with_narrow_ends_equals_the_old_plan_bit_for_bit(monkeypatch):
    from collections import namedtuple

    from model.networks import init_graph_net

    hp = namedtuple("HP", "in_feats out_classes layer_sizes gat_heads gat_residuals")(4, 4, [256, 256], None, None)
    g = synth.geometric_graph(1500, 8, 4).to(DEV)
    torch.manual_seed(11)
    net = init_graph_net("GSpool", hp).to(DEV)
    x = torch.randn(g.n, 4, device=DEV)
    y = torch.randint(0, 4, (g.n,), device=DEV)
    calls = []
    first, top = dense.sage_first_layer_bwd, ops.spmm_max_bwd_lowrank
    monkeypatch.setattr(dense, "sage_first_layer_bwd", lambda *a: calls.append("first") or first(*a))
    monkeypatch.setattr(ops, "spmm_max_bwd_lowrank", lambda *a: calls.append("top") or top(*a))
    new_python = _gradients(net, g, x, y, one_call=False)
    assert calls == ["top", "first"], "the launch-by-launch plan takes both narrow-end passes"
    new_c = _gradients(net, g, x, y, one_call=True)
    # the old plan: the same stack, launch by launch, both ends through the entry points they used to call
    monkeypatch.setattr(dense, "first_layer_bwd_applies", lambda *a: False)
    monkeypatch.setattr(ops, "lowrank_bwd_applies", lambda *a: False)
    old = _gradients(net, g, x, y, one_call=False)
    assert calls == ["top", "first"]
    names = ["logits", "x.grad"] + [k for k, _ in net.named_parameters()]
    assert len(old) == len(names) == 2 + 15
    for name, want, a, b in zip(names, old, new_python, new_c):
        _same_bits(a, want, f"{name} (plan issued from Python)")
        _same_bits(b, want, f"{name} (gts_sage_pool_stack_bwd_f32)")
