"""The turn of the training step at a 256 -> 4 top SAGEConv('pool') layer: gts_sage_top_layer_train_f32 forms the logits,
the weighted cross-entropy, the gradient w.r.t. the logits and the layer's three narrow weight gradients in ONE pass over
the layer's input h and its max-pooled neighbours m (plus a labels-only launch before and one finish launch after), where
the step used to stream both 256-wide tensors twice.  It must give THE SAME BITS as the launches it stands for, which stay
in the library and are the oracle here: gts_linear_fwd_f32 -> gts_weighted_ce_f32 -> torch's div_ by the denominator ->
gts_linear_bwd_weight_f32 (two problems (4, 256), one with bias).  Every comparison is torch.equal on int32 views (so
-0.0 != 0.0, and a NaN must be the same NaN).

Row counts: 1, 3, 4, 5 (the four-row groups of a wave, fewer rows than row lanes), 511 / 512 / 513 (one row per chunk of
the 512-chunk walk; the step to two rows per chunk with a short last chunk), 1 023 / 1 025 (the edge of the loss's
1 024-row blocks), 1 501 (three rows per chunk, no multiple of four).  Labels: -100 on some rows, on every row (den = 0),
one label out of range (NaN loss).  Class weights given and absent; the denominator's division on and off; a logits row
holding +-inf.

The whole stack: 4 -> 256 -> 256 -> 4 at 1 500 rows through both copies of the new plan (issued from Python and by
gts_sage_pool_stack_train_fwd_f32 / _bwd_top_f32) against the plan through autograd, and GNN.train_step on a two-graph
batch against the same steps with the variant switched off, single-GPU branch and data-parallel branch."""
import io
from collections import namedtuple
from contextlib import redirect_stdout

import pytest
import torch

import gts
from gts import dense, ops, synth
from gts import nn as gnn

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = [1, 3, 4, 5, 511, 512, 513, 1023, 1025, 1501]
CLASS_W = [0.1, 1.0, 2.0, 2.0]


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    assert torch.equal(_bits(got), _bits(want)), what


def _operands(m, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    h = torch.relu(torch.randn(m, 256, generator=gen)) * torch.exp2(torch.randint(-6, 6, (m, 256), generator=gen).float())
    mx = torch.relu(torch.randn(m, 256, generator=gen))            # max-pooled ReLU outputs: many exact zeros
    w_self, w_neigh = (torch.randn(4, 256, generator=gen) * 0.05 * scale for _ in range(2))
    bias = torch.randn(4, generator=gen)
    labels = torch.randint(0, 4, (m,), generator=gen)
    return [t.to(DEV) for t in (h, mx, w_self, w_neigh, bias, labels)]


def _oracle(h, mx, w_self, w_neigh, bias, labels, class_w, normalise):
    logits = dense.linear_fwd(h, w_self, mx, w_neigh, bias=bias)
    grad, stats = ops.weighted_ce_numerator_grad(logits, labels, class_w)
    if normalise:
        grad.div_(stats[1])
    (gw_self, g_bias), (gw_neigh, none) = dense.linear_bwd_weight_multi([(grad, h, True), (grad, mx, False)])
    assert none is None
    return logits, grad, gw_self, gw_neigh, g_bias, stats


def _check(operands, class_w, normalise, what):
    want = _oracle(*operands, class_w, normalise)
    got = dense.sage_top_layer_train(*operands, class_w, normalise)
    for name, a, b in zip(("logits", "g", "gw_self", "gw_neigh", "g_bias", "stats"), got, want):
        _same_bits(a, b, f"{name}: {what}")
    return want


@pytest.mark.parametrize("m", ROWS)
def test_top_layer_pass_equals_its_launches_bit_for_bit(m):
    operands = _operands(m, seed=m)
    class_w = torch.tensor(CLASS_W, device=DEV)
    logits, grad, gw_self, _, g_bias, stats = _check(operands, class_w, True, "weights, mean")
    _check(operands, None, True, "no class weights, mean")
    _check(operands, class_w, False, "weights, numerator's gradient")
    _check(operands, None, False, "no class weights, numerator's gradient")
    # not vacuous: the oracle's values are what they stand for
    h, mx, w_self, w_neigh, bias, labels = operands
    ref = h.double() @ w_self.double().t() + mx.double() @ w_neigh.double().t() + bias.double()
    assert torch.allclose(logits.double(), ref, rtol=1e-4, atol=1e-3)
    ref_loss = torch.nn.functional.cross_entropy(ref, labels, weight=class_w.double())
    assert abs(float(stats[2]) - float(ref_loss)) <= 1e-4 * max(1.0, abs(float(ref_loss)))
    assert torch.allclose(g_bias.double(), grad.double().sum(0), rtol=1e-4, atol=1e-6)
    assert torch.allclose(gw_self.double(), grad.double().t() @ h.double(), rtol=1e-4, atol=1e-4)
    assert grad.count_nonzero() > 0


@pytest.mark.parametrize("m", [5, 513, 1025, 1501])
def test_top_layer_pass_keeps_the_label_rules(m):
    operands = _operands(m, seed=100 + m)
    class_w = torch.tensor(CLASS_W, device=DEV)
    labels = operands[5]
    some = labels.clone()
    some[::3] = -100
    for normalise in (True, False):
        for cw in (class_w, None):
            want = _check(operands[:5] + [some], cw, normalise, "-100 on every third row")
            assert not want[1][::3].any() and torch.isfinite(want[5]).all()
            every = torch.full_like(labels, -100)
            want = _check(operands[:5] + [every], cw, normalise, "-100 on every row: den = 0")
            assert float(want[5][1]) == 0.0
            for bad_value in (4, -1, 1 << 40):
                bad = labels.clone()
                bad[m // 2] = bad_value
                want = _check(operands[:5] + [bad], cw, normalise, f"label {bad_value} on one row")
                assert torch.isnan(want[5][0]) and torch.isnan(want[5][2]) and not want[1][m // 2].any()


@pytest.mark.parametrize("m", [4, 513, 1501])
def test_top_layer_pass_keeps_non_finite_logits(m):
    # two weight rows scaled until their products with one large row overflow: a logits row holding +inf and -inf, NaN
    # gradients behind it
    h, mx, w_self, w_neigh, bias, labels = _operands(m, seed=200 + m)
    h[m // 3] = 1e30
    w_self[0], w_self[1] = 1e10, -1e10
    operands = [h, mx, w_self, w_neigh, bias, labels]
    class_w = torch.tensor(CLASS_W, device=DEV)
    for normalise in (True, False):
        logits, grad = _check(operands, class_w, normalise, "a row of non-finite logits")[:2]
        assert float(logits[m // 3, 0]) == float("inf") and float(logits[m // 3, 1]) == float("-inf")
        assert torch.isfinite(logits).sum() == 4 * m - 2 and torch.isnan(grad[m // 3]).any()


def test_top_layer_entry_point_takes_its_shape_only():
    lib = gts._lib.load()
    t = torch.zeros(1000, 256, device=DEV)
    assert not dense.top_layer_train_applies(t, t, torch.zeros(8, 256, device=DEV), torch.zeros(4, 256, device=DEV))
    assert not dense.top_layer_train_applies(t[:, :128], t[:, :128], torch.zeros(4, 128, device=DEV), torch.zeros(4, 128, device=DEV))
    labels = torch.zeros(1000, dtype=torch.int64, device=DEV)
    with pytest.raises(gts.GtsError):
        dense.sage_top_layer_train(t, t, torch.zeros(8, 256, device=DEV), torch.zeros(8, 256, device=DEV),
                                   torch.zeros(8, device=DEV), labels)
    with pytest.raises(gts.GtsError):
        dense.sage_top_layer_train(t, t, torch.zeros(4, 256, device=DEV), torch.zeros(4, 256, device=DEV),
                                   torch.zeros(4, device=DEV), labels.int())
    assert lib.gts_sage_top_layer_train_workspace(1000, 256, 4) > 0


# ---------------------------------------------------------------------------------------------------- the stack
HP = namedtuple("HP", "in_feats out_classes layer_sizes gat_heads gat_residuals")


def _through_autograd(net, g, x, y, class_w):
    """The plan without the variant: forward, weighted CE, div_, backward into a sink, as GNN.train_step issues them."""
    sink = gnn.GradSink(list(net.parameters()))
    logits = net(g, x)
    grad, stats = ops.weighted_ce_numerator_grad(logits, y, class_w)
    grad.div_(stats[1])
    flat = sink.new_buffer()
    with gnn.grad_sink(sink):
        logits.backward(grad)
    assert sink.filled
    return logits.detach(), stats, flat


def _variant(net, g, x, y, class_w, one_call):
    old = gnn.STACK_IN_ONE_CALL
    gnn.STACK_IN_ONE_CALL = one_call
    try:
        sink = gnn.GradSink(list(net.parameters()))
        done = gnn.sage_pool_stack_train(g, x, list(net.layers), y, class_w, sink)
        assert done is not None and sink.filled
        return done[0], done[1], sink.flat
    finally:
        gnn.STACK_IN_ONE_CALL = old


def test_stack_with_the_top_turn_equals_the_plan_through_autograd_bit_for_bit(monkeypatch):
    from model.networks import init_graph_net

    g = synth.geometric_graph(1500, 8, 4).to(DEV)
    torch.manual_seed(11)
    net = init_graph_net("GSpool", HP(4, 4, [256, 256], None, None)).to(DEV)
    x = torch.randn(g.n, 4, device=DEV)
    y = torch.randint(0, 4, (g.n,), device=DEV)
    y[::7] = -100
    class_w = torch.tensor(CLASS_W, device=DEV)
    want = _through_autograd(net, g, x, y, class_w)
    calls = []
    top = dense.sage_top_layer_train
    monkeypatch.setattr(dense, "sage_top_layer_train", lambda *a, **k: calls.append("top") or top(*a, **k))
    new_python = _variant(net, g, x, y, class_w, one_call=False)
    assert calls == ["top"], "the launch-by-launch plan takes the top-layer pass"
    new_c = _variant(net, g, x, y, class_w, one_call=True)
    assert calls == ["top"]
    assert want[2].count_nonzero() > want[2].numel() // 2
    for name, w, a, b in zip(("logits", "stats", "flat gradients"), want, new_python, new_c):
        _same_bits(a, w, f"{name} (plan issued from Python)")
        _same_bits(b, w, f"{name} (gts_sage_pool_stack_train_fwd_f32 / _bwd_top_f32)")
    # a stack with another top layer keeps the path through autograd
    other = init_graph_net("GSpool", HP(4, 4, [64], None, None)).to(DEV)
    assert gnn.sage_pool_stack_train(g, x, list(other.layers), y, class_w, gnn.GradSink(list(other.parameters()))) is None


def _train_steps(top_turn, data_parallel):
    from gts import dist as gdist
    from model.gnn_model import GNN
    from utils.hyperparam_helpers import FullParamSet

    hp = FullParamSet(1, 20, 4, 1e-3, 0.98, 1e-4, [0.1, 1, 2, 2], [256, 256], 0, None, None)
    g = gts.batch([synth.lattice_graph((9, 8, 7)), synth.lattice_graph((6, 6, 6))]).to(DEV)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(g.n, 20, generator=gen).to(DEV)
    y = torch.randint(0, 4, (g.n,), generator=gen).to(DEV)
    old = gnn.TOP_TURN
    gnn.TOP_TURN = top_turn
    try:
        torch.manual_seed(5)
        with redirect_stdout(io.StringIO()):
            model = GNN("GSpool", hp, None)
        model.net.train()
        if data_parallel:      # the branch of a data-parallel run, here with one rank: no collective is issued
            model.grad_sync = gdist.FlatGradSync(model.net.parameters())
        losses = [model.train_step(g, x, y).clone() for _ in range(3)]
        return losses, {k: v.clone() for k, v in model.net.state_dict().items()}
    finally:
        gnn.TOP_TURN = old


@pytest.mark.parametrize("data_parallel", [False, True])
def test_train_step_with_the_top_turn_trains_the_same_network(data_parallel, monkeypatch):
    calls = []
    train = gnn.sage_pool_stack_train

    def spy(*a, **k):
        done = train(*a, **k)
        calls.append(done is not None)
        return done

    monkeypatch.setattr(gnn, "sage_pool_stack_train", spy)
    want_losses, want_state = _train_steps(False, data_parallel)
    got_losses, got_state = _train_steps(True, data_parallel)
    assert calls == [False] * 3 + [True] * 3, "switched off, the step goes through autograd; switched on, it does not"
    for a, b in zip(got_losses, want_losses):
        _same_bits(a.reshape(1), b.reshape(1), "loss")
    assert float(want_losses[0]) != float(want_losses[2])
    for k in want_state:
        _same_bits(got_state[k], want_state[k], k)
