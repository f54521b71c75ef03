"""NaN / Inf through the HIP kernels against fp64 torch: a non-finite value that enters a kernel must come out where the
reference says it does, and nowhere else.

Two things are asserted on every entry.  (1) tests/nonfinite_ref.py::classes_match: NaN where the fp64 reference is NaN,
the same infinity where it is infinite, and elsewhere finite within the rounding bound of test_gpu_gemm.py /
test_gpu_conv3d.py (2e-6 x the operation on absolute values, non-finite inputs counted as 0).  The class rule is exact:
finite data is O(1) and zeros are placed explicitly.  (2) Fences: every operand and every output is carved out of a
NaN-filled buffer (nonfinite_ref.fenced), so a read past an operand that reaches an accumulator, "multiplied by zero" or
not, turns results NaN, and a write past an output breaks the pads' bit pattern.  All reads past an operand stay inside
one allocation of this test.

ReLU is torch.relu in fp64: relu(NaN) = NaN, relu(-0.0) = -0.0, relu(-Inf) = 0, relu(+Inf) = +Inf.  A ReLU MASK operand
(relu_mask, h) is always finite here: the gradient through a NaN mask is out of scope."""
import ctypes
from collections import namedtuple
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

from gts import _lib as glib
from gts import conv3d, dense, ops, synth
from gts import nn as gnn
from gts._lib import check, current_stream, ptr
from tests import conv3d_ref
from tests.dice_ref import dice_ce_ref
from tests.nonfinite_ref import classes_match, fence_intact, fenced, fenced_empty, zero_nonfinite

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _positions(size, seed):
    """First, last and one interior index chosen from the seed (fewer when the axis is shorter)."""
    out = [0, size - 1]
    if size > 2:
        out.insert(1, 1 + (seed * 7919 + 13) % (size - 2))
    return sorted(set(out))


def _same_bits(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


_OPTION_REST = {1: -1, 2: -1, 3: 1, 13: 0}      # the value each tile option has outside a forced test


@contextmanager
def _options(pairs):
    lib = glib.load()
    try:
        for opt, val in pairs:
            assert lib.gts_set_option(opt, val) == 0
        yield
    finally:
        for opt, _ in pairs:
            lib.gts_set_option(opt, _OPTION_REST[opt])


def _fences(pairs):
    """[(view, buf), ...] of device operands; None stays None."""
    return [(None, None) if t is None else fenced(t.to(DEV)) for t in pairs]


def _assert_fences(named):
    torch.cuda.synchronize()
    for name, (view, buf) in named.items():
        if view is not None:
            assert fence_intact(buf, view), f"the pads around {name} were written"


# ---------------------------------------------------------------------------------------------- layer GEMMs
KINDS = ["nan_a", "nan_w", "nan_bias", "inf_times_zero", "inf_minus_inf", "neg_inf_relu", "pos_inf_relu", "combined"]


def _inject(kind, a, bt, bias, seed):
    """Poison copies of the operands of C = a [m, k] @ bt [n, k]^T + bias [n] (bias may be None).  One position at a
    time along the first / last / interior rows and columns, and `combined` all at once."""
    a, bt = a.clone(), bt.clone()
    bias = None if bias is None else bias.clone()
    rows, red, cols = _positions(a.shape[0], seed), _positions(a.shape[1], seed + 1), _positions(bt.shape[0], seed + 2)
    if kind in ("nan_a", "combined"):
        for i, r in enumerate(rows[:1] if kind == "combined" else rows):
            a[r, red[i % len(red)]] = NAN
    if kind in ("nan_w", "combined"):
        for i, c in enumerate(cols[-1:] if kind == "combined" else cols):
            bt[c, red[-1 - i % len(red)]] = NAN
    if kind in ("nan_bias", "combined") and bias is not None:
        bias[cols[len(cols) // 2]] = NAN
    if kind in ("inf_times_zero", "combined"):          # 0 * Inf = NaN in the zeroed columns, +-Inf in the others
        for r in rows[-1:] if kind == "combined" else rows:
            a[r, red[0]] = INF
        bt[cols, red[0]] = 0.0
    if kind in ("inf_minus_inf", "neg_inf_relu", "pos_inf_relu"):
        bt = bt.abs()                                    # positive weights: the sign of the infinity is the operand's
        for r in rows:
            if kind == "inf_minus_inf":
                a[r, red[0]], a[r, red[-1]] = INF, -INF
            else:
                a[r, red[0]] = -INF if kind == "neg_inf_relu" else INF
    return a, bt, bias


def _ref_product(a, bt, bias=None):
    """(want, bound) of a @ bt^T + bias in fp64."""
    want = a.double() @ bt.double().t()
    bound = zero_nonfinite(a) @ zero_nonfinite(bt).t()
    if bias is not None:
        want, bound = want + bias.double(), bound + zero_nonfinite(bias)
    return want, bound


def _linear_fwd_fenced(a0, w0, a1, w1, bias, relu):
    m, n, k0, k1 = a0.shape[0], w0.shape[0], a0.shape[1], 0 if a1 is None else a1.shape[1]
    f = _fences([a0, w0, a1, w1, bias])
    out = fenced_empty((m, n), DEV)
    check(glib.load().gts_linear_fwd_f32(*[ptr(v) for v, _ in f], ptr(out[0]), m, n, k0, k1, int(relu), None, None,
                                         current_stream()), "gts_linear_fwd_f32")
    _assert_fences({"a0": f[0], "w0": f[1], "a1": f[2], "w1": f[3], "bias": f[4], "out": out})
    return out[0]


FWD_SHAPES = [("auto", 37, 4, 8, ()), ("auto", 33, 20, 20, ()), ("auto", 7, 256, 20, ()), ("auto", 257, 64, 256, ()),
              ("tile1", 257, 64, 256, ((1, 1),)), ("tile3", 257, 64, 256, ((1, 3),)), ("tile5", 257, 64, 256, ((1, 5),)),
              ("tile8", 257, 64, 256, ((1, 8),)),
              ("panel10", 241, 32, 260, ((1, 10),)), ("panel10", 5, 36, 4, ((1, 10),)),
              ("rows240", 241, 64, 256, ((13, 240), (1, 10))), ("rows192", 241, 64, 256, ((13, 192), (1, 10))),
              ("rows144", 241, 64, 256, ((13, 144), (1, 10)))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,m,k,n,options", FWD_SHAPES, ids=lambda v: v if isinstance(v, (str, int)) else "")
def test_linear_forward_classes_and_fences(name, m, k, n, options, kind):
    """dense.linear_fwd with bias + ReLU at the smallest ragged shapes: the automatic choice, every 32x32x2 tile forced,
    the panel variant and each panel height.  The wrapper's result and the one computed between fences are both held
    to the fp64 classes."""
    a, w, b = _inject(kind, _rand(m, k, seed=1), _rand(n, k, seed=2), _rand(n, seed=3), seed=m + k + n)
    pre, bound = _ref_product(a, w, b)
    want = torch.relu(pre)
    assert not torch.isfinite(pre).all()                      # the injection reached the reference
    with _options(options):
        got = dense.linear_fwd(a.to(DEV), w.to(DEV), bias=b.to(DEV), relu=True)
        got_fenced = _linear_fwd_fenced(a, w, None, None, b, True)
    classes_match(got, want, bound)
    classes_match(got_fenced, want, bound)


@pytest.mark.parametrize("name,m,k,n,options", FWD_SHAPES, ids=lambda v: v if isinstance(v, (str, int)) else "")
def test_linear_forward_signed_zero_under_relu(name, m, k, n, options):
    """A pre-activation whose every product is exactly -0.0, no bias: the sign bit of the result is torch's, with and
    without the ReLU (relu(-0.0) = -0.0 in torch, so the epilogue must not be what decides it)."""
    a = torch.ones(m, k)
    w = torch.full((n, k), -0.0)
    w[_positions(n, 5)[-1]] = 0.5                             # one ordinary column beside the zeros
    pre = a.double() @ w.double().t()
    with _options(options):
        for relu in (False, True):
            want = torch.relu(pre) if relu else pre
            got = dense.linear_fwd(a.to(DEV), w.to(DEV), relu=relu).cpu()
            assert torch.equal(got.double(), want)
            assert torch.equal(torch.signbit(got), torch.signbit(want))


@pytest.mark.parametrize("kind", KINDS)
def test_dual_segment_forward_classes_and_fences(kind):
    """(250, 300, 132) with a second reduction segment of k + 4: the poison goes into the second segment for every other
    kind, so both segments' loads are covered."""
    m, k, n = 250, 300, 132
    ops_ = [_rand(m, k, seed=1), _rand(n, k, seed=2), _rand(m, k + 4, seed=3), _rand(n, k + 4, seed=4)]
    b = _rand(n, seed=5)
    seg = KINDS.index(kind) % 2
    ops_[2 * seg], ops_[2 * seg + 1], b = _inject(kind, ops_[2 * seg], ops_[2 * seg + 1], b, seed=m + k + n)
    (p0, b0), (p1, b1) = _ref_product(ops_[0], ops_[1], b), _ref_product(ops_[2], ops_[3])
    want, bound = torch.relu(p0 + p1), b0 + b1
    assert not torch.isfinite(p0 + p1).all()
    got = dense.linear_fwd(*[t.to(DEV) for t in ops_], bias=b.to(DEV), relu=True)
    classes_match(got, want, bound)
    classes_match(_linear_fwd_fenced(*ops_, b, True), want, bound)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("options", [(), ((1, 10),)], ids=["auto", "panel10"])
def test_chained_forward_classes_and_fences(options, kind):
    """dense.linear_fwd_chain at (241, 64, 256, 256), as the library chooses and with the panel variant forced (the pair
    in one launch): the second product is held to fp64 on the GPU's own first output
    (both sides see the same operand, as in test_gpu_gemm.py), NaN in w2 / bias2 for the weight and bias kinds."""
    m, k, n, n2 = 241, 64, 256, 256
    a, w, b = _inject(kind, _rand(m, k, seed=41), _rand(n, k, seed=42), _rand(n, seed=43), seed=m + k + n)
    w2, b2 = _rand(n2, n, seed=44), _rand(n2, seed=45)
    if kind in ("nan_w", "combined"):
        w2[_positions(n2, 3)[1], _positions(n, 4)[1]] = NAN
    if kind in ("nan_bias", "combined"):
        b2[_positions(n2, 5)[0]] = NAN
    pre, bound = _ref_product(a, w, b)
    f = _fences([a, w, b, w2, b2])
    out, out2 = fenced_empty((m, n), DEV), fenced_empty((m, n2), DEV)
    dev = [t.to(DEV) for t in (a, w, b, w2, b2)]
    with _options(options):
        check(glib.load().gts_linear_fwd_chain_f32(ptr(f[0][0]), ptr(f[1][0]), None, None, ptr(f[2][0]), ptr(out[0]),
                                                   ptr(f[3][0]), ptr(f[4][0]), ptr(out2[0]), m, n, k, 0, 1, n2, 1, None,
                                                   None, current_stream()), "gts_linear_fwd_chain_f32")
        got, got2 = dense.linear_fwd_chain(dev[0], dev[1], None, None, dev[2], True, dev[3], dev[4], True)
        plain = dense.linear_fwd(dev[0], dev[1], bias=dev[2], relu=True)
        plain2 = dense.linear_fwd(plain, dev[3], bias=dev[4], relu=True)
    _assert_fences({"a": f[0], "w": f[1], "bias": f[2], "w2": f[3], "bias2": f[4], "out": out, "out2": out2})
    classes_match(out[0], torch.relu(pre), bound)
    pre2, bound2 = _ref_product(out[0].cpu(), w2, b2)
    classes_match(out2[0], torch.relu(pre2), bound2)
    assert _same_bits(got, out[0]) and _same_bits(got2, out2[0])
    assert _same_bits(plain, got) and _same_bits(plain2, got2)       # the chain still equals two calls, NaN for NaN


WGRAD_KINDS = ["nan_g", "nan_act", "inf_times_zero", "inf_minus_inf", "combined"]


@pytest.mark.parametrize("kind", WGRAD_KINDS)
@pytest.mark.parametrize("variant", [1, 2, 4, 6])
def test_weight_gradient_classes_and_fences(variant, kind):
    """gts_linear_bwd_weight_f32 at (257, 256, 256) on each tile (GTS_OPT_WGRAD_TILE): gw = g^T act and the column sums
    of g, poison in g and in act, everything between fences (the workspace included)."""
    m, n, k = 257, 256, 256
    g, act = _rand(m, n, seed=51), _rand(m, k, seed=53)
    rows, gc, ac = _positions(m, 1), _positions(n, 2), _positions(k, 3)
    if kind in ("nan_g", "combined"):
        for r, c in zip(rows, gc):
            g[r, c] = NAN
    if kind in ("nan_act", "combined"):
        for r, c in zip(rows, reversed(ac)):
            act[r, c] = NAN
    if kind in ("inf_times_zero", "combined"):
        g[rows[-1], gc[0]] = INF
        act[rows[-1], ac] = 0.0
    if kind == "inf_minus_inf":
        act = act.abs()
        g[rows[0], gc[1]], g[rows[-1], gc[1]] = INF, -INF
    want_w, bound_w = _ref_product(g.t(), act.t())
    want_b, bound_b = g.double().sum(0), zero_nonfinite(g).sum(0)
    assert not torch.isfinite(want_w).all()
    lib = glib.load()
    f = _fences([g, act])
    gw, gb = fenced_empty((n, k), DEV), fenced_empty((n,), DEV)
    nbytes = lib.gts_linear_bwd_weight_workspace(m, n, k, 1)
    ws = fenced_empty(((nbytes + 3) // 4,), DEV)
    arr = ctypes.c_void_p * 1
    with _options(((2, variant),)):
        check(lib.gts_linear_bwd_weight_f32(arr(ptr(f[0][0])), arr(ptr(f[1][0])), arr(ptr(gw[0])), arr(ptr(gb[0])), 1,
                                            ptr(ws[0]), ws[0].numel() * 4, m, n, k, current_stream()),
              "gts_linear_bwd_weight_f32")
        got_w, got_b = dense.linear_bwd_weight(g.to(DEV), act.to(DEV), want_bias_grad=True)
    _assert_fences({"g": f[0], "act": f[1], "gw": gw, "gb": gb, "workspace": ws})
    classes_match(gw[0], want_w, bound_w)
    classes_match(gb[0], want_b, bound_b)
    classes_match(got_w, want_w, bound_w)
    classes_match(got_b, want_b, bound_b)


IGRAD_KINDS = ["nan_a", "nan_w", "inf_times_zero", "inf_minus_inf", "pos_inf_relu", "combined"]


@pytest.mark.parametrize("kind", IGRAD_KINDS)
@pytest.mark.parametrize("m,k,n,options", [(37, 4, 8, ()), (257, 256, 64, ()), (257, 256, 64, ((3, 8),)),
                                           (241, 260, 32, ((1, 10),))], ids=lambda v: v if isinstance(v, int) else "")
def test_input_gradients_classes_and_fences(m, k, n, options, kind):
    """gin [m, k] = g [m, n] @ w [n, k], zeroed where a FINITE relu_mask is not positive (a select, as torch's
    threshold_backward: a NaN product under a closed mask is 0), through gts_linear_bwd_input_f32 (weights as stored) and
    gts_linear_bwd_input_t_f32 (transposed weights): non-finite g, non-finite weight."""
    g, wt, _ = _inject(kind, _rand(m, n, seed=1), _rand(k, n, seed=2), None, seed=m + k + n)      # wt [k, n] = w^T
    mask = _rand(m, k, seed=6)
    mask[_positions(m, 2)[0], _positions(k, 3)[0]] = 0.0        # an explicit zero: closed
    prod, bound = _ref_product(g, wt)
    assert not torch.isfinite(prod).all()
    want = torch.where(mask.double() > 0, prod, torch.zeros_like(prod))
    w = wt.t().contiguous()
    lib = glib.load()
    f = _fences([g, w, wt, mask])
    gin, gin_t = fenced_empty((m, k), DEV), fenced_empty((m, k), DEV)
    with _options(options):
        check(lib.gts_linear_bwd_input_f32(ptr(f[0][0]), ptr(f[1][0]), None, None, ptr(f[3][0]), ptr(gin[0]), m, k, n, 0,
                                           current_stream()), "gts_linear_bwd_input_f32")
        check(lib.gts_linear_bwd_input_t_f32(ptr(f[0][0]), ptr(f[2][0]), None, None, ptr(f[3][0]), None, ptr(gin_t[0]), m, k,
                                             n, 0, None, current_stream()), "gts_linear_bwd_input_t_f32")
        got = dense.linear_bwd_input(g.to(DEV), w.to(DEV), relu_mask=mask.to(DEV))
        got_t = dense.linear_bwd_input_t(g.to(DEV), wt.to(DEV), relu_mask=mask.to(DEV))
        open_t = dense.linear_bwd_input_t(g.to(DEV), wt.to(DEV))
    _assert_fences({"g": f[0], "w": f[1], "wt": f[2], "mask": f[3], "gin": gin, "gin_t": gin_t})
    for out in (gin[0], gin_t[0], got, got_t):
        classes_match(out, want, bound)
    classes_match(open_t, prod, bound)


# ---------------------------------------------------------------------------------------------- conv3d C1-C5
CONV_DIMS = [(1, 1, 1), (2, 3, 18), (7, 9, 11)]
CONV_CHANNELS = [(3, 7, 2), (9, 16, 5)]


def _conv_operands(dims, cin, cmid, cout):
    g = torch.Generator().manual_seed(sum(dims) * 100 + cin + cmid + cout)
    x = torch.randn(*dims, cin, generator=g)
    w1 = torch.randn(cmid, cin, 5, 5, 5, generator=g) * 0.1
    b1 = torch.randn(cmid, generator=g)
    w2 = torch.randn(cout, cmid, 5, 5, 5, generator=g) * 0.1
    dy = torch.randn(dims[0] * dims[1] * dims[2], cout, generator=g)
    h = torch.randn(dims[0] * dims[1] * dims[2], cmid, generator=g)
    return x, w1, b1, w2, dy, h


def _voxels(dims):
    """An interior voxel and the last-z / last-x / last-y boundary voxels: at (2, 3, 18) and (7, 9, 11) each of the
    three lies in a partly filled 4 x 4 x 16 brick."""
    cx, cy, cz = dims
    return {"interior": (cx // 2, cy // 2, cz // 2), "last_z": (cx // 2, cy // 2, cz - 1),
            "last_x": (cx - 1, cy // 2, cz // 2), "last_y": (cx // 2, cy - 1, cz // 2), "corner": (cx - 1, cy - 1, cz - 1)}


def _conv_fwd_fenced(x, w, b, relu):
    cx, cy, cz, cin = x.shape
    cout = w.shape[0]
    lib = glib.load()
    f = _fences([x, w, b])
    y = fenced_empty((cx * cy * cz, cout), DEV)
    ws = fenced_empty((max(1, lib.gts_conv3d_fwd_workspace(cin, cout) // 4),), DEV)
    check(lib.gts_conv3d_fwd_f32(ptr(f[0][0]), ptr(f[1][0]), ptr(f[2][0]), ptr(y[0]), cx, cy, cz, cin, cout, int(relu),
                                 ptr(ws[0]), ws[0].numel() * 4, current_stream()), "gts_conv3d_fwd_f32")
    _assert_fences({"x": f[0], "w": f[1], "b": f[2], "y": y, "workspace": ws})
    return y[0]


CONV_FWD_KINDS = ["nan_x", "inf_x", "nan_w1", "nan_b1"]


@pytest.mark.parametrize("kind", CONV_FWD_KINDS)
@pytest.mark.parametrize("channels", CONV_CHANNELS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("dims", CONV_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_conv3d_forward_classes_and_fences(dims, channels, kind):
    """C1 with and without the ReLU: NaN / +Inf in x at an interior voxel and at each boundary voxel (the clamp replicates
    a boundary voxel into every halo position past it), NaN in w1 and in b1."""
    cin, cmid, cout = channels
    x, w1, b1, _, _, _ = _conv_operands(dims, cin, cmid, cout)
    cases = []
    if kind in ("nan_x", "inf_x"):
        for where, (vx, vy, vz) in _voxels(dims).items():
            xi = x.clone()
            xi[vx, vy, vz, (vx + vy + vz) % cin] = NAN if kind == "nan_x" else INF
            cases.append((where, xi, w1, b1))
    elif kind == "nan_w1":
        wi = w1.clone()
        wi[cmid - 1, cin - 1, 4, 0, 2], wi[0, 0, 0, 0, 0] = NAN, NAN
        cases.append(("w1", x, wi, b1))
    else:
        bi = b1.clone()
        bi[cmid // 2] = NAN
        cases.append(("b1", x, w1, bi))
    for where, xi, wi, bi in cases:
        pre = conv3d_ref.conv(xi.double(), wi.double(), bi.double())
        bound = conv3d_ref.conv(zero_nonfinite(xi), zero_nonfinite(wi), zero_nonfinite(bi))
        assert not torch.isfinite(pre).all(), where
        for relu in (False, True):
            want = torch.relu(pre) if relu else pre
            classes_match(conv3d.conv3d_fwd(xi.to(DEV), wi.to(DEV), bi.to(DEV), relu=relu), want, bound)
            classes_match(_conv_fwd_fenced(xi, wi, bi, relu), want, bound)


@pytest.mark.parametrize("channels", CONV_CHANNELS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("dims", CONV_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_conv3d_data_gradient_classes_and_fences(dims, channels):
    """C3 with a finite mask h: a NaN in dy reaches exactly the input voxels the replicate adjoint sends it to, and is 0
    where the mask is closed."""
    cin, cmid, cout = channels
    _, _, _, w2, dy, h = _conv_operands(dims, cin, cmid, cout)
    cx, cy, cz = dims
    h[0, 0] = 0.0
    lib = glib.load()
    for where, (vx, vy, vz) in _voxels(dims).items():
        dyi = dy.clone()
        dyi[(vx * cy + vy) * cz + vz, (vx + vy + vz) % cout] = NAN
        full = conv3d_ref.data_grad(dyi.double(), w2.double(), dims)
        bound = conv3d_ref.data_grad(zero_nonfinite(dyi), w2.double().abs(), dims)
        assert torch.isnan(full).any(), where
        want = torch.where(h.double() > 0, full, torch.zeros_like(full))
        classes_match(conv3d.conv3d_bwd_data(dyi.to(DEV), w2.to(DEV), dims), full, bound)
        classes_match(conv3d.conv3d_bwd_data(dyi.to(DEV), w2.to(DEV), dims, h=h.to(DEV)), want, bound)
        f = _fences([dyi, w2, h])
        dx = fenced_empty((cx * cy * cz, cmid), DEV)
        ws = fenced_empty((max(1, lib.gts_conv3d_bwd_data_workspace(cx, cy, cz, cmid, cout) // 4),), DEV)
        check(lib.gts_conv3d_bwd_data_f32(ptr(f[0][0]), ptr(f[1][0]), ptr(f[2][0]), ptr(dx[0]), cx, cy, cz, cmid, cout,
                                          ptr(ws[0]), ws[0].numel() * 4, current_stream()), "gts_conv3d_bwd_data_f32")
        _assert_fences({"dy": f[0], "w": f[1], "h": f[2], "dx": dx, "workspace": ws})
        classes_match(dx[0], want, bound)


def _conv_wgrad_check(x, dy, cout, where):
    cx, cy, cz, cin = x.shape
    want_w, want_b = conv3d_ref.weight_grad(x.double(), dy.double(), cout)
    bound_w, bound_b = conv3d_ref.weight_grad(zero_nonfinite(x), zero_nonfinite(dy), cout)
    lib = glib.load()
    f = _fences([x, dy])
    dw, db = fenced_empty((cout, cin, 5, 5, 5), DEV), fenced_empty((cout,), DEV)
    ws = fenced_empty((max(1, lib.gts_conv3d_bwd_weight_workspace(cx, cy, cz, cin, cout) // 4),), DEV)
    check(lib.gts_conv3d_bwd_weight_f32(ptr(f[0][0]), ptr(f[1][0]), ptr(dw[0]), ptr(db[0]), cx, cy, cz, cin, cout,
                                        ptr(ws[0]), ws[0].numel() * 4, current_stream()), "gts_conv3d_bwd_weight_f32")
    _assert_fences({"x": f[0], "dy": f[1], "dw": dw, "db": db, "workspace": ws})
    got_w, got_b = conv3d.conv3d_bwd_weight(x.to(DEV), dy.to(DEV), cout)
    for name, got, want, bound in (("dw fenced", dw[0], want_w, bound_w), ("db fenced", db[0], want_b, bound_b),
                                   ("dw", got_w, want_w, bound_w), ("db", got_b, want_b, bound_b)):
        try:
            classes_match(got, want, bound)
        except AssertionError as e:
            raise AssertionError(f"{where}, {name}: {e}") from None
    return want_w


@pytest.mark.parametrize("kind", ["nan_x", "inf_x", "nan_dy"])
@pytest.mark.parametrize("channels", CONV_CHANNELS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("dims", CONV_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_conv3d_weight_gradient_classes_tap_by_tap(dims, channels, kind):
    """C4 / C5: dw [Cout, Cin, 5, 5, 5] and db against fp64, tap by tap.  A non-finite x at a boundary voxel of a partly
    filled brick reaches a tap only through the voxels INSIDE the volume whose clamped neighbour it is: the brick's
    voxels past the volume carry dy = 0 and must not multiply the clamped halo (0 * Inf = NaN)."""
    cin, cmid, cout = channels
    x, _, _, _, _, _ = _conv_operands(dims, cin, cmid, cout)
    cx, cy, cz = dims
    dz = _rand(cx * cy * cz, cmid, seed=9)                   # gradient of the first layer's output
    for where, (vx, vy, vz) in _voxels(dims).items():
        xi, dzi = x.clone(), dz.clone()
        if kind == "nan_dy":
            dzi[(vx * cy + vy) * cz + vz, (vx + vy + vz) % cmid] = NAN
        else:
            xi[vx, vy, vz, (vx + vy + vz) % cin] = NAN if kind == "nan_x" else INF
        _conv_wgrad_check(xi, dzi, cmid, where)


def test_conv3d_weight_gradient_inf_at_the_last_voxel_of_2x3x18():
    """+Inf at voxel (1, 2, 17) of channel 0 of a 2 x 3 x 18 volume (the second z brick holds z = 16, 17 only).  The
    voxel is the last one along every axis, so tap t reaches it from a voxel inside the volume only when t >= 2 on each
    axis (the voxel itself or one whose clamped neighbour it is): 27 taps of that input channel are non-finite in the
    fp64 reference, 98 stay finite for every output channel — among them all 75 with dz in {0, 1}, which the brick's
    voxels z = 18 .. 31 past the volume would poison if they multiplied the clamped halo."""
    dims, (cin, cmid, cout) = (2, 3, 18), CONV_CHANNELS[0]
    x, _, _, _, _, _ = _conv_operands(dims, cin, cmid, cout)
    x[1, 2, 17, 0] = INF
    dz = _rand(2 * 3 * 18, cmid, seed=9)
    want_w = _conv_wgrad_check(x, dz, cmid, "(1, 2, 17)")
    finite = torch.isfinite(want_w[:, 0])                    # [cmid, 5, 5, 5] = [co, dx, dy, dz]
    assert finite[:, :, :, :2].all() and not finite[:, 2:, 2:, 2:].any()
    assert all(int(finite[co].sum()) == 98 for co in range(cmid)) and torch.isfinite(want_w[:, 1:]).all()


# ---------------------------------------------------------------------------------------------- losses
def _poison_logits(n, c, kind):
    x = _rand(n, c, seed=n + c)
    rows = _positions(n, n)
    if kind in ("nan", "both"):
        x[rows[0], c - 1] = NAN
    if kind in ("inf", "both"):
        x[rows[-1], 1] = INF
    y = torch.randint(0, c, (n,), generator=torch.Generator().manual_seed(n))
    w = torch.linspace(0.5, 2.0, c)
    return x, y, w


@pytest.mark.parametrize("kind", ["nan", "inf", "both"])
@pytest.mark.parametrize("c", [4, 5])
@pytest.mark.parametrize("n", [1, 65, 1025])
def test_weighted_cross_entropy_classes(n, c, kind):
    """ops.weighted_cross_entropy against F.cross_entropy in fp64 with autograd: the class of the loss and of every
    gradient element (the reference decides which rows are poisoned).  Finite gradient elements: a softmax in fp32 is
    good to a few ulp of its largest term, so |err| <= 1e-5 max_c w_c / sum_i w[y_i]."""
    x, y, w = _poison_logits(n, c, kind)
    x64 = x.double().requires_grad_(True)
    loss64 = F.cross_entropy(x64, y, weight=w.double())
    loss64.backward()
    xd = x.to(DEV).requires_grad_(True)
    loss = ops.weighted_cross_entropy(xd, y.to(DEV), w.to(DEV))
    loss.backward()
    scale = float(w.max() / w[y].sum())
    classes_match(loss.reshape(1), loss64.detach().reshape(1), torch.full((1,), 20.0, dtype=torch.float64), rel=1e-5)
    classes_match(xd.grad, x64.grad, torch.full_like(x64, scale), rel=1e-5)


@pytest.mark.parametrize("kind", ["nan", "inf", "both"])
@pytest.mark.parametrize("c", [4, 5])
@pytest.mark.parametrize("n", [1, 65, 1025])
def test_dice_ce_loss_classes(n, c, kind):
    """ops.dice_ce_loss against tests/dice_ref.py (fp64 autograd).  The Dice term couples every row through the region
    sums, so one poisoned row poisons the gradient of all of them: the reference says where.  Finite gradient elements
    within 1e-5 of S_bound, the largest possible |dL/dp| (dice_ref)."""
    x, y, w = _poison_logits(n, c, kind)
    regions = "brats" if c == 4 else "classes"
    ref = dice_ce_ref(x, y, w, regions=regions)
    xd = x.to(DEV).requires_grad_(True)
    loss = ops.dice_ce_loss(xd, y.to(DEV), w.to(DEV), regions=regions)
    loss.backward()
    classes_match(loss.reshape(1), ref.loss.reshape(1), torch.full((1,), 20.0, dtype=torch.float64), rel=1e-5)
    s_bound = ref.s_bound if ref.s_bound == ref.s_bound else 1.0
    classes_match(xd.grad, ref.grad, torch.full_like(ref.grad, s_bound), rel=1e-5)


# ---------------------------------------------------------------------------------------------- whole networks
HP = namedtuple("HP", "in_feats out_classes layer_sizes gat_heads gat_residuals")
CLASS_W = torch.tensor([0.1, 1.0, 2.0, 2.0])


def _network_case(model_type, hp, kind):
    from model.networks import init_graph_net
    from oracle import graph_ref, torch_ref
    from tests.helpers import copy_state

    graph = synth.lattice_graph((6, 6, 6))
    torch.manual_seed(11)
    ref = torch_ref.ref_init_graph_net(model_type, hp)
    net = init_graph_net(model_type, hp)
    copy_state(net, ref)
    ref = ref.double()
    x = torch.from_numpy(synth.node_features(graph.n, hp.in_feats, 5)).float()
    y = torch.from_numpy(synth.node_labels(graph.n, 5))
    node = _positions(graph.n, 3)[1]
    x[node, hp.in_feats - 1] = NAN if kind == "nan" else INF
    tg = torch_ref.TGraph(graph_ref.RefGraph(graph.src, graph.dst, graph.n))
    with torch.no_grad():
        want = ref(tg, x.double())
        loss64 = F.cross_entropy(want, y, weight=CLASS_W.double())
    return net.to(DEV), graph.to(DEV), x.to(DEV), y.to(DEV), want, loss64


def _run_network(net, graph, x, y, one_call):
    old = gnn.STACK_IN_ONE_CALL
    gnn.STACK_IN_ONE_CALL = one_call
    try:
        logits = net(graph, x)
        loss = ops.weighted_cross_entropy(logits, y, CLASS_W.to(DEV))
        return logits.detach(), loss.detach()
    finally:
        gnn.STACK_IN_ONE_CALL = old


@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("model_type,hp", [("GSpool", HP(20, 4, [64, 32], None, None)),
                                           ("GSpool", HP(4, 4, [256] * 3, None, None)),
                                           ("GAT", HP(4, 4, [64] * 3, [4, 4, 4], [False, True, False]))],
                         ids=["pool-20-64-32", "pool-4-256x3", "gat-64x3"])
def test_whole_network_carries_a_poisoned_feature_to_the_loss(model_type, hp, kind):
    """One NaN (or +Inf) node feature on the 6 x 6 x 6 lattice: the logits have the classes of the fp64 oracle (finite
    ones within the network tolerance of test_gpu_model.py, 1e-4 of the logit scale), the loss is NaN exactly when the
    oracle's is, and the stack in one call still equals the stack launch by launch bit for bit."""
    net, graph, x, y, want, loss64 = _network_case(model_type, hp, kind)
    finite = want[torch.isfinite(want)]
    scale = max(1.0, float(finite.abs().max())) if finite.numel() else 1.0
    assert not torch.isfinite(want).all()
    runs = [_run_network(net, graph, x, y, one_call) for one_call in (True, False)]
    for logits, loss in runs:
        classes_match(logits, want, torch.full_like(want, scale), rel=1e-4)
        assert bool(torch.isnan(loss)) == bool(torch.isnan(loss64)), f"loss {float(loss)} vs oracle {float(loss64)}"
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])


def test_refinement_logits_carry_a_nan_voxel_to_the_loss():
    """conv3d.refinement_logits of CnnRefinementNet(8, 4, [16]) on (7, 9, 11) with a NaN at the corner voxel: it reaches
    the 3^3 then 5^3 voxels nearest the corner and no others.  Finite logits: each layer is good to 2e-6 of its magnitude
    bound and the first layer's error passes through |w2|, so 4e-6 of the two-layer bound."""
    from model.networks import CnnRefinementNet

    dims = (7, 9, 11)
    torch.manual_seed(0)
    net = CnnRefinementNet(8, 4, [16])
    x = _rand(*dims, 8, seed=2)
    x[0, 0, 0, 3] = NAN
    y = torch.randint(0, 4, (7 * 9 * 11,), generator=torch.Generator().manual_seed(1))
    c1, c2 = net.conv_layers[0], net.conv_layers[1]
    w1, b1, w2, b2 = (p.detach().double() for p in (c1.weight, c1.bias, c2.weight, c2.bias))
    h1 = torch.relu(conv3d_ref.conv(x.double(), w1, b1)).reshape(*dims, -1)
    want = conv3d_ref.conv(h1, w2, b2)
    bound = conv3d_ref.conv(conv3d_ref.conv(zero_nonfinite(x), w1.abs(), b1.abs()).reshape(*dims, -1), w2.abs(), b2.abs())
    nan_rows = torch.isnan(want).any(1).reshape(dims)
    assert nan_rows[:5, :5, :5].all() and int(nan_rows.sum()) == 125
    loss64 = F.cross_entropy(want, y, weight=CLASS_W.double())
    net.to(DEV)
    logits = conv3d.refinement_logits(x.to(DEV), net)
    loss = ops.weighted_cross_entropy(logits, y.to(DEV), CLASS_W.to(DEV))
    classes_match(logits, want, bound, rel=4e-6)
    assert bool(torch.isnan(loss)) == bool(torch.isnan(loss64)) and bool(torch.isnan(loss64))
