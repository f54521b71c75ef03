"""The column reducers (csrc/gts_gat_reduce.hip) and the flat AdamW kernel (csrc/gts_optim.hip) at their edges, on a real
MI355X, against the host references of tests/reducers_ref.py (validated on the CPU in tests/test_reducers_ref_host.py).

Bars, none of them measured:
  * g_pre is elementwise with one rounding per operation and no contraction: bit-exact.
  * the column sums are added in a documented fixed order: bit-exact against the fp32 restatement of that order, and,
    independently, within  depth * 2^-24 * sum|term|  of the float64 sum of the same fp32 terms, depth = rows per chunk
    + ceil(chunks / 16) + 16 being the longest chain of additions (one more 2^-24 for gat_param_grad, whose terms are
    rounded products);
  * small-integer inputs have exact fp32 sums: the result IS the integer sum, whatever the order;
  * AdamW: see `test_adamw_one_step_against_float64`.
"""
import numpy as np
import pytest
import torch

import gts
from gts import ops
from gts.optim import FlatAdamW
from tests import reducers_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS = [1, 2, 15, 16, 17, 511, 512, 513, 1023, 1025, 8191, 8193, 49999, 60000]
COLS = [4, 8, 60, 256, 1024, 1028, 2052]
HEADS_DIM = [(1, 4), (4, 8), (3, 20), (5, 12), (4, 256), (2, 320), (4, 260), (5, 256)]
TINY = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module", autouse=True)
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _cols_for(n):
    """Every n meets widths on both sides of the 1024-column stride; the two full-size row counts take a subset (a
    [60000, 2052] operand is half a gigabyte) that together still covers every width but 2052, which 8193 rows cover."""
    if n == 49999:
        return [8, 256, 1028]
    if n == 60000:
        return [4, 60, 1024, 1028]
    return COLS


def _heads_dim_for(n):
    if n == 49999:
        return [(3, 20), (2, 320), (4, 260)]
    if n == 60000:
        return [(5, 12), (4, 256), (5, 256)]
    return HEADS_DIM


ACT_CASES = [(n, c) for n in NS for c in _cols_for(n)]
PARAM_CASES = [(n, h, d) for n in NS for h, d in _heads_dim_for(n)]


def test_the_case_lists_cover_what_they_claim():
    for n in NS:
        assert min(_cols_for(n)) <= 1024 < max(_cols_for(n))
        assert any(h * d > 1024 for h, d in _heads_dim_for(n)) and any(d & (d - 1) for h, d in _heads_dim_for(n))
    assert {c for _, c in ACT_CASES} == set(COLS)
    assert {(h, d) for _, h, d in PARAM_CASES} == set(HEADS_DIM)


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def _same_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ, first at flat index {bad[0]}"


def _gout_out(n, cols, seed, integers=False):
    """gout, out [n, cols] fp32.  The sign of `out` alternates with row + column, so that wherever n > 1 every column takes
    both branches of the activation; a ninth of the positive entries are the smallest positive normal and a third of the
    others are 0.0, -0.0 or -1.0 (the branch point from both sides, and where ELU' is exactly 0)."""
    rng = np.random.default_rng(seed)
    if integers:
        gout = rng.integers(-3, 4, size=(n, cols)).astype(np.float32)
        out = rng.integers(-3, 4, size=(n, cols)).astype(np.float32)
        return gout, out
    gout = rng.standard_normal((n, cols), dtype=np.float32)
    out = np.abs(rng.standard_normal((n, cols), dtype=np.float32)) + np.float32(0.01)
    down = (np.add.outer(np.arange(n), np.arange(cols)) & 1) == 1
    pick = rng.integers(0, 9, size=(n, cols))
    out[down] *= np.float32(-1.0)
    out[~down & (pick == 0)] = TINY
    for k, value in enumerate((0.0, -0.0, -1.0)):
        out[down & (pick == k)] = value
    assert np.array_equal(out > 0, ~down)
    return gout, out


def _check_colsum(got, terms, n, what, extra=0):
    """got (device, fp32) against the fp32 restatement (bits) and against the float64 sum of the same terms (bound)."""
    _same_bits(got.reshape(-1), R.chunked_colsum_f32(terms), what + " vs the fp32 restatement")
    want, mag = R.colsum_f64(terms)
    err = np.abs(got.detach().cpu().numpy().reshape(-1).astype(np.float64) - want)
    bar = (R.chain_depth(n) + extra) * R.U * mag
    assert np.all(err <= bar), f"{what} vs float64: worst error / bar = {np.max(err / np.maximum(bar, 1e-300)):.3f}"


# ---------------------------------------------------------------- gat_act_bwd
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("n,cols", ACT_CASES)
def test_gat_act_bwd_bits(n, cols, act):
    gout, out = _gout_out(n, cols, seed=n * 7 + cols + act)
    if n > 1 and act:
        assert np.all((out > 0).any(0) & (out <= 0).any(0))
    gout_d, out_d = torch.from_numpy(gout).to(DEV), torch.from_numpy(out).to(DEV)
    g_pre, g_bias = ops.gat_act_bwd(gout_d, out_d if act else None, act, True)
    terms = R.act_bwd_terms(gout, out, act)
    if act == 0:
        assert g_pre is gout_d                                  # the same storage, and untouched
    _same_bits(g_pre, terms, "g_pre")
    _same_bits(gout_d, gout, "gout after the call")
    _same_bits(out_d, out, "out after the call")
    _check_colsum(g_bias, terms, n, "g_bias")
    again_pre, again_bias = ops.gat_act_bwd(gout_d, out_d if act else None, act, True)
    _same_bits(again_pre, g_pre, "g_pre, second call")
    _same_bits(again_bias, g_bias, "g_bias, second call")
    only_pre, no_bias = ops.gat_act_bwd(gout_d, out_d if act else None, act, False)
    assert no_bias is None
    _same_bits(only_pre, terms, "g_pre without the bias gradient")


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("n", NS)
def test_gat_act_bwd_integer_sums_are_exact(n, act):
    """|g_pre| <= 3 * 4, so every partial sum is an integer below 2^24: a dropped or doubled row shows whatever the order."""
    for cols in (60, 1028):
        gout, out = _gout_out(n, cols, seed=n + cols, integers=True)
        _, g_bias = ops.gat_act_bwd(torch.from_numpy(gout).to(DEV), torch.from_numpy(out).to(DEV), act, True)
        want = R.act_bwd_terms(gout, out, act).astype(np.int64).sum(0)
        assert np.array_equal(g_bias.cpu().numpy().astype(np.int64), want)
        assert np.array_equal(g_bias.cpu().numpy(), want.astype(np.float32))


def test_gat_act_bwd_takes_3d_and_strided_operands():
    """[N, H, D] operands reduce over N; a strided gout or out gives the bits of its contiguous copy (the wrapper copies)."""
    gout, out = _gout_out(513, 24, seed=3)
    g3, o3 = torch.from_numpy(gout).to(DEV).view(513, 2, 12), torch.from_numpy(out).to(DEV).view(513, 2, 12)
    want_pre, want_bias = ops.gat_act_bwd(g3.reshape(513, 24), o3.reshape(513, 24), 1, True)
    g_pre, g_bias = ops.gat_act_bwd(g3, o3, 1, True)
    assert g_pre.shape == g3.shape
    _same_bits(g_pre.reshape(513, 24), want_pre, "g_pre of 3-D operands")
    _same_bits(g_bias, want_bias, "g_bias of 3-D operands")
    gt, ot = torch.from_numpy(gout.T.copy()).to(DEV).t(), torch.from_numpy(out.T.copy()).to(DEV).t()
    assert not gt.is_contiguous() and not ot.is_contiguous() and gt.shape == (513, 24)
    for a, b in ((gt, o3.reshape(513, 24)), (g3.reshape(513, 24), ot), (gt, ot)):
        g_pre, g_bias = ops.gat_act_bwd(a, b, 1, True)
        _same_bits(g_pre, want_pre, "g_pre of strided operands")
        _same_bits(g_bias, want_bias, "g_bias of strided operands")
    none_pre, none_bias = ops.gat_act_bwd(gt, None, 0, True)
    _same_bits(none_pre, gout, "a strided gout with no activation comes back as its copy")
    _same_bits(none_bias, R.chunked_colsum_f32(gout), "g_bias of a strided gout")


def _call_act_bwd(lib, gout, out, act, g_pre, g_bias, ws, ws_bytes, n, cols):
    return lib.gts_gat_act_bwd_f32(gout.data_ptr(), out.data_ptr(), act, g_pre.data_ptr(), g_bias.data_ptr(),
                                   ws.data_ptr(), ws_bytes, n, cols, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("n,cols", [(17, 8), (1025, 1028), (8193, 256)])
def test_gat_act_bwd_in_place_through_the_c_abi(lib, n, cols, act):
    """g_pre may be gout itself (the fused input-gradient GEMM relies on it): the bits of the out-of-place call."""
    gout, out = _gout_out(n, cols, seed=n + act)
    gout_d, out_d = torch.from_numpy(gout).to(DEV), torch.from_numpy(out).to(DEV)
    want_pre, want_bias = ops.gat_act_bwd(gout_d, out_d, act, True)
    buf = gout_d.clone()
    g_bias = torch.full((cols,), float("nan"), device=DEV)
    nbytes = lib.gts_gat_reduce_workspace(n, cols)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    assert _call_act_bwd(lib, buf, out_d, act, buf, g_bias, ws, nbytes, n, cols) == 0
    _same_bits(buf, want_pre, "g_pre written over gout")
    _same_bits(g_bias, want_bias, "g_bias of the in-place call")


# ---------------------------------------------------------------- gat_param_grad
def _param_operands(n, heads, dim, seed, integers=False):
    rng = np.random.default_rng(seed)
    if integers:
        return tuple(rng.integers(-3, 4, size=s).astype(np.float32) for s in ((n, heads, dim), (n, heads), (n, heads)))
    ft = rng.standard_normal((n, heads, dim), dtype=np.float32)
    gel = rng.standard_normal((n, heads), dtype=np.float32)
    ger = rng.standard_normal((n, heads), dtype=np.float32) * np.float32(10.0)
    return ft, gel, ger


@pytest.mark.parametrize("n,heads,dim", PARAM_CASES)
def test_gat_param_grad_bits(n, heads, dim):
    ft, gel, ger = _param_operands(n, heads, dim, seed=n + 31 * heads + dim)
    dev = [torch.from_numpy(a).to(DEV) for a in (ft, gel, ger)]
    gl, gr = ops.gat_param_grad(*dev)
    assert gl.shape == gr.shape == (heads, dim)
    _check_colsum(gl, R.param_grad_terms(ft, gel), n, "g_attn_l", extra=1)
    _check_colsum(gr, R.param_grad_terms(ft, ger), n, "g_attn_r", extra=1)
    for got, want in zip(dev, (ft, gel, ger)):
        _same_bits(got, want, "an operand after the call")
    gl2, gr2 = ops.gat_param_grad(*dev)
    _same_bits(gl2, gl, "g_attn_l, second call")
    _same_bits(gr2, gr, "g_attn_r, second call")


@pytest.mark.parametrize("n", NS)
def test_gat_param_grad_integer_sums_are_exact(n):
    """Products of integers up to 3 are at most 9: the sums are exact.  Each head's weights differ, so a column that read
    the wrong head's gel (a head boundary inside a workgroup's span: (3, 20), (5, 12)) is caught exactly."""
    for heads, dim in ((3, 20), (5, 12), (4, 260)):
        ft, gel, ger = _param_operands(n, heads, dim, seed=n + heads, integers=True)
        gl, gr = ops.gat_param_grad(*(torch.from_numpy(a).to(DEV) for a in (ft, gel, ger)))
        for got, w in ((gl, gel), (gr, ger)):
            want = np.einsum("nh,nhd->hd", w.astype(np.int64), ft.astype(np.int64))
            assert np.array_equal(got.cpu().numpy().astype(np.int64), want)


def test_gat_param_grad_strided_operands_give_the_bits_of_their_copies():
    ft, gel, ger = _param_operands(1025, 3, 20, seed=9)
    ft_d, gel_d, ger_d = (torch.from_numpy(a).to(DEV) for a in (ft, gel, ger))
    want_l, want_r = ops.gat_param_grad(ft_d, gel_d, ger_d)
    ft_s = torch.from_numpy(np.ascontiguousarray(ft.transpose(1, 0, 2))).to(DEV).transpose(0, 1)
    gel_s = torch.from_numpy(np.ascontiguousarray(gel.T)).to(DEV).t()
    ger_s = torch.stack([ger_d, ger_d], dim=2)[:, :, 0]
    for t, ref in ((ft_s, ft), (gel_s, gel), (ger_s, ger)):
        assert not t.is_contiguous() and t.shape == ref.shape
        _same_bits(t.contiguous(), ref, "the strided view holds the same values")
    for args in ((ft_s, gel_d, ger_d), (ft_d, gel_s, ger_d), (ft_d, gel_d, ger_s), (ft_s, gel_s, ger_s)):
        gl, gr = ops.gat_param_grad(*args)
        _same_bits(gl, want_l, "g_attn_l of strided operands")
        _same_bits(gr, want_r, "g_attn_r of strided operands")


# ---------------------------------------------------------------- the shared workspace
@pytest.mark.parametrize("n,cols", [(15, 8), (513, 60), (1025, 1028), (60000, 256)])
def test_a_dirty_workspace_does_not_leak_into_the_sums(lib, n, cols):
    """The wrappers take their scratch from torch.empty.  Freed blocks full of NaN make it likely that the scratch starts
    as NaN: the results stay the same bits, so the adder reads no partial sum that nobody wrote (fewer than 16 chunks leave
    adder lanes without one; the last chunk is short)."""
    gout, out = _gout_out(n, cols, seed=11)
    ft, gel, ger = _param_operands(n, cols // 4, 4, seed=12)
    gout_d, out_d = torch.from_numpy(gout).to(DEV), torch.from_numpy(out).to(DEV)
    dev = [torch.from_numpy(a).to(DEV) for a in (ft, gel, ger)]
    clean = ops.gat_act_bwd(gout_d, out_d, 1, True) + ops.gat_param_grad(*dev)
    torch.cuda.synchronize()
    floats = lib.gts_gat_reduce_workspace(n, cols) // 4
    for _ in range(2):
        junk = [torch.full((k,), float("nan"), device=DEV) for k in (floats, floats, cols, cols, gout_d.numel())]
        torch.cuda.synchronize()
        del junk
        dirty = ops.gat_act_bwd(gout_d, out_d, 1, True) + ops.gat_param_grad(*dev)
        for a, b in zip(dirty, clean):
            _same_bits(a, b, "a result computed in recycled NaN memory")
    # and through the C ABI, where the scratch is NaN for certain
    ws = torch.full((floats,), float("nan"), device=DEV)
    g_pre, g_bias = torch.empty_like(gout_d), torch.empty(cols, device=DEV)
    assert _call_act_bwd(lib, gout_d, out_d, 1, g_pre, g_bias, ws, floats * 4, n, cols) == 0
    _same_bits(g_bias, clean[1], "g_bias from NaN scratch")
    ws.fill_(float("nan"))
    gl, gr = torch.empty(cols, device=DEV), torch.empty(cols, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.gts_gat_param_grad_f32(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), gl.data_ptr(), gr.data_ptr(),
                                      ws.data_ptr(), floats * 4, n, cols // 4, 4, st) == 0
    _same_bits(gl, clean[2].reshape(-1), "g_attn_l from NaN scratch")
    _same_bits(gr, clean[3].reshape(-1), "g_attn_r from NaN scratch")


def test_reduce_workspace_size_and_refusal_of_a_short_one(lib):
    """gts_gat_reduce_workspace(n, cols) = 2 * chunks * cols * 4 bytes: two arrays of per-chunk sums, which
    gts_gat_param_grad_f32 needs both of and gts_gat_act_bwd_f32 one of (include/gts_hip.h).  One byte less than a
    call needs is refused before anything is launched: the outputs keep their fill."""
    for n in NS + [1024, 2 ** 31 + 5]:
        for cols in (4, 60, 1028):
            assert lib.gts_gat_reduce_workspace(n, cols) == 2 * R.chunk_geometry(n)[1] * cols * 4
    for n, cols in ((0, 8), (-1, 8), (-2 ** 40, 8), (5, 0), (5, -4), (5, 1), (5, 6), (5, 1027), (60000, 2050)):
        assert lib.gts_gat_reduce_workspace(n, cols) == 0
    n, cols = 1025, 60
    need = lib.gts_gat_reduce_workspace(n, cols)
    gout, out = _gout_out(n, cols, seed=1)
    gout_d, out_d = torch.from_numpy(gout).to(DEV), torch.from_numpy(out).to(DEV)
    ws = torch.zeros(need // 4, device=DEV)
    g_pre, g_bias = torch.full_like(gout_d, 7.0), torch.full((cols,), 7.0, device=DEV)
    assert _call_act_bwd(lib, gout_d, out_d, 1, g_pre, g_bias, ws, need // 2 - 1, n, cols) != 0
    ft, gel, ger = (torch.from_numpy(a).to(DEV) for a in _param_operands(n, 3, 20, seed=2))
    gl, gr = torch.full((cols,), 7.0, device=DEV), torch.full((cols,), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.gts_gat_param_grad_f32(ft.data_ptr(), gel.data_ptr(), ger.data_ptr(), gl.data_ptr(), gr.data_ptr(),
                                      ws.data_ptr(), need - 1, n, 3, 20, st) != 0
    torch.cuda.synchronize()
    for t in (g_pre, g_bias, gl, gr):
        assert bool((t == 7.0).all())
    assert not bool(ws.any())
    # exactly what each needs is enough, and gives the usual bits
    want_pre, want_bias = ops.gat_act_bwd(gout_d, out_d, 1, True)
    assert _call_act_bwd(lib, gout_d, out_d, 1, g_pre, g_bias, ws, need // 2, n, cols) == 0
    _same_bits(g_pre, want_pre, "g_pre with one array of scratch")
    _same_bits(g_bias, want_bias, "g_bias with one array of scratch")
    assert not bool(ws[need // 8:].any())                      # the second array was not touched
    assert lib.gts_gat_param_grad_f32(ft.data_ptr(), gel.data_ptr(), ger.data_ptr(), gl.data_ptr(), gr.data_ptr(),
                                      ws.data_ptr(), need, n, 3, 20, st) == 0
    want_l, want_r = ops.gat_param_grad(ft, gel, ger)
    _same_bits(gl, want_l.reshape(-1), "g_attn_l")
    _same_bits(gr, want_r.reshape(-1), "g_attn_r")


# ---------------------------------------------------------------- wrapper refusals
def test_the_reducer_wrappers_refuse_what_the_kernels_cannot_take():
    """A mismatch is a Python error, never a raw pointer handed to a kernel (the rule of
    test_shape_mismatches_raise_on_the_host_before_any_launch).  tests/test_reducers_ref_host.py shows that these are
    decided before the library is reached."""
    g, o = torch.randn(50, 8, device=DEV), torch.randn(50, 8, device=DEV)
    ft, ge = torch.randn(50, 2, 4, device=DEV), torch.randn(50, 2, device=DEV)
    refused = [
        lambda: ops.gat_act_bwd(g.double(), o, 1, True),
        lambda: ops.gat_act_bwd(g, o.double(), 2, True),
        lambda: ops.gat_act_bwd(g.cpu(), o, 1, True),
        lambda: ops.gat_act_bwd(g, o.cpu(), 1, True),
        lambda: ops.gat_act_bwd(g, o, 3, True),
        lambda: ops.gat_act_bwd(g, None, 1, True),
        lambda: ops.gat_act_bwd(g, o[:49], 1, True),
        lambda: ops.gat_act_bwd(g, torch.randn(8, 50, device=DEV), 1, True),
        lambda: ops.gat_act_bwd(g[:, :6], o[:, :6], 2, True),               # cols % 4 != 0
        lambda: ops.gat_act_bwd(g[:, :6], None, 0, False),
        lambda: ops.gat_act_bwd(g[:0], o[:0], 1, True),
        lambda: ops.gat_act_bwd(torch.zeros((), device=DEV), None, 0, True),
        lambda: ops.gat_param_grad(ft.cpu(), ge, ge),
        lambda: ops.gat_param_grad(ft, ge.cpu(), ge),
        lambda: ops.gat_param_grad(ft.double(), ge, ge),
        lambda: ops.gat_param_grad(ft, ge, ge.double()),
        lambda: ops.gat_param_grad(ft, ge[:, :1], ge),                       # gel of the wrong shape
        lambda: ops.gat_param_grad(ft, ge, ge[:49]),
        lambda: ops.gat_param_grad(ft.reshape(50, 8), ge, ge),
        lambda: ops.gat_param_grad(torch.randn(50, 2, 6, device=DEV), ge, ge),   # dim % 4 != 0
        lambda: ops.gat_param_grad(ft[:0], ge[:0], ge[:0]),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(gts.GtsError):
            call()
            pytest.fail(f"refusal {i} did not raise")


# ---------------------------------------------------------------- AdamW through the C ABI
ADAMW_NS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 1254403, 4194304 + 4099]
BIG = 4194304 + 4099          # a full stride of the 4096-block grid, a second trip, and a scalar tail behind it
GUARD = 64                    # floats on either side of a buffer (a multiple of 4: the buffer stays 16-byte aligned)
SENTINEL = -12345.5
EPS = 1e-8


class _Buffers:
    """p, g, m, v on the device, each inside its own guarded allocation; `shift` names the buffers that start one float
    past a 16-byte boundary."""

    def __init__(self, arrays, shift=()):
        self.n = arrays[0].size
        self.whole, self.view = [], []
        for name, a in zip("pgmv", arrays):
            off = GUARD + (1 if name in shift else 0)
            w = torch.full((self.n + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device=DEV)
            w[off:off + self.n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
            assert w.data_ptr() % 16 == 0
            self.whole.append(w)
            self.view.append(w[off:off + self.n])
            assert (self.view[-1].data_ptr() % 16 == 0) == (name not in shift) or self.n == 0

    def step(self, lib, lr, betas, eps, wd, step, n=None):
        p, g, m, v = self.view
        return lib.gts_adamw_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), self.n if n is None else n,
                                 lr, betas[0], betas[1], eps, wd, step, torch.cuda.current_stream().cuda_stream)

    def host(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.view]

    def assert_guards(self):
        for w, view in zip(self.whole, self.view):
            off = (view.data_ptr() - w.data_ptr()) // 4
            assert bool((w[:off] == SENTINEL).all()) and bool((w[off + self.n:] == SENTINEL).all()), "a guard word changed"


def _assert_within(got, ref, bar, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: worst error / bar = {worst:.3f}")
    assert np.all(err <= bar), f"{what}: worst error / bar = {worst:.3f} at {int(np.argmax(err - bar))}"


def _check_one_step(lib, n, lr, wd, betas, step, agree=True, shift=()):
    p, g, m, v = R.adamw_case(n, step, seed=n % 1000 + step, agree=agree)
    ref_p, ref_m, ref_v, delta = R.adamw_ref64(p, g, m, v, lr, betas, EPS, wd, step, with_delta=True)
    bar_p, bar_m, bar_v = R.adamw_bars(p, g, m, ref_v, delta)
    if not agree:
        bar_p = bar_p + R.adamw_cancellation_allowance(g, m, ref_v, lr, betas, EPS, step)
    buf = _Buffers((p, g, m, v), shift)
    assert buf.step(lib, lr, betas, EPS, wd, step) == 0
    got_p, got_g, got_m, got_v = buf.host()
    buf.assert_guards()
    _same_bits(got_g, g, "the gradient after the step")
    _assert_within(got_p, ref_p, bar_p, "param")
    _assert_within(got_m, ref_m, bar_m, "exp_avg")
    _assert_within(got_v, ref_v, bar_v, "exp_avg_sq")
    if n > 8:
        assert np.any(got_p != p) and np.any(got_v != v)
    return got_p, got_m, got_v


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("lr,wd", [(3e-3, 1e-2), (1e-4, 0.0)])
@pytest.mark.parametrize("n", ADAMW_NS)
def test_adamw_one_step_against_float64(lib, n, lr, wd, betas, step):
    """One update against `adamw_ref64` (float64 from the fp32 inputs; itself checked against torch.optim.AdamW in float64
    on the host).  Bars per element, u = 2^-24:
        |p - ref_p| <= 16 u (|p_old| + |delta|)      |m - ref_m| <= 4 u (|m_old| + |g|)      |v - ref_v| <= 4 u ref_v
    The update has at most eight fp32 roundings per element, the constants are rounded to fp32 once, and division and
    square root are correctly rounded; the factors are twice the raw rounding counts, the other half being the allowance
    for the float-rounded constants.
    The p bar presumes that the new first moment is accurate RELATIVE to itself.  beta1 * m + (1 - beta1) * g loses that
    when m and g have opposite signs and nearly cancel, so the state here has m agree in sign with g (it is a running mean
    of gradients); then |m_new| >= min(beta1, 1 - beta1)(|m| + |g|), the moment is good to 4u relative, and
    3u|p| + 15u|delta| bounds the whole update.  `test_adamw_with_cancelling_first_moment` covers the other case."""
    _check_one_step(lib, n, lr, wd, betas, step)


@pytest.mark.parametrize("step", [2, 1000])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("n", [1025, BIG])
def test_adamw_with_cancelling_first_moment(lib, n, betas, step):
    """Signs of m and g independent: the first moment's absolute error, up to 4u(|m_old| + |g|), reaches p through the
    step whatever |p_old| + |delta| is, so the p bar gains exactly that term (reducers_ref.adamw_cancellation_allowance).
    The m and v bars are the same."""
    _check_one_step(lib, n, 3e-3, 1e-2, betas, step, agree=False)


@pytest.mark.parametrize("quad", [(0.7310586, -1.5, 0.25, 0.0625), (-2.5e-3, 3.0e2, -4.0, 9.5e3), (1.0, 0.0, 0.0, 0.0)])
def test_adamw_is_position_independent(lib, quad):
    """One (p, g, m, v) everywhere: the vector body, the second trip of the grid stride and the scalar tail give one set of
    bits, which is also what a 1-element and an unaligned (all-scalar) launch give."""
    arrays = [np.full(BIG, x, np.float32) for x in quad]
    buf = _Buffers(arrays)
    assert buf.step(lib, 3e-3, (0.9, 0.999), EPS, 1e-2, 7) == 0
    got = buf.host()
    buf.assert_guards()
    one = _Buffers([a[:1] for a in arrays])
    assert one.step(lib, 3e-3, (0.9, 0.999), EPS, 1e-2, 7) == 0
    for name, arr, ref, old in zip("pgmv", got, one.host(), quad):
        b = _bits(arr)
        assert np.all(b == b[0]), f"{name}: {np.count_nonzero(b != b[0])} elements differ from element 0, " \
                                  f"first at {int(np.flatnonzero(b != b[0])[0])}"
        assert b[0] == _bits(ref)[0]
        if name == "g":
            assert arr[0] == np.float32(old)
    assert got[0][0] != np.float32(quad[0])


@pytest.mark.parametrize("shift", ["pgmv", "g", "p", "v"])
@pytest.mark.parametrize("n", [5, 1025, BIG])
def test_adamw_unaligned_buffers_give_the_aligned_bits(lib, n, shift):
    """A buffer that starts off a 16-byte boundary (all four, or one of them) sends the whole update down the scalar path:
    same bits, same untouched neighbours."""
    p, g, m, v = R.adamw_case(n, 3, seed=21)
    aligned = _Buffers((p, g, m, v))
    assert aligned.step(lib, 3e-3, (0.9, 0.999), EPS, 1e-2, 3) == 0
    shifted = _Buffers((p, g, m, v), shift)
    assert shifted.step(lib, 3e-3, (0.9, 0.999), EPS, 1e-2, 3) == 0
    for name, a, b in zip("pgmv", aligned.host(), shifted.host()):
        _same_bits(b, a, f"{name} with {shift} shifted by one float")
    aligned.assert_guards()
    shifted.assert_guards()
    ref_p, _, _ = R.adamw_ref64(p, g, m, v, 3e-3, (0.9, 0.999), EPS, 1e-2, 3)
    assert np.allclose(shifted.host()[0], ref_p, rtol=1e-5, atol=1e-6)      # and they are an update at all


def test_adamw_refusals_leave_the_buffers_alone(lib):
    arrays = R.adamw_case(1025, 2, seed=4)
    buf = _Buffers(arrays)
    for lr, betas, step in ((3e-3, (0.9, 0.999), 0), (3e-3, (0.9, 0.999), -3), (3e-3, (1.0, 0.999), 1),
                            (3e-3, (0.9, -0.1), 1), (3e-3, (0.9, 1.0), 1), (3e-3, (float("nan"), 0.999), 1)):
        assert buf.step(lib, lr, betas, EPS, 1e-2, step) != 0
    assert buf.step(lib, 3e-3, (0.9, 0.999), EPS, 1e-2, 1, n=-1) != 0
    assert buf.step(lib, 3e-3, (0.9, 0.999), EPS, 1e-2, 1, n=0) == 0           # nothing to do is not an error
    for got, want in zip(buf.host(), arrays):
        _same_bits(got, want, "a buffer after refused and empty calls")
    buf.assert_guards()


def test_flat_adamw_at_network_size_without_weight_decay():
    """FlatAdamW over 32 irregularly sized tensors, 1 254 403 parameters in all (the network's count), weight_decay = 0, three
    steps with the learning rate changed through param_groups between them, against `adamw_ref64` applied three times in
    float64.  Bar: the one-step bars summed over the three steps (each step adds at most its own rounding error to what it
    inherits; the gradients keep one sign per element, so no step's first moment cancels)."""
    rng = np.random.default_rng(17)
    total, pieces = 1254403, 32
    sizes = [int(s) | 1 for s in rng.integers(1000, 60000, size=pieces - 1)]      # no piece ends on a 16-byte boundary
    sizes.append(total - sum(sizes))
    assert len(sizes) == 32 and sum(sizes) == total and min(sizes) > 0
    p0 = rng.standard_normal(total, dtype=np.float32)
    sign = np.where(rng.random(total) < 0.5, -1.0, 1.0).astype(np.float32)
    cuts = np.cumsum([0] + sizes)
    params = [torch.nn.Parameter(torch.from_numpy(p0[a:b].copy()).to(DEV)) for a, b in zip(cuts[:-1], cuts[1:])]
    betas, lrs = (0.9, 0.999), (3e-3, 1e-3, 2e-4)
    opt = FlatAdamW(params, lr=lrs[0], betas=betas, eps=EPS, weight_decay=0.0)
    p, m, v = p0.astype(np.float64), np.zeros(total), np.zeros(total)
    bar_p, bar_m, bar_v = np.zeros(total), np.zeros(total), np.zeros(total)
    for step, lr in enumerate(lrs, start=1):
        g = sign * (np.abs(rng.standard_normal(total, dtype=np.float32)) * np.float32(step))
        g[step::9] = 0.0
        for q, a, b in zip(params, cuts[:-1], cuts[1:]):
            q.grad = torch.from_numpy(g[a:b].copy()).to(DEV)
        opt.param_groups[0]["lr"] = lr
        opt.step()
        p_old, m_old = p, m
        p, m, v, delta = R.adamw_ref64(p, g, m, v, lr, betas, EPS, 0.0, step, with_delta=True)
        for acc, one in zip((bar_p, bar_m, bar_v), R.adamw_bars(p_old, g, m_old, v, delta)):
            acc += one
    torch.cuda.synchronize()
    assert opt.steps == 3
    _assert_within(opt.flat_param.cpu().numpy(), p, bar_p, "flat_param after three steps")
    _assert_within(opt.exp_avg.cpu().numpy(), m, bar_m, "exp_avg after three steps")
    _assert_within(opt.exp_avg_sq.cpu().numpy(), v, bar_v, "exp_avg_sq after three steps")
    _same_bits(torch.cat([q.detach().reshape(-1) for q in params]), opt.flat_param, "the parameters are the flat buffer")
