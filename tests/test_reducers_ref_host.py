"""The host references of tests/test_gpu_reducers.py, validated on the CPU (tests/reducers_ref.py), and the host-side
refusals of the two reducer wrappers, which need no device: they must come before the library is even loaded."""
import numpy as np
import pytest
import torch

import gts
from gts import _lib, ops
from tests import reducers_ref as R

GEOMETRY_NS = [1, 2, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 60000, 2 ** 31 + 5]


@pytest.mark.parametrize("n", GEOMETRY_NS)
def test_chunk_geometry_tiles_the_rows(n):
    rpc, chunks = R.chunk_geometry(n)
    assert 1 <= chunks <= R.MAX_CHUNKS
    first = np.arange(chunks, dtype=np.int64) * rpc
    last = np.minimum(first + rpc, n)
    assert first[0] == 0 and last[-1] == n
    assert np.array_equal(first[1:], last[:-1])            # no gap, no overlap
    assert np.all(last > first)                            # no empty chunk: every partial sum is written
    for lane in range(R.LANES):                            # a lane walks its chunks in ascending order, each chunk once
        mine = np.arange(lane, chunks, R.LANES)
        assert np.all(np.diff(mine) > 0)
    owners = np.concatenate([np.arange(lane, chunks, R.LANES) for lane in range(R.LANES)])
    assert np.array_equal(np.sort(owners), np.arange(chunks))


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 8193, 60000])
def test_chunked_colsum_is_exact_on_small_integers(n):
    rng = np.random.default_rng(n)
    rows = rng.integers(-3, 4, size=(n, 12)).astype(np.float32)
    got = R.chunked_colsum_f32(rows)
    assert got.dtype == np.float32
    assert np.array_equal(got.astype(np.int64), rows.astype(np.int64).sum(0))


@pytest.mark.parametrize("n", [1, 17, 513, 1025, 8193, 60000])
def test_chunked_colsum_meets_the_depth_bound_on_random_rows(n):
    rng = np.random.default_rng(100 + n)
    rows = rng.standard_normal((n, 20), dtype=np.float32)
    rows[::3] *= np.float32(1e3)
    got = R.chunked_colsum_f32(rows).astype(np.float64)
    want, mag = R.colsum_f64(rows)
    assert np.all(np.abs(got - want) <= R.chain_depth(n) * R.U * mag)
    if n > 1:
        assert np.any(got != want)                         # it is an fp32 sum, not the float64 one rounded


def test_chunked_colsum_depends_on_the_association():
    """The restatement is order-sensitive where it should be: a value that only survives if the big terms cancel first."""
    rows = np.zeros((1024, 4), np.float32)                 # 2 rows per chunk: rows 0 and 1 share chunk 0
    rows[0], rows[1], rows[2] = 2.0 ** 30, -2.0 ** 30, 1.0
    assert np.array_equal(R.chunked_colsum_f32(rows), np.ones(4, np.float32))
    rows[1], rows[2] = 1.0, -2.0 ** 30                     # now 1.0 is absorbed inside chunk 0
    assert np.array_equal(R.chunked_colsum_f32(rows), np.zeros(4, np.float32))


def test_act_bwd_and_param_grad_references():
    out = np.array([[0.0, -0.0, -1.0, np.finfo(np.float32).tiny], [2.0, -0.5, 0.25, -3.0]], np.float32)
    g = np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]], np.float32)
    elu, bias = R.act_bwd_ref(g, out, 1)
    assert np.array_equal(elu, np.array([[1.0, 2.0, 0.0, 4.0], [5.0, 3.0, 7.0, -16.0]], np.float32))
    assert np.array_equal(bias, elu.sum(0))
    relu, _ = R.act_bwd_ref(g, out, 2)
    assert np.array_equal(relu, np.array([[0.0, 0.0, 0.0, 4.0], [5.0, 0.0, 7.0, 0.0]], np.float32))
    same, bias0 = R.act_bwd_ref(g, None, 0)
    assert same is g and np.array_equal(bias0, g.sum(0))
    ft = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    gel = np.array([[1, 0, -1], [2, 1, 3]], np.float32)
    gl, gr = R.param_grad_ref(ft, gel, -gel)
    assert np.array_equal(gl, np.einsum("nh,nhd->hd", gel, ft)) and np.array_equal(gr, -gl)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("lr,wd", [(3e-3, 1e-2), (1e-4, 0.0)])
def test_adamw_ref64_is_torch_adamw_in_float64(lr, wd, betas):
    """The one place where torch's optimizer is the judge: ten float64 steps on the CPU, 1e-12 relative."""
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(301)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([tp], lr=lr, betas=betas, eps=1e-8, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(301), np.zeros(301)
    for step in range(1, 11):
        g = rng.standard_normal(301) * step
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = R.adamw_ref64(p, g, m, v, lr, betas, 1e-8, wd, step)
        state = opt.state[tp]
        for mine, theirs in ((p, tp.detach()), (m, state["exp_avg"]), (v, state["exp_avg_sq"])):
            theirs = theirs.numpy()
            assert np.all(np.abs(mine - theirs) <= 1e-12 * np.abs(theirs)), step


def _worst(got, ref, bar):
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= bar), f"worst error / bar = {np.max(err[bar > 0] / bar[bar > 0]):.3f}"


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("lr,wd", [(3e-3, 1e-2), (1e-4, 0.0)])
@pytest.mark.parametrize("agree", [True, False])
def test_a_correctly_rounded_fp32_adamw_meets_the_bars_of_the_gpu_test(agree, lr, wd, betas, step):
    """The bars the device is held to (tests/test_gpu_reducers.py) are reachable: the kernel's arithmetic restated in numpy
    fp32 meets them on the GPU test's own data.  With the signs of m and g independent the p bar needs the cancellation
    allowance (it is not a theorem there: the restatement exceeds the plain bar at 2 of 4 198 403 such elements)."""
    n = 262144 + 4099
    p, g, m, v = R.adamw_case(n, step, 5, agree)
    ref_p, ref_m, ref_v, delta = R.adamw_ref64(p, g, m, v, lr, betas, 1e-8, wd, step, with_delta=True)
    bar_p, bar_m, bar_v = R.adamw_bars(p, g, m, ref_v, delta)
    if not agree:
        bar_p = bar_p + R.adamw_cancellation_allowance(g, m, ref_v, lr, betas, 1e-8, step)
    got_p, got_m, got_v = R.adamw_f32(p, g, m, v, lr, betas, 1e-8, wd, step)
    _worst(got_p, ref_p, bar_p)
    _worst(got_m, ref_m, bar_m)
    _worst(got_v, ref_v, bar_v)


def test_adamw_case_plants_the_edges():
    p, g, m, v = R.adamw_case(4099, 2, 1)
    assert np.any(g == 0) and np.any((np.abs(g) > 0) & (np.abs(g) < 1e-5)) and np.any(np.abs(g) > 500)
    assert np.all(v > 0) and np.all((m * g >= 0))
    p, g, m, v = R.adamw_case(4099, 1, 1)
    assert not m.any() and not v.any()
    p, g, m, v = R.adamw_case(4099, 2, 1, agree=False)
    assert np.any(m * g < 0)


# ---------------------------------------------------------------- wrapper refusals that need no device
@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to reach the library fails the test: the refusals below are decided on the host before that."""
    def load():
        raise AssertionError("the wrapper reached _lib.load() with operands it must refuse")
    monkeypatch.setattr(_lib, "load", load)


def test_gat_act_bwd_refuses_on_the_host(no_library):
    g, o = torch.zeros(6, 8), torch.ones(6, 8)
    for args in [(g, o, 3, True), (g, o, -1, False), (g, o, 1.5, True),            # activation
                 (torch.zeros(()), None, 0, True), (torch.zeros(0, 8), None, 0, True),   # no rows
                 (torch.zeros(6, 6), torch.ones(6, 6), 1, True), (torch.zeros(6, 6), None, 0, False),   # cols % 4
                 (g, None, 1, True), (g, o[:5], 2, True), (g, o.t().reshape(8, 6), 2, True),   # out missing / misshapen
                 (g.double(), o, 1, True), (g, o.double(), 2, True), (g.double(), None, 0, True),   # dtype
                 (g, o, 1, True), (g, None, 0, True)]:                                # CPU tensors
        with pytest.raises(gts.GtsError):
            ops.gat_act_bwd(*args)


def test_gat_param_grad_refuses_on_the_host(no_library):
    ft, ge = torch.zeros(6, 2, 8), torch.zeros(6, 2)
    for args in [(ft.reshape(6, 16), ge, ge), (ft, ge[:, :1], ge), (ft, ge, ge[:5]), (ft, ge.reshape(2, 6), ge),
                 (torch.zeros(6, 2, 6), ge, ge), (torch.zeros(0, 2, 8), ge[:0], ge[:0]),
                 (ft.double(), ge, ge), (ft, ge.double(), ge), (ft, ge, ge.double()),
                 (ft, ge, ge)]:                                                        # CPU tensors
        with pytest.raises(gts.GtsError):
            ops.gat_param_grad(*args)
