"""gts.ops.dice_ce_loss (csrc/gts_dice_ce.hip) on the GPU against the float64 definition of tests/dice_ref.py
evaluated on the same float32 inputs.

Bounds.  The loss and each part lie within 1e-5 |ref| (the bound tests/test_gpu_refinement.py holds the
cross-entropy kernel to): the fixed-association float32 sums err by about (log2 N + 10) 2^-24 <= 2.5e-6.  Every
gradient entry lies within 1e-5 S_bound |upstream|, S_bound = ce_weight max_c w_c / sum w + dice_weight
sum_r (|a_r| + |b_r|) being the largest possible |dL/dp|: relative to the coefficients, not to the largest entry,
because on saturated logits the true gradient is ~1e-18 of the coefficients and the rounding of g - sum g p is not.

B = rows per workgroup of the two streaming kernels, F = threads of the finishing kernel.
"""
import math

import pytest
import torch

from tests import dice_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
B, F = 1024, 256
ROW_COUNTS = [1, 2, 63, 64, 65, B - 1, B, B + 1, B * F + 3]
UPSTREAM = 2.5
W4 = [0.1, 1.0, 2.0, 2.0]
KINDS = ["gaussian", "equal", "saturated", "class_absent", "region_absent", "one_class", "ignored"]


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def make_inputs(kind, n, c, seed):
    """(logits float32 [n, c], labels int64 [n]) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * 3
    y = torch.randint(0, c, (n,), generator=g)
    if kind == "equal":                      # every class equally likely: p = 1 / C exactly
        x = torch.full((n, c), 0.75)
    elif kind == "saturated":                # +-40: p is one-hot in float32; the predicted class is mostly wrong
        x = torch.full((n, c), -40.0)
        x[torch.arange(n), torch.randint(0, c, (n,), generator=g)] = 40.0
    elif kind == "class_absent":             # the last class never occurs in the truth, only in the prediction
        y = torch.randint(0, max(1, c - 1), (n,), generator=g)
    elif kind == "region_absent":            # the last class neither occurs nor is predicted (its mass is ~e^-80)
        x = torch.full((n, c), -40.0)
        x[torch.arange(n), torch.randint(0, max(1, c - 1), (n,), generator=g)] = 40.0
        y = torch.randint(0, max(1, c - 1), (n,), generator=g)
    elif kind == "one_class":
        y = torch.full((n,), c - 1, dtype=torch.int64)
    elif kind == "ignored":                  # 10 % of the rows: at least one where there are two, never row 0
        drop = torch.rand(n, generator=g) < 0.1
        drop[n // 2] = True
        drop[0] = False
        y[drop] = dice_ref.IGNORE
    else:
        assert kind == "gaussian"
    return x.float().contiguous(), y


def run_gpu(x, y, class_w, upstream=UPSTREAM, **kw):
    from gts import ops

    xd = x.to(DEV).requires_grad_(True)
    wd = None if class_w is None else class_w.to(DEV)
    loss, parts = ops.dice_ce_loss(xd, y.to(DEV), wd, return_parts=True, **kw)
    assert loss.shape == () and loss.dtype == torch.float32 and not parts.requires_grad
    (upstream * loss).backward()
    return loss.detach(), parts, xd.grad


def check_case(x, y, class_w, tag, **kw):
    """Run forward + backward on the GPU and hold loss, parts and gradient to the reference.  Returns the largest
    ratios error / bound met (loss and parts, gradient)."""
    loss, parts, grad = run_gpu(x, y, class_w, **kw)
    ref = dice_ref.dice_ce_ref(x, y, class_w, kw.get("regions", "brats"), kw.get("ce_weight", 1.0),
                               kw.get("dice_weight", 1.0), kw.get("smooth", 1.0))
    want = torch.cat([ref.loss[None], ref.ce[None], ref.l_dice[None], ref.dices])
    got = torch.cat([loss[None], parts]).cpu().double()
    assert got.shape == want.shape
    err = (got - want).abs()
    bound = 1e-5 * want.abs()
    g_err = float((grad.cpu().double() - UPSTREAM * ref.grad).abs().max())
    g_bound = 1e-5 * ref.s_bound * UPSTREAM
    ratios = (float((err / bound.clamp(min=1e-300)).max()), g_err / g_bound)
    print(f"{tag}: loss {float(want[0]):.6f} parts err/bound {ratios[0]:.3f}, grad err {g_err:.3e} "
          f"bound {g_bound:.3e} ratio {ratios[1]:.3f}")
    assert bool((err <= bound).all()), f"{tag}: got {got.tolist()} want {want.tolist()}"
    assert g_err <= g_bound, f"{tag}: gradient error {g_err:.3e} above {g_bound:.3e}"
    assert bool((grad[(y == dice_ref.IGNORE).to(DEV)] == 0).all())
    return ratios


@pytest.mark.parametrize("regions", ["brats", "classes"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_four_classes_against_fp64(n, regions):
    w = torch.tensor(W4)
    worst = (0.0, 0.0)
    for k, kind in enumerate(KINDS):
        x, y = make_inputs(kind, n, 4, seed=1000 * k + n)
        for class_w in (w, None):
            tag = f"C=4 {regions} N={n} {kind} {'weighted' if class_w is not None else 'unweighted'}"
            r = check_case(x, y, class_w, tag, regions=regions)
            worst = tuple(max(a, b) for a, b in zip(worst, r))
    print(f"C=4 {regions} N={n}: largest ratios {worst[0]:.3f} (loss, parts) {worst[1]:.3f} (gradient)")


EXPLICIT = {
    2: [[1]],
    4: [[1, 2, 3], [2, 3], [3], [0], [1, 3]],                     # five regions: the 8-region form at C = 4
    5: [[1, 2, 3, 4], [2, 4], [3], [0, 4]],
    32: [[31], [0, 1], list(range(1, 32)), [7], list(range(16, 32)), [0, 31], [2, 3, 5, 7, 11, 13], [30]],
}


@pytest.mark.parametrize("c", [2, 4, 5, 32])
def test_runtime_class_count_and_explicit_regions(c):
    g = torch.Generator().manual_seed(c)
    w = torch.rand(c, generator=g) + 0.1
    for n in (65, B + 1):
        for k, kind in enumerate(KINDS):
            x, y = make_inputs(kind, n, c, seed=77 * k + n + c)
            for class_w in (w, None):
                check_case(x, y, class_w, f"C={c} N={n} {kind}", regions=EXPLICIT[c])


@pytest.mark.parametrize("n", [65, B + 1, B * F + 3])
def test_term_weights_smooth_and_upstream(n):
    w = torch.tensor(W4)
    x, y = make_inputs("ignored", n, 4, seed=n)
    check_case(x, y, w, f"N={n} ce 0.3 dice 1.7 smooth 1e-5", ce_weight=0.3, dice_weight=1.7, smooth=1e-5)
    check_case(x, y, w, f"N={n} ce off", ce_weight=0.0)
    check_case(x, y, None, f"N={n} dice off", dice_weight=0.0, regions="classes")


@pytest.mark.parametrize("n", [65, B + 1, B * F + 3])
def test_without_the_dice_term_it_is_the_weighted_cross_entropy(n):
    """Same bounds, not the same bits: the two kernels associate their sums differently."""
    from gts import ops

    w = torch.tensor(W4)
    for class_w in (w, None):
        x, y = make_inputs("ignored", n, 4, seed=3 * n)
        loss, parts, grad = run_gpu(x, y, class_w, dice_weight=0.0)
        xd = x.to(DEV).requires_grad_(True)
        other = ops.weighted_cross_entropy(xd, y.to(DEV), None if class_w is None else class_w.to(DEV))
        (UPSTREAM * other).backward()
        ref = dice_ref.dice_ce_ref(x, y, class_w, "brats", 1.0, 0.0, 1.0)
        assert abs(float(loss) - float(other)) <= 1e-5 * abs(float(ref.loss))
        assert float(parts[0]) == float(loss) and float(parts[1]) == 0.0
        assert float((grad - xd.grad).abs().max()) <= 1e-5 * ref.s_bound * UPSTREAM


@pytest.mark.parametrize("n", [1, 65, B + 1])
def test_all_rows_ignored(n):
    from gts import ops

    x, _ = make_inputs("gaussian", n, 4, seed=n)
    y = torch.full((n,), dice_ref.IGNORE, dtype=torch.int64)
    loss, parts, grad = run_gpu(x, y, torch.tensor(W4), ce_weight=0.0)
    assert float(loss) == 0.0 and float(parts[1]) == 0.0 and bool((parts[2:] == 1.0).all())
    assert bool((grad == 0).all())
    # with the cross-entropy on it is 0 / 0, as torch's
    assert math.isnan(float(ops.dice_ce_loss(x.to(DEV), y.to(DEV))))


@pytest.mark.parametrize("n", [1, 65, B + 1])
@pytest.mark.parametrize("c", [4, 5])
def test_a_label_out_of_range_poisons_the_loss(n, c):
    from gts import ops

    x, y = make_inputs("gaussian", n, c, seed=n + c)
    for bad in (c, -1):
        y[n // 2] = bad
        for kw in (dict(), dict(ce_weight=0.0), dict(dice_weight=0.0)):
            assert math.isnan(float(ops.dice_ce_loss(x.to(DEV), y.to(DEV), regions="classes", **kw)))
        assert math.isnan(float(dice_ref.dice_ce_ref(x, y, None, "classes").loss))


@pytest.mark.parametrize("n,c", [(B + 1, 4), (B * F + 3, 4), (B + 1, 5)])
def test_two_calls_return_the_same_bits(n, c):
    x, y = make_inputs("ignored", n, c, seed=n)
    w = torch.rand(c) + 0.1
    a = run_gpu(x, y, w, regions="classes")
    b = run_gpu(x, y, w, regions="classes")
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("n", [65, B + 1])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_rows_that_are_not_16_byte_aligned(n, shift):
    """A contiguous [N, 4] view `shift` floats into its storage: the one-access-per-row form does not apply, the
    result is held to the same bounds; the gradient of the view lands in the buffer it is a view of."""
    from gts import ops

    x, y = make_inputs("ignored", n, 4, seed=n + shift)
    ref = dice_ref.dice_ce_ref(x, y, torch.tensor(W4), "brats")
    buf = torch.zeros(4 * n + 4, device=DEV)
    buf[shift:shift + 4 * n] = x.reshape(-1).to(DEV)
    buf.requires_grad_(True)
    view = buf[shift:shift + 4 * n].view(n, 4)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * shift
    loss = ops.dice_ce_loss(view, y.to(DEV), torch.tensor(W4, device=DEV))
    loss.backward()
    assert abs(float(loss.detach()) - float(ref.loss)) <= 1e-5 * abs(float(ref.loss))
    got = buf.grad[shift:shift + 4 * n].view(n, 4).cpu().double()
    assert float((got - ref.grad).abs().max()) <= 1e-5 * ref.s_bound
    assert float(buf.grad[:shift].abs().max()) == 0 and float(buf.grad[shift + 4 * n:].abs().max()) == 0


def test_upstream_gradient_of_another_dtype_or_offset():
    """The upstream gradient as autograd may hand it over: a float64 scalar, and a float32 scalar that is a view
    at a storage offset; both give 2.5 times the gradient."""
    from gts import ops

    x, y = make_inputs("gaussian", B + 1, 4, seed=4)
    ref = dice_ref.dice_ce_ref(x, y, None, "brats")
    ups = (torch.tensor(UPSTREAM, dtype=torch.float64, device=DEV),
           torch.tensor([0.0, UPSTREAM, 0.0], device=DEV)[1],
           torch.tensor([UPSTREAM], device=DEV).expand(3)[2])
    grads = []
    for up in ups:
        xd = x.to(DEV).requires_grad_(True)
        ops.dice_ce_loss(xd, y.to(DEV)).backward(gradient=up)
        grads.append(xd.grad)
        assert float((xd.grad.cpu().double() - UPSTREAM * ref.grad).abs().max()) <= 1e-5 * ref.s_bound * UPSTREAM
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


def test_a_second_derivative_is_refused():
    """D2 is a raw kernel: its output is not differentiable, and asking for it raises instead of treating the
    gradient as a constant."""
    from gts import ops

    x, y = make_inputs("gaussian", 65, 4, seed=5)
    xd = x.to(DEV).requires_grad_(True)
    (grad,) = torch.autograd.grad(ops.dice_ce_loss(xd, y.to(DEV)), xd, create_graph=True)
    assert not grad.requires_grad
    with pytest.raises(RuntimeError):
        grad.sum().backward()
    # an upstream factor that itself wants a gradient reaches the function's own refusal
    factor = torch.tensor(UPSTREAM, device=DEV, requires_grad=True)
    (grad,) = torch.autograd.grad(factor * ops.dice_ce_loss(xd, y.to(DEV)), xd, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        grad.sum().backward()


def test_no_grad_runs_the_statistics_pass_alone(hip_lib, monkeypatch):
    from gts import ops

    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = hip_lib.gts_dice_ce_fwd_f32, hip_lib.gts_dice_ce_bwd_f32

    def counted(name, fn):
        def call(*args):
            calls[name] += 1
            return fn(*args)
        return call

    monkeypatch.setattr(hip_lib, "gts_dice_ce_fwd_f32", counted("fwd", fwd))
    monkeypatch.setattr(hip_lib, "gts_dice_ce_bwd_f32", counted("bwd", bwd))
    n = B * F + 3
    x, y = make_inputs("gaussian", n, 4, seed=1)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        loss = ops.dice_ce_loss(xd, yd)
    torch.cuda.synchronize()
    assert calls == {"fwd": 1, "bwd": 0} and not loss.requires_grad
    # no [N, 4] gradient (4 MiB) was allocated: partials, the stats block and the scalar are a few KiB
    assert torch.cuda.max_memory_allocated() - before < 1 << 20
    loss = ops.dice_ce_loss(xd, yd)
    assert calls == {"fwd": 2, "bwd": 0} and loss.requires_grad      # the forward never launches D2
    loss.backward()
    assert calls == {"fwd": 2, "bwd": 1} and xd.grad is not None


def test_input_checks():
    from gts import _lib, ops

    x, y = make_inputs("gaussian", 10, 4, seed=0)
    xd, yd = x.to(DEV), y.to(DEV)
    for bad in (lambda: ops.dice_ce_loss(x, y), lambda: ops.dice_ce_loss(xd.double(), yd),
                lambda: ops.dice_ce_loss(xd, yd.int()), lambda: ops.dice_ce_loss(xd, yd[:5]),
                lambda: ops.dice_ce_loss(xd, yd, torch.ones(3, device=DEV)),
                lambda: ops.dice_ce_loss(xd, yd, ce_weight=-1.0), lambda: ops.dice_ce_loss(xd, yd, smooth=0.0),
                lambda: ops.dice_ce_loss(xd[:, :3].contiguous(), yd), lambda: ops.dice_ce_loss(xd, yd, regions=[[4]])):
        with pytest.raises(_lib.GtsError):
            bad()
