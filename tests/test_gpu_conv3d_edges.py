"""C1-C5 (csrc/gts_conv3d.hip) layer by layer against torch CPU fp64 over the instantiation and plan matrix:
every conv_kernel<CC, NT> and wgrad_kernel<CC, MT>, one and two channel chunks with last chunks of 1, 4, 13 and
16 real channels, on the forward route and on the data gradient's swapped one; volumes of exactly one brick,
one voxel over on every axis and one under in z; and weight-gradient split plans at each family's whole-launch
target and with a short last split.  tests/test_conv3d_cases_host.py asserts that the lists below reach all of
that (from tests/conv3d_ref.plan, which it ties to the library's workspace queries) and that the integer-valued
operands stay exactly representable.

Each case runs twice.  Integer-valued operands (x, bias in -3..3, weights, dy in -2..2, stored as float32):
every product and every partial sum in any order is an exact float32, so the result must EQUAL the fp64
reference; a wrong tap, channel, clamp, flip, chunk stride or dropped brick shows at any magnitude.  Random
normal operands as in test_gpu_conv3d.py, held to that file's rule |err| <= 2e-6 * bound."""
import functools

import pytest
import torch

from tests.conv3d_ref import conv, d64, data_grad, weight_grad

DEV = torch.device("cuda", 0)

# ---- case lists (plain data: the host test imports them without a GPU) --------------------------------
CHANNEL_PAIRS = [(1, 17), (4, 32), (5, 31), (8, 16), (9, 17), (12, 32), (13, 1), (16, 31), (16, 16), (17, 16),
                 (20, 15), (29, 1), (32, 32), (1, 1),
                 # the data gradient swaps the counts: CC 8 and 12 there need 5..12 OUTPUT channels
                 (12, 8), (8, 12), (20, 5), (31, 9)]
CHANNEL_VOLUMES = [(5, 5, 17), (3, 4, 15)]
VOLUMES = [(4, 4, 16), (5, 5, 17), (3, 4, 15), (1, 9, 33), (9, 1, 16), (8, 8, 32)]
VOLUME_CHANNELS = [(12, 20), (17, 3)]
LAYER_CASES = ([(d, ci, co) for d in CHANNEL_VOLUMES for ci, co in CHANNEL_PAIRS] +
               [(d, ci, co) for d in VOLUMES for ci, co in VOLUME_CHANNELS])

# weight gradient only: (cin, volume), each at both output widths
SPLIT_ROWS = [
    (17, (16, 16, 64)), (32, (20, 52, 16)), (29, (20, 52, 32)),                    # two chunks, target 64
    (16, (16, 32, 64)), (13, (12, 36, 80)),                                        # CC 16, target 128
    (10, (34, 75, 13)), (9, (20, 28, 80)), (12, (20, 28, 80)),                     # CC 12, target 171
    (6, (31, 30, 50)), (5, (20, 44, 80)), (8, (20, 44, 80)),                       # CC 8, target 256
    (2, (29, 30, 113)), (1, (36, 76, 48)), (4, (36, 76, 48)),                      # CC 4, target 512
]
SPLIT_COUTS = (16, 17)
WGRAD_CASES = [(d, ci, co) for ci, d in SPLIT_ROWS for co in SPLIT_COUTS]
REPEAT_CASE = ((20, 52, 16), 32, 17)                                               # two chunks, short last split
KINDS = ("integer", "normal")


def case_id(case):
    dims, cin, cout = case
    return "x".join(map(str, dims)) + f"-{cin}-{cout}"


# ---- operands -----------------------------------------------------------------------------------------
def _generator(dims, cin, cout, salt):
    return torch.Generator().manual_seed((((dims[0] * 131 + dims[1]) * 131 + dims[2]) * 64 + cin) * 64 + cout + salt)


def integer_operands(dims, cin, cout):
    """(x, w, b, dy) with small integer values: no operation on them rounds in float32."""
    g = _generator(dims, cin, cout, 0)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    return (ints(-3, 3, *dims, cin), ints(-2, 2, cout, cin, 5, 5, 5), ints(-3, 3, cout),
            ints(-2, 2, dims[0] * dims[1] * dims[2], cout))


def normal_operands(dims, cin, cout):
    g = _generator(dims, cin, cout, 1 << 40)
    x = torch.randn(*dims, cin, generator=g)
    w = torch.randn(cout, cin, 5, 5, 5, generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    dy = torch.randn(dims[0] * dims[1] * dims[2], cout, generator=g)
    return x, w, b, dy


def relu_output(dims, cin, cout):
    """A stand-in for the ReLU output that fed the layer, [V, cin]: positive and negative values and both zeros."""
    g = _generator(dims, cin, cout, 2 << 40)
    h = torch.randint(-2, 3, (dims[0] * dims[1] * dims[2], cin), generator=g).float()
    flat = h.view(-1)
    flat[torch.arange(flat.numel()) % 2 == 1] *= -1.0          # every second zero becomes -0.0
    flat[:4] = torch.tensor([1.0, -1.0, 0.0, -0.0])
    return h


def _operands(case, kind):
    ops = integer_operands(*case) if kind == "integer" else normal_operands(*case)
    return ops, tuple(t.to(DEV) for t in ops)


# ---- comparisons --------------------------------------------------------------------------------------
def _compare(kind, what, got, want, bound):
    got = d64(got).reshape(want.shape)
    if kind == "integer":
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (f"{what}: {bad.shape[0]} of {want.numel()} values differ from fp64, first at "
                                  f"{bad[:8].tolist()}: got {[got[tuple(i)].item() for i in bad[:8]]}, "
                                  f"want {[want[tuple(i)].item() for i in bad[:8]]}")
    else:
        err = (got - want).abs()
        assert torch.all(err <= 2e-6 * bound().reshape(want.shape) + 1e-30), f"{what}: max err {err.max():.3e}"


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _weight_gradient(case, kind):
    from gts import conv3d

    (x, _, _, dy), (xd, _, _, dyd) = _operands(case, kind)
    cout = case[2]
    dw, db = conv3d.conv3d_bwd_weight(xd, dyd, cout)
    want_w, want_b = weight_grad(x.double(), dy.double(), cout)
    bound = functools.lru_cache(None)(lambda: weight_grad(x.double().abs(), dy.double().abs(), cout))
    _compare(kind, "dw", dw, want_w, lambda: bound()[0])
    _compare(kind, "db", db, want_b, lambda: bound()[1])
    dw_only, no_db = conv3d.conv3d_bwd_weight(xd, dyd, cout, want_bias=False)
    assert no_db is None
    assert _same_bits(dw_only, dw), "dw changes with want_bias=False"


# ---- tests --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", LAYER_CASES, ids=case_id)
def test_forward_against_fp64(hip_lib, case, kind):
    from gts import conv3d

    (x, w, b, _), (xd, wd, bd, _) = _operands(case, kind)
    pre = conv(x.double(), w.double(), b.double())
    bound = functools.lru_cache(None)(lambda: conv(x.double().abs(), w.double().abs(), b.double().abs()))
    _compare(kind, "conv", conv3d.conv3d_fwd(xd, wd, bd, relu=False), pre, bound)
    _compare(kind, "relu(conv)", conv3d.conv3d_fwd(xd, wd, bd, relu=True), pre.clamp(min=0), bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", LAYER_CASES, ids=case_id)
def test_data_gradient_against_fp64(hip_lib, case, kind):
    from gts import conv3d

    dims = case[0]
    (_, w, _, dy), (_, wd, _, dyd) = _operands(case, kind)
    want = data_grad(dy.double(), w.double(), dims)
    bound = functools.lru_cache(None)(lambda: data_grad(dy.double().abs(), w.double().abs(), dims))
    _compare(kind, "dx", conv3d.conv3d_bwd_data(dyd, wd, dims), want, bound)
    h = relu_output(*case)
    assert (h > 0).any() and (h < 0).any() and (h == 0).any()
    assert ((h == 0) & torch.signbit(h)).any() and ((h == 0) & ~torch.signbit(h)).any()
    mask = (h > 0).double()
    _compare(kind, "masked dx", conv3d.conv3d_bwd_data(dyd, wd, dims, h=h.to(DEV)), want * mask,
             lambda: bound() * mask)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", LAYER_CASES, ids=case_id)
def test_weight_gradient_against_fp64(hip_lib, case, kind):
    _weight_gradient(case, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", WGRAD_CASES, ids=case_id)
def test_weight_gradient_split_plans_against_fp64(hip_lib, case, kind):
    _weight_gradient(case, kind)


@pytest.mark.gpu
def test_short_last_split_with_two_chunks_repeats_bit_for_bit(hip_lib):
    from gts import conv3d

    dims, _, cout = REPEAT_CASE
    _, (xd, wd, bd, dyd) = _operands(REPEAT_CASE, "normal")
    hd = relu_output(*REPEAT_CASE).to(DEV)
    runs = []
    for _ in range(2):
        runs.append([conv3d.conv3d_fwd(xd, wd, bd, relu=True), conv3d.conv3d_bwd_data(dyd, wd, dims, h=hd),
                     *conv3d.conv3d_bwd_weight(xd, dyd, cout)])
    for a, b in zip(*runs):
        assert _same_bits(a, b)
