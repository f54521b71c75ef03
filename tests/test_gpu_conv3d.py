"""C1-C5 (csrc/gts_conv3d.hip) against torch CPU fp64: every launch of a refinement-CNN training step
at volumes whose every voxel is near a boundary, a 48^3 brick and one crop above 2 M voxels, for the
hyper-parameters' 8->16->4, the shipped checkpoint's 9->16->5 and an odd 3->7->2.  Tolerance as in
test_gpu_gemm.py: |err| <= 2e-6 * bound, bound = the operation on absolute values.  The matrix of kernel
instantiations, brick-edge volumes and weight-gradient split plans is in test_gpu_conv3d_edges.py."""
import pytest
import torch

from tests.conv3d_ref import conv, d64, data_grad, weight_grad

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(1, 1, 1), (2, 3, 40), (7, 9, 11), (48, 48, 48)]
CHANNELS = [(8, 16, 4), (9, 16, 5), (3, 7, 2)]


def _check(got, want, bound):
    err = (d64(got) - want).abs()
    assert torch.all(err <= 2e-6 * bound + 1e-30), f"max err {err.max():.3e}, bound {bound.max():.3e}"


def _operands(dims, cin, cmid, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*dims, cin, generator=g)
    w1 = torch.randn(cmid, cin, 5, 5, 5, generator=g) * 0.1
    b1 = torch.randn(cmid, generator=g)
    w2 = torch.randn(cout, cmid, 5, 5, 5, generator=g) * 0.1
    b2 = torch.randn(cout, generator=g)
    dy = torch.randn(dims[0] * dims[1] * dims[2], cout, generator=g)
    return x, w1, b1, w2, b2, dy


def _layer_checks(dims, cin, cmid, cout, seed):
    from gts import conv3d

    x, w1, b1, w2, b2, dy = _operands(dims, cin, cmid, cout, seed)
    xd, w1d, b1d, w2d, b2d, dyd = (t.to(DEV) for t in (x, w1, b1, w2, b2, dy))
    # C1 with and without the ReLU
    pre = conv(x.double(), w1.double(), b1.double())
    bound1 = conv(x.double().abs(), w1.double().abs(), b1.double().abs())
    _check(conv3d.conv3d_fwd(xd, w1d, b1d, relu=False), pre, bound1)
    h1 = conv3d.conv3d_fwd(xd, w1d, b1d, relu=True)
    _check(h1, pre.clamp(min=0), bound1)
    # C2 on the GPU's own H1 (so both sides see the same operand)
    h1_64 = d64(h1).reshape(*dims, cmid)
    _check(conv3d.conv3d_fwd(h1.view(*dims, cmid), w2d, b2d, relu=False), conv(h1_64, w2.double(), b2.double()),
           conv(h1_64.abs(), w2.double().abs(), b2.double().abs()))
    # C3: replicate adjoint, then the ReLU mask
    want = data_grad(dy.double(), w2.double(), dims)
    bound = data_grad(dy.double().abs(), w2.double().abs(), dims)
    _check(conv3d.conv3d_bwd_data(dyd, w2d, dims), want, bound)
    mask = (d64(h1) > 0).double()
    dz1 = conv3d.conv3d_bwd_data(dyd, w2d, dims, h=h1)
    _check(dz1, want * mask, bound * mask)
    # C4 / C5
    for inp, grad, c in ((h1.view(*dims, cmid), dyd, cout), (xd, dz1, cmid)):
        dw, db = conv3d.conv3d_bwd_weight(inp, grad, c)
        want_w, want_b = weight_grad(d64(inp), d64(grad), c)
        bound_w, bound_b = weight_grad(d64(inp).abs(), d64(grad).abs(), c)
        _check(dw, want_w, bound_w)
        _check(db, want_b, bound_b)


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("channels", CHANNELS, ids=lambda c: "-".join(map(str, c)))
def test_every_launch_against_fp64(hip_lib, dims, channels):
    _layer_checks(dims, *channels, seed=sum(dims) * 100 + sum(channels))


def test_wide_channels_and_two_chunks(hip_lib):
    """Channel counts past one LDS chunk (17..32) and past one 16-wide N tile."""
    _layer_checks((5, 6, 19), 20, 32, 17, seed=7)


def test_crop_above_two_million_voxels(hip_lib):
    """128 x 144 x 112 (2.06 M voxels), 8->16->4: all five launches, the weight gradients split over every brick."""
    from gts import conv3d

    dims, cin, cmid, cout = (128, 144, 112), 8, 16, 4
    x, w1, b1, w2, b2, dy = _operands(dims, cin, cmid, cout, seed=3)
    xd, w1d, b1d, w2d, b2d, dyd = (t.to(DEV) for t in (x, w1, b1, w2, b2, dy))
    h1 = conv3d.conv3d_fwd(xd, w1d, b1d, relu=True)                                           # C1
    _check(h1, conv(x.double(), w1.double(), b1.double()).clamp(min=0),
           conv(x.double().abs(), w1.double().abs(), b1.double().abs()))
    h1_64 = d64(h1).reshape(*dims, cmid)
    _check(conv3d.conv3d_fwd(h1.view(*dims, cmid), w2d, b2d, relu=False),                   # C2
           conv(h1_64, w2.double(), b2.double()), conv(h1_64.abs(), w2.double().abs(), b2.double().abs()))
    dz1 = conv3d.conv3d_bwd_data(dyd, w2d, dims, h=h1)                                        # C3
    mask = (d64(h1) > 0).double()
    _check(dz1, data_grad(dy.double(), w2.double(), dims) * mask,
           data_grad(dy.double().abs(), w2.double().abs(), dims) * mask)
    for inp, grad, c in ((h1.view(*dims, cmid), dyd, cout), (xd, dz1, cmid)):                # C4, C5
        dw, db = conv3d.conv3d_bwd_weight(inp, grad, c)
        want_w, want_b = weight_grad(d64(inp), d64(grad), c)
        bound_w, bound_b = weight_grad(d64(inp).abs(), d64(grad).abs(), c)
        _check(dw, want_w, bound_w)
        _check(db, want_b, bound_b)


def test_mismatched_operands_are_refused_before_a_launch(hip_lib):
    from gts import _lib, conv3d

    x = torch.zeros(4, 5, 6, 8, device=DEV)
    w1, b1 = torch.zeros(16, 8, 5, 5, 5, device=DEV), torch.zeros(16, device=DEV)
    w2 = torch.zeros(4, 16, 5, 5, 5, device=DEV)
    v = 4 * 5 * 6
    bad = [
        lambda: conv3d.conv3d_fwd(x, torch.zeros(16, 9, 5, 5, 5, device=DEV), b1, True),     # Cin of w vs x
        lambda: conv3d.conv3d_fwd(x, torch.zeros(16, 8, 3, 3, 3, device=DEV), b1, True),     # kernel size
        lambda: conv3d.conv3d_fwd(x, w1, torch.zeros(15, device=DEV), True),                  # bias length
        lambda: conv3d.conv3d_fwd(x.double(), w1, b1, True),                                  # dtype
        lambda: conv3d.conv3d_bwd_data(torch.zeros(v, 5, device=DEV), w2, (4, 5, 6)),         # dy channels
        lambda: conv3d.conv3d_bwd_data(torch.zeros(v - 1, 4, device=DEV), w2, (4, 5, 6)),     # dy voxels
        lambda: conv3d.conv3d_bwd_data(torch.zeros(v, 4, device=DEV), w2, (4, 5, 6),
                                       h=torch.zeros(v, 8, device=DEV)),                      # mask channels
        lambda: conv3d.conv3d_bwd_weight(x, torch.zeros(v, 15, device=DEV), 16),              # dy vs cout
        lambda: conv3d.conv3d_bwd_weight(x, torch.zeros(v + 1, 16, device=DEV), 16),          # dy voxels
    ]
    for call in bad:
        with pytest.raises(_lib.GtsError):
            call()


def test_two_runs_give_identical_bits(hip_lib):
    from gts import conv3d
    from model.networks import CnnRefinementNet

    torch.manual_seed(0)
    net = CnnRefinementNet(8, 4, [16]).to(DEV)
    x = torch.randn(40, 37, 29, 8, device=DEV)
    runs = []
    for _ in range(2):
        net.zero_grad()
        y = conv3d.refinement_logits(x, net)
        (y * torch.linspace(-1, 1, y.numel(), device=DEV).view_as(y)).sum().backward()
        runs.append([y.detach().clone()] + [p.grad.clone() for p in net.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
