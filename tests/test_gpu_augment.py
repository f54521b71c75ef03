"""The augmentation kernels (csrc/gts_augment.hip) against tests/augment_ref.py on the GPU.

Without noise everything is bit-equal to numpy: the mirror to np.flip, the affine to float32 `x * a + b` (a multiply,
then an add: the library is built without fp contraction, no fma on either side).  With noise the bound is
2e-5 sigma on the noise term, derived, not measured: the radius is at most sqrt(2 * 24 ln 2) = 5.77, the float32
angle carries about 2 pi 2^-24, logf / sqrtf / sinf / cosf a few ulps: about 4e-6 in the worst case, a 5x margin.
The final float32 add rounds x' by half an ulp of |x'| < 8 here, 4.8e-7: the sigmas of these tests (>= 0.25) keep
that below a tenth of the bound, so it needs no allowance of its own."""
import itertools

import numpy as np
import pytest
import torch

from tests import augment_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FLIPS = list(itertools.product((False, True), repeat=3))
CROPS = [(1, 1, 1), (5, 3, 7), (2, 16, 33), (3, 2, 130)]
LAYOUTS = [(8, 4), (4, 1), (5, 3), (4, 0), (4, 4)]


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _plan(ci, flips=(False, False, False), sigma=None, seed=(1234, 0), step=3, rng=None, feature_sigma=0.0):
    from gts.augment import AugmentPlan

    rng = rng or np.random.default_rng(ci)
    scale = rng.uniform(0.7, 1.3, ci).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, ci).astype(np.float32)
    if ci > 1:                              # one channel that is copied, not multiplied
        scale[1], shift[1] = 1.0, 0.0
    sigma = np.zeros(ci, dtype=np.float32) if sigma is None else np.asarray(sigma, dtype=np.float32)
    return AugmentPlan(flips, scale, shift, sigma, feature_sigma, seed, step)


def _sample(shape, channels, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape + (channels,)).astype(np.float32)
    labels = rng.integers(0, 4, shape).astype(np.int64)
    return x, labels


def _run(x, labels, plan):
    from gts import ops

    xd = torch.from_numpy(x).to(DEV) if x is not None else None
    ld = torch.from_numpy(labels).to(DEV) if labels is not None else None
    xo, lo = ops.augment_crop(xd, ld, plan)
    if xd is not None:
        assert xo.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), torch.from_numpy(x))      # never in place
    return (xo.cpu().numpy() if xo is not None else None), (lo.cpu().numpy() if lo is not None else None)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"C{l[0]}_Ci{l[1]}")
@pytest.mark.parametrize("shape", CROPS, ids=lambda s: "x".join(map(str, s)))
def test_crop_without_noise_is_bit_equal(shape, layout):
    channels, ci = layout
    x, labels = _sample(shape, channels, seed=sum(shape))
    x.reshape(-1)[0] = -0.0
    for flips in FLIPS:
        plan = _plan(ci, flips)
        got_x, got_l = _run(x, labels.reshape(-1), plan)
        want_x, want_l = augment_ref.crop_no_noise(x, labels, plan)
        assert got_x.tobytes() == want_x.tobytes(), f"flips {flips}"
        assert np.array_equal(got_l, want_l.reshape(-1)), f"flips {flips}"


def test_x_alone_and_labels_alone():
    x, labels = _sample((5, 3, 7), 8)
    plan = _plan(4, (True, False, True))
    want_x, want_l = augment_ref.crop_no_noise(x, labels, plan)
    got_x, none = _run(x, None, plan)
    assert none is None and got_x.tobytes() == want_x.tobytes()
    none, got_l = _run(None, labels, plan)
    assert none is None and got_l.shape == labels.shape and np.array_equal(got_l, want_l)


def test_identity_plan_returns_the_input_bits():
    from gts.augment import AugmentPlan

    x, labels = _sample((5, 3, 7), 8)
    x[0, 0, 0, :] = -0.0
    x[1, 1, 1, 2] = np.float32(1e-42)          # a denormal stays one
    for channels in (8, 5):
        xs = np.ascontiguousarray(x[..., :channels])
        got_x, got_l = _run(xs, labels, AugmentPlan.identity(4))
        assert got_x.tobytes() == xs.tobytes() and np.array_equal(got_l, labels)
        assert np.all(np.signbit(got_x[0, 0, 0, :]))


@pytest.mark.parametrize("layout", [(8, 4), (9, 5)], ids=lambda l: f"C{l[0]}_Ci{l[1]}")
def test_crop_noise_against_the_reference_bits(layout):
    channels, ci = layout
    shape = (5, 3, 7)
    x, _ = _sample(shape, channels, seed=9)
    sigma = [0.5, 1.0, 0.0, 0.25, 0.75][:ci]
    worst = 0.0
    for flips in ((False, False, False), (True, True, False), (True, True, True)):
        plan = _plan(ci, flips, sigma=sigma, seed=(0xDEADBEEF, 0x1234), step=(7 << 32) | 5)
        got, _ = _run(x, None, plan)
        base, _ = augment_ref.crop_no_noise(x, None, plan)
        noise = augment_ref.crop_noise(shape, channels, plan)
        assert np.any(noise[..., 0] != 0) and not np.any(noise[..., 2]) and not np.any(noise[..., ci:])
        err = np.abs((got.astype(np.float64) - base.astype(np.float64)) - noise)
        for c in range(channels):
            s = float(plan.sigma[c]) if c < ci else 0.0
            if s == 0.0:        # nothing is drawn and nothing is added: the bits of the no-noise form
                assert got[..., c].tobytes() == np.ascontiguousarray(base[..., c]).tobytes()
                continue
            worst = max(worst, float(err[..., c].max()) / s)
            assert err[..., c].max() <= 2e-5 * s, f"channel {c}: {err[..., c].max():.3e}"
    print(f"largest noise error / sigma, C = {channels}: {worst:.3e}")


def test_noise_depends_on_step_and_is_reproducible():
    x, _ = _sample((5, 3, 7), 8)
    a = _plan(4, sigma=[0.5, 0.5, 0.5, 0.5], step=3)
    b = _plan(4, sigma=[0.5, 0.5, 0.5, 0.5], step=4)
    c = _plan(4, sigma=[0.5, 0.5, 0.5, 0.5], step=3, seed=(1235, 0))
    first, again, other, reseeded = (_run(x, None, p)[0] for p in (a, a, b, c))
    assert first.tobytes() == again.tobytes()
    assert np.count_nonzero(first[..., :4] != other[..., :4]) > 0.99 * first[..., :4].size
    assert np.count_nonzero(first[..., :4] != reseeded[..., :4]) > 0.99 * first[..., :4].size
    assert first[..., 4:].tobytes() == other[..., 4:].tobytes()


def test_noise_statistics():
    from gts.augment import AugmentPlan

    shape = (20, 18, 14)
    x = np.zeros(shape + (4,), dtype=np.float32)
    plan = AugmentPlan((False,) * 3, np.ones(4), np.zeros(4), np.ones(4), 0.0, (1234, 0), 3)
    got, _ = _run(x, None, plan)
    ref = augment_ref.crop_noise(shape, 4, plan)
    print(f"mean {got.mean():.4f} std {got.std():.4f} over {got.size} draws (reference {ref.mean():.4f}, {ref.std():.4f})")
    assert abs(float(got.mean())) <= 0.02 and abs(float(got.std()) - 1.0) <= 0.02
    for c in range(4):
        assert abs(float(got[..., c].mean())) <= 0.05 and abs(float(got[..., c].std()) - 1.0) <= 0.05


@pytest.mark.parametrize("k", [4, 3, 1])
def test_flip_crop_is_an_involution_and_its_own_adjoint(k):
    from gts import ops

    dims = (5, 3, 7)
    rng = np.random.default_rng(k)
    u = torch.from_numpy(rng.integers(-8, 9, dims + (k,)).astype(np.float32)).to(DEV)
    w = torch.from_numpy(rng.integers(-8, 9, dims + (k,)).astype(np.float32)).to(DEV)
    for flips in FLIPS:
        fu = ops.flip_crop(u, dims, flips)
        assert fu.shape == u.shape
        assert np.array_equal(fu.cpu().numpy(), augment_ref.flip(u.cpu().numpy(), flips))
        assert torch.equal(ops.flip_crop(fu, dims, flips), u)
        rows = ops.flip_crop(u.reshape(-1, k), dims, flips)             # the [V, K] form
        assert rows.shape == (u.numel() // k, k) and torch.equal(rows.view(u.shape), fu)
        # <flip(u), w> == <u, flip(w)>, exactly: the values are small integers
        assert float((fu * w).sum()) == float((u * ops.flip_crop(w, dims, flips)).sum())


GRAPHS = [(1, 0, 130), (0,), (7,)]


@pytest.mark.parametrize("fm", [(20, 4), (5, 1)], ids=lambda p: f"F{p[0]}_M{p[1]}")
@pytest.mark.parametrize("sizes", GRAPHS, ids=lambda s: "-".join(map(str, s)))
def test_features(sizes, fm):
    from gts import ops
    from gts.augment import AugmentPlan

    n_feats, modalities = fm
    n = sum(sizes)
    rng = np.random.default_rng(n + n_feats)
    feats = rng.standard_normal((n, n_feats)).astype(np.float32)
    if n:
        feats[0, 0] = -0.0
    fd = torch.from_numpy(feats).to(DEV)
    for feature_sigma in (0.0, 0.5):
        plans = [_plan(modalities, rng=rng, feature_sigma=feature_sigma, seed=(77, 1), step=11) for _ in sizes]
        if len(plans) > 1:          # one graph left as it is
            plans[-1] = AugmentPlan((False,) * 3, np.ones(modalities), np.zeros(modalities), np.zeros(modalities),
                                    feature_sigma, (77, 1), 11)
        out = ops.augment_features(fd, torch.tensor(sizes, dtype=torch.int64), plans)
        assert out.shape == fd.shape and (n == 0 or out.data_ptr() != fd.data_ptr())
        assert fd.cpu().numpy().tobytes() == feats.tobytes()                 # the input is left alone
        base = augment_ref.features_no_noise(feats, list(sizes), plans)
        got = out.cpu().numpy()
        if feature_sigma == 0.0:
            assert got.tobytes() == base.astype(np.float32).tobytes()
            continue
        noise = augment_ref.features_noise(n, n_feats, plans[0])
        err = np.abs((got.astype(np.float64) - base.astype(np.float64)) - noise)
        if n:
            print(f"sizes {sizes} F {n_feats}: largest noise error / sigma {err.max() / feature_sigma:.3e}")
            assert err.max() <= 2e-5 * feature_sigma
            # the rows' stream is not the voxels': the same index and step give other values
            voxel_noise = augment_ref.normals(n, n_feats, plans[0].seed, plans[0].step, 0)
            assert np.abs(noise / feature_sigma - voxel_noise).max() > 0.1


def test_features_follow_their_graph():
    """Three graphs, each with its own scale: every row takes its owner's, the empty graph in between owns none."""
    from gts import ops
    from gts.augment import AugmentPlan

    sizes = (2, 0, 3)
    feats = np.ones((5, 20), dtype=np.float32)
    plans = [AugmentPlan((False,) * 3, np.full(4, s), np.zeros(4), np.zeros(4)) for s in (2.0, 3.0, 4.0)]
    out = ops.augment_features(torch.from_numpy(feats).to(DEV), sizes, plans).cpu().numpy()
    assert np.all(out[:2] == 2.0) and np.all(out[2:] == 4.0)
