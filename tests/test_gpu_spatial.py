"""The rotated / zoomed crop kernels (csrc/gts_augment.hip A3 / A4) against tests/spatial_ref.py on the
GPU.

A3 at sigma == 0 is bit-equal to the numpy reference: every product, sum and rounding of the definition is fixed
(float64 without fma, one rounding to float32, the float32 affine).  Its noise term is A1's and is held to A1's bound
(2e-5 sigma, derived in tests/test_gpu_augment.py).  A4 sums the same float64 terms as the reference's scatter-add in
another order and rounds once: one float32 ulp of the reference plus 2^-40 of the sum of the terms' magnitudes (a few
hundred float64 additions move a sum by far less than 2^-40 of that)."""
import itertools

import numpy as np
import pytest
import torch

from tests import augment_ref, spatial_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FLIPS = list(itertools.product((False, True), repeat=3))
ANGLES = (20.0, -15.0, 10.0)
ZOOMS = (1.25, 0.8)
# (crop, channels, image channels): the scalar path, the vector path over several workgroups, an extent of 1, three
# channel groups per voxel
CASES = [((5, 4, 3), 5, 2), ((17, 13, 9), 8, 4), ((7, 1, 6), 4, 1), ((33, 17, 9), 12, 4)]


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _plan(ci, matrix, flips=(False, False, False), sigma=None, seed=(1234, 0), step=3):
    from gts.augment import AugmentPlan

    rng = np.random.default_rng(ci)
    scale = rng.uniform(0.7, 1.3, ci).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, ci).astype(np.float32)
    if ci > 1:                              # one channel that is copied, not multiplied
        scale[1], shift[1] = 1.0, 0.0
    sigma = np.zeros(ci, dtype=np.float32) if sigma is None else np.asarray(sigma, dtype=np.float32)
    return AugmentPlan(flips, scale, shift, sigma, 0.0, seed, step, matrix)


def _sample(shape, channels, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape + (channels,)).astype(np.float32)
    labels = rng.integers(1, 5, shape).astype(np.int64)          # 0 is what the border gives: never an input label
    return x, labels


def _run(x, labels, plan, a3_directly=False):
    from gts import ops

    xd = torch.from_numpy(x).to(DEV) if x is not None else None
    ld = torch.from_numpy(labels).to(DEV) if labels is not None else None
    if a3_directly:         # the library's A3 whatever the matrix: augment_crop sends an identity matrix to A1
        params = torch.from_numpy(np.stack([plan.scale, plan.shift, plan.sigma], axis=1)).to(DEV)
        xo, lo = ops._crop_augment(xd, ld, x.shape[:3], plan.channels, params, plan.flip_mask, plan.seed64, plan.step,
                                   "A3", plan.matrix)
    else:
        xo, lo = ops.augment_crop(xd, ld, plan)
    if xd is not None:
        assert xo.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), torch.from_numpy(x))      # never in place
    return (xo.cpu().numpy() if xo is not None else None), (lo.cpu().numpy() if lo is not None else None)


def _bwd(dy, dims, plan):
    from gts import ops

    return ops.spatial_crop_bwd(torch.from_numpy(dy).to(DEV), dims, plan).cpu().numpy()


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------- A3 against the reference
@pytest.mark.parametrize("zoom", ZOOMS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + f"_C{c[1]}")
def test_resample_without_noise_is_bit_equal(case, zoom):
    shape, channels, ci = case
    x, labels = _sample(shape, channels, seed=sum(shape))
    matrix = spatial_ref.matrix_from(ANGLES, zoom)
    flips_here = FLIPS if shape == (17, 13, 9) else [FLIPS[0], FLIPS[5], FLIPS[7]]
    for flips in flips_here:
        plan = _plan(ci, matrix, flips)
        assert plan.spatial
        got_x, got_l = _run(x, labels.reshape(-1), plan)
        want_x, want_l = spatial_ref.resample(x, labels, plan)
        assert got_x.dtype == np.float32 and got_l.dtype == np.int64
        assert got_x.tobytes() == want_x.tobytes(), f"flips {flips}"
        assert np.array_equal(got_l, want_l.reshape(-1)), f"flips {flips}"
        # the transform did something and the border is in play
        assert np.any(want_l == 0) or zoom > 1
        assert not np.array_equal(want_l, augment_ref.flip(labels, flips))


def test_x_alone_and_labels_alone():
    x, labels = _sample((17, 13, 9), 8)
    plan = _plan(4, spatial_ref.matrix_from(ANGLES, 0.8), (True, False, True))
    want_x, want_l = spatial_ref.resample(x, labels, plan)
    got_x, none = _run(x, None, plan)
    assert none is None and got_x.tobytes() == want_x.tobytes()
    none, got_l = _run(None, labels, plan)
    assert none is None and got_l.shape == labels.shape and np.array_equal(got_l, want_l)
    both_x, both_l = _run(x, labels, plan)
    assert both_x.tobytes() == want_x.tobytes() and np.array_equal(both_l, want_l)


def test_noise_is_a1s_term_whatever_the_launch_shape():
    shape = (17, 13, 9)
    x, _ = _sample(shape, 8, seed=9)
    sigma = [0.5, 1.0, 0.0, 0.25]
    seed, step = (0xDEADBEEF, 0x1234), (7 << 32) | 5
    for zoom, flips in ((1.25, (False, False, False)), (0.8, (True, True, False))):
        matrix = spatial_ref.matrix_from(ANGLES, zoom)
        quiet = _plan(4, matrix, flips, seed=seed, step=step)
        noisy = _plan(4, matrix, flips, sigma=sigma, seed=seed, step=step)
        outs = {}
        for channels in (8, 5):
            xs = np.ascontiguousarray(x[..., :channels])
            base, _ = _run(xs, None, quiet)
            got, _ = _run(xs, None, noisy)
            assert base.tobytes() == spatial_ref.resample(xs, None, quiet)[0].tobytes()
            noise = augment_ref.crop_noise(shape, channels, noisy)
            err = np.abs((got.astype(np.float64) - base.astype(np.float64)) - noise)
            for c in range(channels):
                s = sigma[c] if c < 4 else 0.0
                if s == 0.0:        # nothing is drawn and nothing is added
                    assert got[..., c].tobytes() == np.ascontiguousarray(base[..., c]).tobytes()
                    continue
                print(f"zoom {zoom} C {channels} channel {c}: largest noise error / sigma {err[..., c].max() / s:.3e}")
                assert err[..., c].max() <= 2e-5 * s, f"channel {c}: {err[..., c].max():.3e}"
            outs[channels] = got
        # a value depends on (seed, step, output voxel, channel), not on how many channels the launch carries
        assert outs[8][..., :5].tobytes() == outs[5].tobytes()


# ---------------------------------------------------------------- A3 without the reference
QUARTER_TURNS = [
    (np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), 3, (0, 1)),
    (np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]]), 1, (0, 1)),
    (np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]), 3, (1, 2)),
    (np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0.0]]), 3, (2, 0)),
]


def test_quarter_turns_equal_torch_rot90():
    x, labels = _sample((5, 5, 5), 4, seed=5)
    for matrix, k, dims in QUARTER_TURNS:
        plan = _plan(0, matrix)
        got_x, got_l = _run(x, labels, plan)
        assert np.array_equal(got_x, torch.rot90(torch.from_numpy(x), k, dims).numpy())
        assert np.array_equal(got_l, torch.rot90(torch.from_numpy(labels), k, dims).numpy())


@pytest.mark.parametrize("layout", [(8, 4), (5, 3)], ids=lambda l: f"C{l[0]}_Ci{l[1]}")
def test_identity_matrix_through_a3_equals_a1(layout):
    channels, ci = layout
    x, labels = _sample((5, 3, 7), channels, seed=2)
    sigma = [0.5, 0.0, 0.25, 0.0][:ci]
    for flips in (FLIPS[0], FLIPS[3], FLIPS[7]):
        plan = _plan(ci, np.eye(3), flips, sigma=sigma)
        assert not plan.spatial
        a1_x, a1_l = _run(x, labels, plan)
        a3_x, a3_l = _run(x, labels.reshape(-1), plan, a3_directly=True)
        assert np.array_equal(a1_x, a3_x) and np.array_equal(a1_l.reshape(-1), a3_l)          # ==: the sign of a zero aside


def test_ramp_is_reproduced_at_interior_voxels():
    """On x = alpha i + beta j + gamma k + delta the trilinear lerp is exact in real arithmetic wherever all eight
    corners are inside: only the float64 roundings of the lerp and the one rounding to float32 remain."""
    shape = (17, 13, 9)
    coeffs = np.array([[0.5, -1.25, 2.0, 3.0], [-2.0, 0.75, 0.25, -1.0], [1.0, 1.0, 1.0, 0.0], [0.0, 0.0, -3.5, 40.0]])
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    ramp = np.stack([c[0] * i + c[1] * j + c[2] * k + c[3] for c in coeffs], axis=-1)
    x = ramp.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), ramp)            # multiples of 1 / 4: exact in float32
    plan = _plan(0, spatial_ref.matrix_from(ANGLES, 1.25))
    got, _ = _run(x, None, plan)
    p, _ = spatial_ref.source_points(shape, plan)
    f = np.floor(p)
    interior = np.all((f >= 0) & (f + 1 <= np.asarray(shape) - 1), axis=-1)
    print(f"interior share {interior.mean():.3f}")
    assert interior.mean() >= 0.85
    for c, (alpha, beta, gamma, delta) in enumerate(coeffs):
        want = alpha * p[..., 0] + beta * p[..., 1] + gamma * p[..., 2] + delta
        tol = _ulp32(want) + 1e-12 * (abs(alpha) + abs(beta) + abs(gamma)) * max(shape)
        err = np.abs(got[..., c].astype(np.float64) - want)
        print(f"ramp {c}: largest error / tolerance {(err / tol)[interior].max():.3f}")
        assert np.all(err[interior] <= tol[interior])


# ---------------------------------------------------------------- A4
def test_adjoint_of_basis_volumes_is_the_transpose_of_the_resample():
    dims, v = (5, 4, 3), 60
    eye = np.eye(v, dtype=np.float32).reshape(dims + (v,))
    for zoom, flips in ((1.25, FLIPS[0]), (0.8, FLIPS[6])):
        plan = _plan(0, spatial_ref.matrix_from(ANGLES, zoom), flips)
        forward, _ = _run(eye, None, plan)                       # [o, q]
        back = _bwd(eye, dims, plan)                             # [q, o]
        w, wt = forward.reshape(v, v).astype(np.float64), back.reshape(v, v).astype(np.float64).T
        assert np.count_nonzero(w) > v                           # several corners per output
        assert np.array_equal(w != 0, wt != 0)
        assert np.all(np.abs(w - wt) <= np.maximum(_ulp32(w), _ulp32(wt)))


@pytest.mark.parametrize("k", [4, 5])
def test_adjoint_against_the_reference(k):
    dims = (17, 13, 9)
    rng = np.random.default_rng(k)
    dy = rng.standard_normal(dims + (k,)).astype(np.float32)
    worst = 0.0
    for n, flips in enumerate(FLIPS):
        plan = _plan(0, spatial_ref.matrix_from(ANGLES, ZOOMS[n % 2]), flips)
        got = _bwd(dy, dims, plan)
        want, mass = spatial_ref.adjoint_terms(dy, dims, plan)
        tol = _ulp32(want) + 2.0 ** -40 * mass
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert got.shape == dy.shape and np.all(err <= tol), f"flips {flips}"
        assert np.count_nonzero(want) > 0.5 * want.size
    print(f"K = {k}: largest error / tolerance {worst:.3f}")


@pytest.mark.parametrize("case", [((7, 1, 6), spatial_ref.matrix_from((25.0, 0.0, 0.0), 1.0)),     # out of the plane
                                  ((9, 8, 7), np.eye(3) / 3.0),               # h = 3: boxes of up to 9^3 candidates
                                  ((6, 5, 4), spatial_ref.matrix_from(ANGLES, 1.0) * 2.5)],        # h < 1: sparse
                         ids=["extent1", "zoom3", "shrink"])
def test_adjoint_at_the_edges_of_its_box(case):
    dims, matrix = case
    rng = np.random.default_rng(sum(dims))
    dy = rng.standard_normal(dims + (4,)).astype(np.float32)
    plan = _plan(0, matrix, (False, True, False))
    got = _bwd(dy.reshape(-1, 4), dims, plan)                    # the [V, K] form
    assert got.shape == (int(np.prod(dims)), 4)
    want, mass = spatial_ref.adjoint_terms(dy, dims, plan)
    err = np.abs(got.reshape(dims + (4,)).astype(np.float64) - want)
    assert np.all(err <= _ulp32(want) + 2.0 ** -40 * mass)
    assert np.any(want != 0)
    # <A x, dy> == <x, A^T dy> with the GPU's forward and backward: every entry of A x and of A^T dy carries one
    # float32 rounding (2^-24 relative) on top of float64 work, doubled here
    x = rng.standard_normal(dims + (4,)).astype(np.float32)
    ax, _ = _run(x, None, plan)
    lhs = float((ax.astype(np.float64) * dy).sum())
    rhs = float((x.astype(np.float64) * got.reshape(dims + (4,))).sum())
    mass = float(np.abs(ax.astype(np.float64) * dy).sum() + np.abs(x.astype(np.float64) * got.reshape(x.shape)).sum())
    assert abs(lhs - rhs) <= 2.0 ** -23 * mass


def test_adjoint_is_deterministic():
    dims = (17, 13, 9)
    dy = np.random.default_rng(1).standard_normal(dims + (4,)).astype(np.float32)
    plan = _plan(0, spatial_ref.matrix_from(ANGLES, 0.8), (True, False, False))
    assert _bwd(dy, dims, plan).tobytes() == _bwd(dy, dims, plan).tobytes()


def test_spatial_crop_bwd_of_a_plain_plan_is_flip_crop():
    from gts import ops

    dims = (5, 3, 7)
    t = torch.from_numpy(np.random.default_rng(2).standard_normal(dims + (5,)).astype(np.float32)).to(DEV)
    for flips in FLIPS:
        plan = _plan(0, np.eye(3), flips)
        got = ops.spatial_crop_bwd(t, dims, plan)
        want = ops.flip_crop(t, dims, flips)
        assert got.shape == want.shape and got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
