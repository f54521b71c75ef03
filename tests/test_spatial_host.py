"""Host side of the rotated / zoomed crops (gts/augment.py): the plan's matrix and the second generator's
draws, the numpy reference against np.rot90 and against its own transpose, the command-line flags and the library's
argument errors.  No GPU."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import spatial_ref


def _plan(matrix, flips=(False, False, False), channels=0):
    from gts.augment import AugmentPlan

    return AugmentPlan(flips, np.ones(channels), np.zeros(channels), np.zeros(channels), matrix=matrix)


# ---------------------------------------------------------------- plan and augmenter
def test_plan_matrix_field_and_spatial_property():
    from gts.augment import AugmentPlan

    plain = AugmentPlan.identity(4)
    assert plain.matrix.dtype == np.float64 and np.array_equal(plain.matrix, np.eye(3))
    assert not plain.spatial and plain.is_identity
    turned = AugmentPlan(matrix=spatial_ref.matrix_from((10, 0, 0), 1.0))
    assert turned.spatial and not turned.is_identity
    zoomed = AugmentPlan(matrix=np.eye(3) / 1.1)
    assert zoomed.spatial and not zoomed.is_identity
    # the positional constructor of before: seven fields, the matrix stays the identity
    old = AugmentPlan((True, False, False), np.ones(4), np.zeros(4), np.zeros(4), 0.0, (1, 2), 3)
    assert not old.spatial and old.flip_mask == 1 and old.step == 3
    last = AugmentPlan((True, False, False), np.ones(4), np.zeros(4), np.zeros(4), 0.0, (1, 2), 3, 2 * np.eye(3))
    assert last.spatial and np.array_equal(last.matrix, 2 * np.eye(3))


def test_bad_matrices_raise():
    from gts.augment import AugmentPlan

    nan = np.eye(3)
    nan[1, 2] = np.nan
    inf = np.eye(3)
    inf[0, 0] = np.inf
    for matrix in (np.eye(4), np.ones(9), nan, inf, np.zeros((3, 3)), np.array([[1, 2, 3], [1, 2, 3], [0, 0, 1.0]])):
        with pytest.raises(ValueError):
            AugmentPlan(matrix=matrix)


@pytest.mark.parametrize("kwargs", [dict(rotate=-1.0), dict(rotate=180.5), dict(zoom=1.0), dict(zoom=-0.1),
                                    dict(zoom=float("nan")), dict(rotate=float("nan")), dict(spatial_prob=1.5),
                                    dict(spatial_prob=-0.1)])
def test_bad_augmenter_arguments_raise(kwargs):
    from gts.augment import Augmenter

    with pytest.raises(ValueError):
        Augmenter(0, **kwargs)


def test_second_generator_replays_from_numpy_and_leaves_the_first_alone():
    from gts.augment import Augmenter

    seed = 11
    aug = Augmenter(seed, rotate=25.0, zoom=0.2, spatial_prob=0.6)
    old = Augmenter(seed)
    rng2 = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(1,)))
    spatial = 0
    for _ in range(40):
        plan, before = aug.draw(), old.draw()
        u = rng2.random()
        angles = rng2.uniform(-25.0, 25.0, 3)
        s = rng2.uniform(0.8, 1.2)
        want = spatial_ref.matrix_from(angles, s) if u < 0.6 else np.eye(3)
        assert plan.matrix.tobytes() == want.tobytes()
        assert plan.spatial == bool(u < 0.6)
        spatial += plan.spatial
        assert plan.flips == before.flips and plan.step == before.step and plan.seed == before.seed
        for name in ("scale", "shift", "sigma"):
            assert getattr(plan, name).tobytes() == getattr(before, name).tobytes()
        if plan.spatial:
            gram = plan.matrix.dot(plan.matrix.T) * s * s
            assert np.abs(gram - np.eye(3)).max() <= 1e-15
    assert 10 < spatial < 35


def test_without_rotation_and_zoom_every_plan_is_the_plan_of_before():
    from gts.augment import Augmenter

    new = Augmenter(5, rotate=0.0, zoom=0.0, spatial_prob=1.0)
    old = Augmenter(5)
    for _ in range(30):
        p, q = new.draw(), old.draw()
        assert p.matrix.tobytes() == np.eye(3).tobytes() and not p.spatial
        assert q.matrix.tobytes() == np.eye(3).tobytes()
        assert p.flips == q.flips
        for name in ("scale", "shift", "sigma"):
            assert getattr(p, name).tobytes() == getattr(q, name).tobytes()


def test_spatial_probabilities_0_and_1_are_exact():
    from gts.augment import Augmenter

    never = Augmenter(2, rotate=30.0, zoom=0.2, spatial_prob=0.0)
    always = Augmenter(2, rotate=30.0, zoom=0.2, spatial_prob=1.0)
    zoom_only = Augmenter(2, zoom=0.2, spatial_prob=1.0)
    for _ in range(200):
        assert not never.draw().spatial
        assert always.draw().spatial
        m = zoom_only.draw().matrix
        assert m[0, 0] == m[1, 1] == m[2, 2] and np.count_nonzero(m) == 3 and 1 / 1.2 <= m[0, 0] <= 1 / 0.8


def test_describe_names_the_spatial_settings_only_when_on():
    from gts.augment import Augmenter

    assert "rotation" not in Augmenter(1).describe() and "zoom" not in Augmenter(1).describe()
    text = Augmenter(1, rotate=15.0, zoom=0.1, spatial_prob=0.25).describe()
    assert "rotation +- 15.0" in text and "zoom 1 +- 0.1" in text and "0.25" in text
    assert text.startswith(Augmenter(1).describe())


# ---------------------------------------------------------------- the reference against itself
QUARTER_TURNS = [
    # (matrix with exact 0 / +-1 entries, the np.rot90 call that equals it: k, axes)
    # out[i, j] = x[n - 1 - j, i] is np.rot90(x, 3): the matrix maps OUTPUT offsets to source offsets
    (np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), 3, (0, 1)),
    (np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]]), 1, (0, 1)),
    (np.array([[-1, 0, 0], [0, -1, 0], [0, 0, 1.0]]), 2, (0, 1)),
    (np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]), 3, (1, 2)),
    (np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0.0]]), 3, (2, 0)),
]


@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("turn", range(len(QUARTER_TURNS)))
def test_reference_quarter_turns_equal_rot90(turn, n):
    matrix, k, axes = QUARTER_TURNS[turn]
    rng = np.random.default_rng(n + turn)
    x = rng.standard_normal((n, n, n, 3)).astype(np.float32)
    labels = rng.integers(0, 4, (n, n, n)).astype(np.int64)
    got_x, got_l = spatial_ref.resample(x, labels, _plan(matrix))
    assert got_x.tobytes() == np.ascontiguousarray(np.rot90(x, k, axes)).tobytes()
    assert np.array_equal(got_l, np.rot90(labels, k, axes))
    # the half turn is two mirrors: the plan's flips give the same volume
    if turn == 2:
        flipped, flipped_l = spatial_ref.resample(x, labels, _plan(np.eye(3), flips=(True, True, False)))
        assert flipped.tobytes() == got_x.tobytes() and np.array_equal(flipped_l, got_l)


def _dense(dims, plan):
    """W [V, V]: row o, column q, the resample as a matrix (basis volumes as channels)."""
    v = int(np.prod(dims))
    basis = np.eye(v, dtype=np.float32).reshape(dims + (v,))
    p, _ = spatial_ref.source_points(dims, plan)
    f = np.floor(p)
    t = p - f
    # in float64, without the float32 rounding: the same lerp on the basis
    out = np.zeros((v, v))
    flat = lambda q: (q[..., 0] * dims[1] + q[..., 1]) * dims[2] + q[..., 2]
    for corner in np.ndindex(2, 2, 2):
        q = f.astype(np.int64) + np.array(corner)
        w = np.ones(dims)
        for a in range(3):
            w = w * (t[..., a] if corner[a] else 1.0 - t[..., a])
        inside = np.all((q >= 0) & (q < np.asarray(dims)), axis=-1)
        rows = np.arange(v).reshape(dims)[inside]
        np.add.at(out, (rows, flat(q)[inside]), w[inside])
    return out, spatial_ref.resample_values(basis, plan).reshape(v, v)


@pytest.mark.parametrize("flips", [(False, False, False), (True, False, True)])
def test_reference_adjoint_is_the_transpose_of_the_resample(flips):
    dims = (5, 4, 3)
    v = 60
    plan = _plan(spatial_ref.matrix_from((20, -15, 10), 1.25), flips)
    weights, lerped = _dense(dims, plan)
    # the lerp form and the product-of-weights form are the same real numbers
    assert np.abs(lerped.astype(np.float64) - weights).max() <= 2.0 ** -23
    assert 0.3 * v < weights.sum() <= v + 1e-9          # a zoom in: most outputs keep all their corners
    dy = np.eye(v).reshape(dims + (v,))
    back = spatial_ref.adjoint(dy, dims, plan).reshape(v, v)         # [q, o]
    assert np.abs(back - weights.T).max() <= 1e-15
    rng = np.random.default_rng(3)
    dy = rng.standard_normal(dims + (4,))
    x = rng.standard_normal(dims + (4,))
    lhs = float((weights.dot(x.reshape(v, 4)) * dy.reshape(v, 4)).sum())
    rhs = float((x * spatial_ref.adjoint(dy, dims, plan)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_reference_zero_border_and_tie_rule_at_an_exact_zoom_of_2():
    """M = I / 2 on an even extent: d = o - c is a half-integer, p = c + d / 2 falls on quarters; on an extent of 5 the
    sources of odd o fall on half-integers, where floor(p + 0.5) rounds the tie UP."""
    n = 5
    plan = _plan(np.eye(3) / 2.0)
    labels = np.zeros((n, 1, 1), dtype=np.int64)
    labels[:, 0, 0] = np.arange(10, 10 + n)
    x = labels.astype(np.float32)[..., None]
    # extent 1 on y and z: c = 0, d = 0, p = 0 exactly
    got_x, got_l = spatial_ref.resample(x, labels, plan)
    p = 2.0 + (np.arange(n) - 2.0) / 2.0                             # 1, 1.5, 2, 2.5, 3
    assert np.array_equal(got_l[:, 0, 0], 10 + np.floor(p + 0.5).astype(np.int64))
    assert list(got_l[:, 0, 0]) == [11, 12, 12, 13, 13]
    assert np.array_equal(got_x[:, 0, 0, 0], (10 + p).astype(np.float32))
    # zoom 1 / 2 (M = 2 I): the outer outputs look outside the crop: p = -2, 0, 2, 4, 6
    out_x, out_l = spatial_ref.resample(x, labels, _plan(2.0 * np.eye(3)))
    assert list(out_l[:, 0, 0]) == [0, 10, 12, 14, 0]
    assert list(out_x[:, 0, 0, 0]) == [0.0, 10.0, 12.0, 14.0, 0.0]
    # a source half a voxel outside: half of the edge value (the border is 0.0, not the edge)
    shifted = _plan(np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1]]) * 1.25)
    edge_x, edge_l = spatial_ref.resample(x, labels, shifted)          # p = -0.5, 0.75, 2, 3.25, 4.5
    assert edge_x[0, 0, 0, 0] == np.float32(0.5 * 10) and edge_x[4, 0, 0, 0] == np.float32(0.5 * 14)
    assert edge_l[0, 0, 0] == 10 and edge_l[4, 0, 0] == 0              # floor(0) = 0 inside, floor(5) = 5 outside


# ---------------------------------------------------------------- command line
def test_cli_flags_default_off_and_reach_the_augmenter():
    from gts.augment import add_augment_arguments, augmenter_from_args
    from scripts import train_gnn, train_joint, train_refinement_cnn

    parser = argparse.ArgumentParser()
    add_augment_arguments(parser)
    args = parser.parse_args(["--augment"])
    assert (args.aug_rotate, args.aug_zoom, args.aug_spatial_prob) == (0, 0, 0.5)
    aug = augmenter_from_args(args)
    assert (aug.rotate, aug.zoom, aug.spatial_prob) == (0.0, 0.0, 0.5)
    assert not any(aug.draw().spatial for _ in range(20))
    args = parser.parse_args(["--augment", "--aug_rotate", "15", "--aug_zoom", "0.1", "--aug_spatial_prob", "1"])
    aug = augmenter_from_args(args, rank=1)
    assert (aug.seed, aug.rotate, aug.zoom, aug.spatial_prob) == (1, 15.0, 0.1, 1.0)
    assert all(aug.draw().spatial for _ in range(20)) and "rotation" in aug.describe()
    gnn = augmenter_from_args(args, features_only=True)
    assert (gnn.rotate, gnn.zoom) == (0.0, 0.0) and not any(gnn.draw().spatial for _ in range(20))
    for cli in (train_refinement_cnn, train_joint, train_gnn):
        got = cli.build_cli_parser().parse_args(["-r", "run"])
        assert (got.aug_rotate, got.aug_zoom, got.aug_spatial_prob) == (0, 0, 0.5)
        got = cli.build_cli_parser().parse_args(["-r", "run", "--augment", "--aug_rotate", "20", "--aug_zoom", "0.2",
                                                 "--aug_spatial_prob", "0.75"])
        assert (got.aug_rotate, got.aug_zoom, got.aug_spatial_prob) == (20.0, 0.2, 0.75)
    def helps(cli):
        return {a.dest: a.help for a in cli.build_cli_parser()._actions}

    for dest in ("aug_rotate", "aug_zoom", "aug_spatial_prob"):
        assert "ignored" in helps(train_gnn)[dest] and "ignored" not in helps(train_joint)[dest]
    assert "ignored" in train_gnn.build_cli_parser().format_help()


# ---------------------------------------------------------------- the library without a GPU
def test_library_argument_errors_need_no_gpu(hip_lib):
    one = ctypes.c_void_p(16)
    fwd, bwd = hip_lib.gts_augment_spatial_f32, hip_lib.gts_augment_spatial_bwd_f32

    def mat(values):
        return (ctypes.c_double * 9)(*np.asarray(values, dtype=np.float64).reshape(-1))

    eye = mat(np.eye(3))
    turned = mat(spatial_ref.matrix_from((20, -15, 10), 1.25))
    singular = mat([[1, 2, 3], [1, 2, 3], [0, 0, 1]])
    zero = mat(np.zeros((3, 3)))
    nan = mat([[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]])
    inf = mat([[float("inf"), 0, 0], [0, 1, 0], [0, 0, 1]])
    far = mat(np.eye(3) / 3.0)              # M^-1 = 3 I: h = 3, legal
    too_far = mat(np.eye(3) / 8.5)          # h = 8.5
    # A3
    assert fwd(None, None, None, eye, None, None, 2, 2, 2, 4, 0, 0, 0, 0, None) == -1        # nothing to do
    assert fwd(one, None, None, eye, None, None, 2, 2, 2, 4, 0, 0, 0, 0, None) == -1         # x without its output
    assert fwd(None, one, None, eye, None, None, 2, 2, 2, 0, 0, 0, 0, 0, None) == -1         # labels without theirs
    assert fwd(one, None, None, None, one, None, 2, 2, 2, 4, 0, 0, 0, 0, None) == -1         # no matrix
    assert fwd(one, None, None, eye, one, None, 2, 2, 2, 4, 2, 0, 0, 0, None) == -1          # image channels, no params
    assert fwd(one, None, one, eye, one, None, 2, 2, 2, 4, 5, 0, 0, 0, None) == -2           # Ci > C
    assert fwd(one, None, one, eye, one, None, -1, 2, 2, 4, 2, 0, 0, 0, None) == -2          # negative extent
    assert fwd(one, None, one, eye, one, None, 2, 2, 2, 513, 2, 0, 0, 0, None) == -2         # too many channels
    assert fwd(one, None, one, eye, one, None, 1 << 30, 1 << 20, 1 << 10, 4, 2, 0, 0, 0, None) == -2
    assert fwd(None, one, None, eye, None, one, 2, 2, 2, 0, 2, 0, 0, 0, None) == -2          # image channels without x
    assert fwd(one, None, one, eye, one, None, 2, 2, 2, 4, 2, 8, 0, 0, None) == -3           # a fourth axis
    assert fwd(one, None, one, eye, one, None, 2, 2, 2, 4, 2, -1, 0, 0, None) == -3
    for bad in (singular, zero, nan, inf, too_far):
        assert fwd(one, None, one, bad, one, None, 2, 2, 2, 4, 2, 0, 0, 0, None) == -3
        assert bwd(one, bad, one, 2, 2, 2, 4, 0, None) == -3
    for good in (eye, turned, far):
        assert fwd(one, None, one, good, one, None, 0, 2, 2, 4, 2, 0, 0, 0, None) == 0       # no voxels: no launch
        assert fwd(None, one, None, good, None, one, 2, 0, 2, 0, 0, 5, 0, 0, None) == 0
        assert bwd(one, good, one, 2, 2, 0, 4, 7, None) == 0
    # A4
    assert bwd(None, eye, one, 2, 2, 2, 4, 0, None) == -1
    assert bwd(one, None, one, 2, 2, 2, 4, 0, None) == -1
    assert bwd(one, eye, None, 2, 2, 2, 4, 0, None) == -1
    assert bwd(one, eye, one, 2, -2, 2, 4, 0, None) == -2
    assert bwd(one, eye, one, 2, 2, 2, 0, 0, None) == -2
    assert bwd(one, eye, one, 2, 2, 2, 513, 0, None) == -2
    assert bwd(one, eye, one, 1 << 30, 1 << 20, 1 << 10, 4, 0, None) == -2
    assert bwd(one, eye, one, 2, 2, 2, 4, 8, None) == -3
    assert bwd(one, eye, one, 2, 2, 2, 4, -1, None) == -3


def test_ops_exports_and_cpu_refusals(hip_lib):
    import torch

    import gts
    from gts import ops
    from gts.augment import AugmentPlan

    plan = AugmentPlan(matrix=spatial_ref.matrix_from((20, -15, 10), 1.25))
    with pytest.raises(gts.GtsError, match="MI355X only"):
        ops.augment_crop(torch.zeros(2, 2, 2, 8), None, plan)
    with pytest.raises(gts.GtsError, match="MI355X only"):
        ops.spatial_crop_bwd(torch.zeros(8, 4), (2, 2, 2), plan)
    with pytest.raises(gts.GtsError, match="expected"):
        ops.spatial_crop_bwd(torch.zeros(9, 4), (2, 2, 2), plan)
    with pytest.raises(gts.GtsError, match="fp32"):
        ops.spatial_crop_bwd(torch.zeros(8, 4, dtype=torch.float64), (2, 2, 2), plan)
