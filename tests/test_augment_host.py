"""Host side of the training-time augmentation (gts/augment.py): the reference generator against the
Random123 known answers, the plan draws, the quantile-feature identity the design rests on, the command-line flags
and the library's argument errors.  No GPU."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import augment_ref


def _words(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter, key, want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_reference_philox_reproduces_the_random123_known_answers(counter, key, want):
    got = augment_ref.philox4x32_10(np.array(_words(counter), dtype=np.uint32), _words(key))
    assert [int(w) for w in got] == _words(want)


def test_reference_normals_use_the_documented_words():
    words = np.array([[0, 0, 0xFFFFFFFF, 0x40000000]], dtype=np.uint32)
    n = augment_ref.normals_from_words(words)[0]
    r0 = np.sqrt(-2 * np.log(2.0 ** -24))           # u = (0 + 1) 2^-24, theta = 0
    assert abs(n[0] - r0) < 1e-12 and n[1] == 0
    assert n[2] == 0 and n[3] == 0                   # u = 1: r = 0
    assert 5.76 < r0 < 5.77                          # the largest radius there is


def test_same_seed_same_plans_and_step_counts_draws():
    from gts.augment import Augmenter

    a, b, c = Augmenter(7), Augmenter(7), Augmenter(8)
    different = False
    for i in range(20):
        p, q, r = a.draw(), b.draw(), c.draw()
        assert p.step == q.step == i and p.seed == (7, 0)
        assert p.flips == q.flips and p.feature_sigma == q.feature_sigma
        for name in ("scale", "shift", "sigma"):
            assert getattr(p, name).tobytes() == getattr(q, name).tobytes()
            assert getattr(p, name).dtype == np.float32
        different = different or p.scale.tobytes() != r.scale.tobytes()
    assert different
    big = Augmenter((5 << 32) | 9).draw()
    assert big.seed == (9, 5) and big.seed64 == (5 << 32) | 9


def test_draw_order_can_be_replayed_from_numpy():
    from gts.augment import Augmenter

    aug = Augmenter(11, channels=3, flip_axes="xz", flip_prob=0.3, scale=0.2, shift=0.4, noise_prob=0.6, noise_sigma=0.5)
    rng = np.random.default_rng(11)
    for _ in range(5):
        plan = aug.draw()
        u = rng.random(3)
        scale = rng.uniform(0.8, 1.2, 3)
        shift = rng.uniform(-0.4, 0.4, 3)
        noisy = rng.random(3) < 0.6
        sigma = np.where(noisy, rng.uniform(0.0, 0.5, 3), 0.0)
        assert plan.flips == (bool(u[0] < 0.3), False, bool(u[2] < 0.3))
        assert plan.scale.tobytes() == scale.astype(np.float32).tobytes()
        assert plan.shift.tobytes() == shift.astype(np.float32).tobytes()
        assert plan.sigma.tobytes() == sigma.astype(np.float32).tobytes()


def test_every_parameter_lies_in_its_range():
    from gts.augment import Augmenter

    aug = Augmenter(1, channels=4, flip_axes="y", flip_prob=0.5, scale=0.25, shift=0.3, noise_prob=0.5, noise_sigma=0.2,
                    feature_noise_sigma=0.05)
    flipped = noisy = quiet = 0
    for _ in range(1000):
        p = aug.draw()
        assert not p.flips[0] and not p.flips[2]            # axes that are not named never flip
        flipped += p.flips[1]
        assert np.all(p.scale >= np.float32(0.75)) and np.all(p.scale <= np.float32(1.25))
        assert np.all(np.abs(p.shift) <= np.float32(0.3))
        assert np.all(p.sigma >= 0) and np.all(p.sigma <= np.float32(0.2))
        noisy += int(np.count_nonzero(p.sigma))
        quiet += int(np.count_nonzero(p.sigma == 0))
        assert p.feature_sigma == 0.05 and p.channels == 4 and not p.is_identity
    assert 400 < flipped < 600 and 1700 < noisy < 2300 and noisy + quiet == 4000


def test_flip_probabilities_0_and_1_are_exact():
    from gts.augment import Augmenter

    never, always = Augmenter(2, flip_prob=0.0), Augmenter(2, flip_prob=1.0, flip_axes="xy")
    for _ in range(200):
        assert never.draw().flips == (False, False, False)
        assert always.draw().flips == (True, True, False)
    off = Augmenter(3, flip_prob=0.0, scale=0.0, shift=0.0, noise_sigma=0.0)
    assert all(off.draw().is_identity for _ in range(50))


def test_identity_plan():
    from gts.augment import AugmentPlan

    plan = AugmentPlan.identity(3)
    assert plan.is_identity and plan.channels == 3 and plan.flip_mask == 0
    assert not AugmentPlan(flips=(False, True, False)).is_identity
    assert AugmentPlan(flips=(True, False, True)).flip_mask == 5
    assert not AugmentPlan(shift=np.array([0, 0, 0, 1e-3])).is_identity
    assert not AugmentPlan(feature_sigma=0.1).is_identity


@pytest.mark.parametrize("kwargs", [
    dict(scale=1.0), dict(scale=-0.1), dict(flip_prob=1.5), dict(flip_prob=-0.1), dict(noise_prob=2.0),
    dict(noise_sigma=-1.0), dict(feature_noise_sigma=-0.5), dict(shift=-0.1), dict(flip_axes="xw"),
    dict(channels=0), dict(seed=-1), dict(shift=float("nan")),
])
def test_bad_arguments_raise(kwargs):
    from gts.augment import Augmenter

    kwargs = dict(dict(seed=0), **kwargs)
    with pytest.raises(ValueError):
        Augmenter(**kwargs)


def test_bad_plans_raise():
    from gts.augment import AugmentPlan

    for kwargs in (dict(scale=np.array([1, 0, 1, 1.0])), dict(sigma=np.array([0, -1, 0, 0.0])),
                   dict(scale=np.ones(3)), dict(flips=(True, False)), dict(seed=(1 << 32, 0)), dict(step=-1)):
        with pytest.raises(ValueError):
            AugmentPlan(**kwargs)


def test_draw_leaves_torch_random_state_alone():
    import torch

    from gts.augment import Augmenter

    torch.manual_seed(5)
    before = torch.random.get_rng_state().clone()
    aug = Augmenter(5)
    for _ in range(10):
        aug.draw()
    assert torch.equal(before, torch.random.get_rng_state())


def test_affine_on_quantile_features_is_the_feature_of_the_mapped_intensities():
    """Columns 5 m .. 5 m + 4 of the 20 node features are the quantiles (0.1, 0.25, 0.5, 0.75, 0.9) of modality m over
    the supervoxel: mapping the intensities by a * v + b (a > 0) maps exactly those columns by the same a, b."""
    from gts.augment import Augmenter

    quantiles = [0.1, 0.25, 0.5, 0.75, 0.9]
    rng = np.random.default_rng(0)
    aug = Augmenter(4, scale=0.3, shift=0.5)
    sizes, plans = [3, 0, 4], [aug.draw() for _ in range(3)]
    supervoxels = [rng.standard_normal((int(rng.integers(1, 60)), 4)) for _ in range(sum(sizes))]

    def features(voxels):       # [n, 4] intensities -> the 20 features, modality-major
        return np.quantile(voxels, quantiles, axis=0).T.reshape(-1)

    feats = np.stack([features(v) for v in supervoxels])
    a, b = augment_ref.feature_params(sizes, plans, 20)
    a, b = a.astype(np.float64), b.astype(np.float64)
    owner = np.repeat(np.arange(3), sizes)
    for r, voxels in enumerate(supervoxels):
        p = plans[owner[r]]
        mapped = voxels * p.scale.astype(np.float64) + p.shift.astype(np.float64)
        assert np.abs(features(mapped) - (feats[r] * a[r] + b[r])).max() <= 1e-12
    # the modality <-> column map: column 5 m + j takes modality m's parameters
    for m in range(4):
        assert np.all(a[0, 5 * m:5 * m + 5] == np.float64(plans[0].scale[m]))
        assert np.all(b[-1, 5 * m:5 * m + 5] == np.float64(plans[2].shift[m]))


def test_cli_helper_parses_its_flags_and_builds_nothing_without_augment():
    from gts.augment import add_augment_arguments, augmenter_from_args
    from scripts import train_gnn, train_joint, train_refinement_cnn

    parser = argparse.ArgumentParser()
    add_augment_arguments(parser)
    args = parser.parse_args([])
    assert (args.augment, args.aug_flip_axes, args.aug_flip_prob, args.aug_scale, args.aug_shift, args.aug_noise,
            args.aug_noise_prob, args.aug_seed) == (False, "xyz", 0.5, 0.1, 0.1, 0.1, 0.5, 0)
    assert augmenter_from_args(args) is None
    args = parser.parse_args(["--augment", "--aug_flip_axes", "xy", "--aug_flip_prob", "0.25", "--aug_scale", "0.2",
                              "--aug_shift", "0.3", "--aug_noise", "0.05", "--aug_noise_prob", "0.75", "--aug_seed", "12"])
    aug = augmenter_from_args(args, rank=2)
    assert (aug.seed, aug.flip_axes, aug.flip_prob, aug.scale, aug.shift, aug.noise_sigma, aug.noise_prob) == \
        (14, "xy", 0.25, 0.2, 0.3, 0.05, 0.75)
    assert "seed 14" in aug.describe()
    gnn = augmenter_from_args(args, features_only=True)
    assert gnn.flip_axes == "" and gnn.noise_sigma == 0.0 and (gnn.scale, gnn.shift) == (0.2, 0.3)
    assert all(p.flips == (False, False, False) and not np.any(p.sigma) for p in (gnn.draw() for _ in range(20)))
    for cli, required in ((train_refinement_cnn, ["-r", "run"]), (train_joint, ["-r", "run"]), (train_gnn, ["-r", "run"])):
        assert cli.build_cli_parser().parse_args(required).augment is False
        assert cli.build_cli_parser().parse_args(required + ["--augment", "--aug_seed", "3"]).aug_seed == 3
    assert "ignored" in train_gnn.build_cli_parser().format_help()


def test_library_argument_errors_need_no_gpu(hip_lib):
    one = ctypes.c_void_p(16)
    crop, feats = hip_lib.gts_augment_crop_f32, hip_lib.gts_augment_features_f32
    assert crop(None, None, None, None, None, 2, 2, 2, 4, 0, 0, 0, 0, None) == -1          # nothing to do
    assert crop(one, None, None, None, None, 2, 2, 2, 4, 0, 0, 0, 0, None) == -1           # x without its output
    assert crop(None, one, None, None, None, 2, 2, 2, 0, 0, 0, 0, 0, None) == -1           # labels without theirs
    assert crop(one, None, None, one, None, 2, 2, 2, 4, 2, 0, 0, 0, None) == -1            # image channels, no params
    assert crop(one, None, one, one, None, 2, 2, 2, 4, 5, 0, 0, 0, None) == -2             # Ci > C
    assert crop(one, None, one, one, None, -1, 2, 2, 4, 2, 0, 0, 0, None) == -2            # negative extent
    assert crop(one, None, one, one, None, 2, 2, 2, 513, 2, 0, 0, 0, None) == -2           # more channels than the counter holds
    assert crop(one, None, one, one, None, 1 << 30, 1 << 20, 1 << 10, 4, 2, 0, 0, 0, None) == -2   # 2^60 voxels
    assert crop(one, None, one, one, None, 2, 2, 2, 4, 2, 8, 0, 0, None) == -3             # a fourth axis
    assert crop(one, None, one, one, None, 0, 2, 2, 4, 2, 0, 0, 0, None) == 0              # no voxels: nothing launched
    ptr_ok = (ctypes.c_int64 * 4)(0, 1, 1, 5)
    ptr_short = (ctypes.c_int64 * 4)(0, 1, 1, 4)
    ptr_down = (ctypes.c_int64 * 4)(0, 3, 1, 5)
    ptr_late = (ctypes.c_int64 * 4)(1, 1, 1, 5)
    assert feats(one, None, ptr_ok, one, one, 5, 20, 4, 3, 0.0, 0, 0, None) == -1
    assert feats(one, one, None, one, one, 5, 20, 4, 3, 0.0, 0, 0, None) == -1
    assert feats(one, one, ptr_ok, None, one, 5, 20, 4, 3, 0.0, 0, 0, None) == -1
    assert feats(None, one, ptr_ok, one, one, 5, 20, 4, 3, 0.0, 0, 0, None) == -1
    assert feats(one, one, ptr_ok, one, one, 5, 20, 3, 3, 0.0, 0, 0, None) == -2           # F % M
    assert feats(one, one, ptr_ok, one, one, -5, 20, 4, 3, 0.0, 0, 0, None) == -2
    assert feats(one, one, ptr_short, one, one, 5, 20, 4, 3, 0.0, 0, 0, None) == -2        # does not end at N
    assert feats(one, one, ptr_down, one, one, 5, 20, 4, 3, 0.0, 0, 0, None) == -2         # goes down
    assert feats(one, one, ptr_late, one, one, 5, 20, 4, 3, 0.0, 0, 0, None) == -2         # does not start at 0
    assert feats(one, one, ptr_ok, one, one, 5, 20, 4, 3, -1.0, 0, 0, None) == -3
    empty = (ctypes.c_int64 * 2)(0, 0)
    assert feats(None, one, empty, one, None, 0, 20, 4, 1, 0.0, 0, 0, None) == 0           # no rows: nothing launched


def test_ops_refuse_cpu_tensors_and_bad_shapes(hip_lib):
    import torch

    import gts
    from gts import ops
    from gts.augment import AugmentPlan

    plan = AugmentPlan.identity(4)
    with pytest.raises(gts.GtsError, match="MI355X only"):
        ops.augment_crop(torch.zeros(2, 2, 2, 8), None, plan)
    with pytest.raises(gts.GtsError, match="MI355X only"):
        ops.augment_features(torch.zeros(3, 20), [3], [plan])
    with pytest.raises(gts.GtsError, match="fp32"):
        ops.flip_crop(torch.zeros(8, 4, dtype=torch.float64), (2, 2, 2), (True, False, False))
    with pytest.raises(gts.GtsError, match="expected"):
        ops.flip_crop(torch.zeros(9, 4), (2, 2, 2), (True, False, False))
    with pytest.raises(gts.GtsError, match="one plan per graph"):
        ops.augment_features(torch.zeros(3, 20), [1, 2], [plan])
    with pytest.raises(gts.GtsError, match="labels must be"):
        ops.augment_crop(None, torch.zeros(8, dtype=torch.int64), plan)
