"""Host plan of the training-time augmentation: pure numpy, importable without a GPU.

An `Augmenter` draws one `AugmentPlan` per step: which axes of the crop are mirrored, a scale / shift per image
modality and the strength of the additive Gaussian noise, and (off by default) a rotation with an
isotropic zoom about the crop's centre.  The plan is applied on the GPU by gts.ops.augment_crop
(the CNN's input and labels), gts.ops.augment_features (the GNN's quantile features: quantiles with linear
interpolation commute with a * v + b for a > 0, so the same scale / shift on the five columns of a modality is exactly
the features of the mapped image; they do not change under a rotation) and gts.ops.flip_crop /
gts.ops.spatial_crop_bwd (labels and gradients of the joint step).

The augmenter owns one numpy generator and never touches torch's: a run with a given torch.manual_seed visits the
same samples in the same order with or without augmentation.
"""
from dataclasses import dataclass, field

import numpy as np

AXES = "xyz"
_MASK64 = (1 << 64) - 1


@dataclass(frozen=True)
class AugmentPlan:
    """What one step does to one sample.  flips: (x, y, z) booleans; scale / shift / sigma: float32 [channels], one per
    image modality (x' = x * scale + shift + sigma * n); feature_sigma: the noise on node features; seed: the two
    32-bit key words (low, high) of the noise generator; step: its 64-bit counter word; matrix: float64 [3, 3], the
    map from (mirrored) output offsets about the crop's centre to source offsets (include/gts_hip.h, A3): the identity
    leaves the grid alone."""
    flips: tuple = (False, False, False)
    scale: np.ndarray = field(default_factory=lambda: np.ones(4, dtype=np.float32))
    shift: np.ndarray = field(default_factory=lambda: np.zeros(4, dtype=np.float32))
    sigma: np.ndarray = field(default_factory=lambda: np.zeros(4, dtype=np.float32))
    feature_sigma: float = 0.0
    seed: tuple = (0, 0)
    step: int = 0
    matrix: np.ndarray = field(default_factory=lambda: np.eye(3))

    def __post_init__(self):
        flips = tuple(bool(f) for f in self.flips)
        if len(flips) != 3:
            raise ValueError("flips are three booleans, one per axis")
        object.__setattr__(self, "flips", flips)
        for name in ("scale", "shift", "sigma"):
            object.__setattr__(self, name, np.ascontiguousarray(getattr(self, name), dtype=np.float32).reshape(-1))
        if not (len(self.scale) == len(self.shift) == len(self.sigma)):
            raise ValueError("scale, shift and sigma hold one entry per channel")
        if np.any(~(self.scale > 0)) or np.any(~(self.sigma >= 0)) or not np.all(np.isfinite(self.shift)):
            raise ValueError("scales must be positive, sigmas not negative, shifts finite")
        if not self.feature_sigma >= 0:
            raise ValueError("feature_sigma must not be negative")
        seed = tuple(int(w) for w in self.seed)
        if len(seed) != 2 or any(w < 0 or w >= 1 << 32 for w in seed) or not 0 <= int(self.step) <= _MASK64:
            raise ValueError("seed is two 32-bit words, step a 64-bit counter")
        object.__setattr__(self, "seed", seed)
        object.__setattr__(self, "step", int(self.step))
        object.__setattr__(self, "feature_sigma", float(self.feature_sigma))
        matrix = np.array(self.matrix, dtype=np.float64)
        if matrix.shape != (3, 3):
            raise ValueError("matrix is float64 [3, 3]")
        if not np.all(np.isfinite(matrix)):
            raise ValueError("matrix entries must be finite")
        det = np.linalg.det(matrix)
        if det == 0 or not np.isfinite(det) or not np.all(np.isfinite(np.linalg.inv(matrix))):
            raise ValueError("matrix must be invertible")
        matrix.setflags(write=False)
        object.__setattr__(self, "matrix", matrix)

    @classmethod
    def identity(cls, channels=4):
        return cls(scale=np.ones(channels, dtype=np.float32), shift=np.zeros(channels, dtype=np.float32),
                   sigma=np.zeros(channels, dtype=np.float32))

    @property
    def channels(self):
        return len(self.scale)

    @property
    def flip_mask(self):
        """Bit 0 / 1 / 2: axis x / y / z is mirrored (the kernels' flip_mask)."""
        return sum(1 << a for a in range(3) if self.flips[a])

    @property
    def seed64(self):
        return self.seed[0] | (self.seed[1] << 32)

    @property
    def spatial(self):
        """The matrix differs from the identity: the crop is resampled (A3), not only mirrored (A1)."""
        return not np.array_equal(self.matrix, np.eye(3))

    @property
    def is_identity(self):
        return not any(self.flips) and bool(np.all(self.scale == 1)) and bool(np.all(self.shift == 0)) \
            and not np.any(self.sigma) and self.feature_sigma == 0.0 and not self.spatial


def rotation_zoom_matrix(angles, zoom):
    """M = Rz(gamma) Ry(beta) Rx(alpha) / zoom in float64: angles (alpha, beta, gamma) in degrees about x, y, z;
    zoom > 1 magnifies (the source offsets shrink)."""
    a, b, g = (np.deg2rad(float(t)) for t in angles)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0.0, np.sin(b)], [0.0, 1.0, 0.0], [-np.sin(b), 0.0, np.cos(b)]])
    rz = np.array([[np.cos(g), -np.sin(g), 0.0], [np.sin(g), np.cos(g), 0.0], [0.0, 0.0, 1.0]])
    return (rz @ ry @ rx) / float(zoom)


class Augmenter:
    """Draws AugmentPlans from np.random.default_rng(seed).

    One draw() consumes, in this order (a test can replay it from numpy):
      1. rng.random(3)                      -> axis a is mirrored when it is named in flip_axes and value < flip_prob
      2. rng.uniform(1 - scale, 1 + scale, channels)       -> scale
      3. rng.uniform(-shift, shift, channels)              -> shift
      4. rng.random(channels)               -> channel c is noisy when value < noise_prob
      5. rng.uniform(0, noise_sigma, channels)             -> sigma of the noisy channels (0 elsewhere)
    All five are drawn whatever the settings, so the stream of one setting lines up with that of another.  scale,
    shift and sigma are rounded to float32 (what the kernels take).  plan.step counts the draws from 0;
    plan.seed is (seed & 0xffffffff, seed >> 32 & 0xffffffff).

    The rotation and zoom draw from a SECOND generator, np.random.default_rng(np.random.SeedSequence(seed,
    spawn_key=(1,))), so the five draws above are what they are without them.  Per draw(), always in this order:
      6. rng2.random()                                     -> u
      7. rng2.uniform(-rotate, rotate, 3)                  -> the angles about x, y, z in degrees
      8. rng2.uniform(1 - zoom, 1 + zoom)                  -> s (s > 1 magnifies)
    The plan is spatial when u < spatial_prob and (rotate > 0 or zoom > 0): matrix = Rz Ry Rx / s
    (rotation_zoom_matrix); otherwise the matrix is the exact identity."""

    def __init__(self, seed, channels=4, flip_axes="xyz", flip_prob=0.5, scale=0.1, shift=0.1, noise_prob=0.5,
                 noise_sigma=0.1, feature_noise_sigma=0.0, rotate=0.0, zoom=0.0, spatial_prob=0.5):
        seed, channels = int(seed), int(channels)
        if seed < 0:
            raise ValueError("seed must not be negative")
        if channels < 1:
            raise ValueError("channels must be positive")
        if not isinstance(flip_axes, str) or any(a not in AXES for a in flip_axes):
            raise ValueError(f'flip_axes is a subset of "{AXES}", got {flip_axes!r}')
        for name, p in (("flip_prob", flip_prob), ("noise_prob", noise_prob), ("spatial_prob", spatial_prob)):
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"{name} is a probability, got {p}")
        if not 0.0 <= scale < 1.0:
            raise ValueError(f"scale must be in [0, 1): the map a * v + b needs a > 0, got {scale}")
        for name, s in (("shift", shift), ("noise_sigma", noise_sigma), ("feature_noise_sigma", feature_noise_sigma)):
            if not (s >= 0.0 and np.isfinite(s)):
                raise ValueError(f"{name} must be finite and not negative, got {s}")
        if not 0.0 <= rotate <= 180.0:
            raise ValueError(f"rotate is an angle in degrees in [0, 180], got {rotate}")
        if not 0.0 <= zoom < 1.0:
            raise ValueError(f"zoom must be in [0, 1): the zoom factor 1 +- zoom stays positive, got {zoom}")
        self.seed, self.channels = seed, channels
        self.flip_axes = "".join(a for a in AXES if a in flip_axes)
        self.flip_prob, self.scale, self.shift = float(flip_prob), float(scale), float(shift)
        self.noise_prob, self.noise_sigma = float(noise_prob), float(noise_sigma)
        self.feature_noise_sigma = float(feature_noise_sigma)
        self.rotate, self.zoom, self.spatial_prob = float(rotate), float(zoom), float(spatial_prob)
        self.rng = np.random.default_rng(seed)
        self.rng2 = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(1,)))
        self.steps = 0

    def draw(self):
        rng, n = self.rng, self.channels
        flip_u = rng.random(3)
        scale = rng.uniform(1.0 - self.scale, 1.0 + self.scale, n)
        shift = rng.uniform(-self.shift, self.shift, n)
        noisy = rng.random(n) < self.noise_prob
        sigma = np.where(noisy, rng.uniform(0.0, self.noise_sigma, n), 0.0)
        flips = tuple(bool(AXES[a] in self.flip_axes and flip_u[a] < self.flip_prob) for a in range(3))
        rng2 = self.rng2
        u = rng2.random()
        angles = rng2.uniform(-self.rotate, self.rotate, 3)
        s = rng2.uniform(1.0 - self.zoom, 1.0 + self.zoom)
        spatial = u < self.spatial_prob and (self.rotate > 0 or self.zoom > 0)
        matrix = rotation_zoom_matrix(angles, s) if spatial else np.eye(3)
        plan = AugmentPlan(flips, scale.astype(np.float32), shift.astype(np.float32), sigma.astype(np.float32),
                           self.feature_noise_sigma, (self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF),
                           self.steps, matrix)
        self.steps += 1
        return plan

    def describe(self):
        text = (f"augmentation: seed {self.seed}, flips {self.flip_axes or '-'} with probability {self.flip_prob}, "
                f"scale 1 +- {self.scale}, shift +- {self.shift}, noise sigma <= {self.noise_sigma} with "
                f"probability {self.noise_prob}, feature noise sigma {self.feature_noise_sigma}")
        if self.rotate > 0 or self.zoom > 0:
            text += (f", rotation +- {self.rotate} degrees per axis and zoom 1 +- {self.zoom} with probability "
                     f"{self.spatial_prob}")
        return text


# ---------------------------------------------------------------- command line (shared by the three trainers)
def add_augment_arguments(parser, flips=True):
    """--augment and its settings.  flips=False (train_gnn): the flip, rotation, zoom and noise flags are accepted and
    ignored, node features have no axes to mirror or turn and image noise has no exact counterpart on quantiles."""
    ignored = " (ignored here: node features have no axes)" if not flips else ""
    no_noise = " (ignored here: the node features take scale and shift only)" if not flips else ""
    parser.add_argument("--augment", default=False, action="store_true",
                        help="augment training samples on the GPU: mirrored crops, per-modality scale / shift, noise")
    parser.add_argument("--aug_flip_axes", default="xyz", type=str, help="axes that may be mirrored" + ignored)
    parser.add_argument("--aug_flip_prob", default=0.5, type=float, help="probability of mirroring each axis" + ignored)
    parser.add_argument("--aug_scale", default=0.1, type=float, help="modality scale drawn in [1 - s, 1 + s]")
    parser.add_argument("--aug_shift", default=0.1, type=float, help="modality shift drawn in [-s, s]")
    parser.add_argument("--aug_noise", default=0.1, type=float, help="largest sigma of the additive Gaussian noise" + no_noise)
    parser.add_argument("--aug_noise_prob", default=0.5, type=float, help="probability that a modality gets noise" + no_noise)
    parser.add_argument("--aug_seed", default=0, type=int, help="seed of the augmentation's own generator")
    parser.add_argument("--aug_rotate", default=0.0, type=float,
                        help="largest rotation about each axis in degrees, 0: none" + ignored)
    parser.add_argument("--aug_zoom", default=0.0, type=float,
                        help="isotropic zoom drawn in [1 - z, 1 + z], 0: none" + ignored)
    parser.add_argument("--aug_spatial_prob", default=0.5, type=float,
                        help="probability that a sample is rotated and zoomed" + ignored)


def augmenter_from_args(args, channels=4, rank=0, features_only=False):
    """None without --augment, else the configured Augmenter (seeded with --aug_seed + rank).  features_only: for the
    GNN, whose input is node features alone: scale and shift, no flips and no noise."""
    if not args.augment:
        return None
    if features_only:
        return Augmenter(args.aug_seed + rank, channels, "", 0.0, args.aug_scale, args.aug_shift, 0.0, 0.0)
    return Augmenter(args.aug_seed + rank, channels, args.aug_flip_axes, args.aug_flip_prob, args.aug_scale,
                     args.aug_shift, args.aug_noise_prob, args.aug_noise, rotate=args.aug_rotate, zoom=args.aug_zoom,
                     spatial_prob=args.aug_spatial_prob)
