"""Co-register the modalities of a study that lie on different grids (R1 / R2, csrc/gts_register.hip).

Two steps, both on the device:
  header alignment   every modality is resampled from its own grid straight into the reference modality's conformed
                     frame (LPS, 1 mm) by one trilinear interpolation through T_k = inv(A_k) . R(params) . W, with W
                     the conformed frame's index -> world map (conform.conformed_affine) and A_k the modality's own
                     header affine;
  rigid refinement   params = (tx, ty, tz in mm, rx, ry, rz in degrees), found by a deterministic compass search that
                     maximises the mutual information of the joint intensity histogram of the conformed reference
                     and the resampled modality.  One R2 launch scores the 12 probes of a sweep; the only
                     synchronisation of a sweep is the copy of its K * (B^2 + 1) counts.

header_transform and mutual_information are pure numpy and run without a GPU.  Volumes on the device are [Z, Y, X],
x fastest, as intake.stage_scan lays them out; shapes are given (X, Y, Z) as conform.Plan gives them.
"""
from dataclasses import dataclass

import numpy as np

from . import conform

DEFAULT_LEVELS = (4, 2)
DEFAULT_BINS = 32
DEFAULT_MAX_ROTATE = 15.0
MIN_STEP = 0.0625
MAX_SWEEPS = 1000          # per level; every move raises the score, so this only guards against a cycle of ties


def rotation(rx, ry, rz):
    """Rz . Ry . Rx, angles in degrees."""
    ax, ay, az = (np.radians(np.float64(a)) for a in (rx, ry, rz))
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    r_x = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    r_y = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    r_z = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return r_z @ (r_y @ r_x)


def rigid(params, centre):
    """The 4x4 world -> world motion p -> R (p - centre) + centre + t of params = (tx, ty, tz, rx, ry, rz)."""
    params = np.asarray(params, dtype=np.float64).reshape(6)
    centre = np.asarray(centre, dtype=np.float64).reshape(3)
    m = np.eye(4)
    m[:3, :3] = rotation(*params[3:])
    m[:3, 3] = (centre + params[:3]) - m[:3, :3] @ centre
    return m


def header_transform(plan_ref, affine_ref, affine_k, params=None):
    """T_k = inv(A_k) . R(params) . W as a 3 x 4 float64 matrix: the index (x, y, z) of the reference modality's
    conformed volume -> index coordinates of modality k's stored volume.  W = conformed_affine(plan_ref, affine_ref);
    R (identity without params) rotates about the world position of the conformed volume's centre."""
    world = conform.conformed_affine(plan_ref, affine_ref)
    to_index = np.linalg.inv(np.asarray(affine_k, dtype=np.float64))
    if params is None:
        full = to_index @ world
    else:
        centre = world @ np.array([(n - 1) / 2.0 for n in plan_ref.out_shape] + [1.0])
        full = to_index @ (rigid(params, centre[:3]) @ world)
    return np.ascontiguousarray(full[:3, :])


def mutual_information(counts):
    """float64 sum of p log(p / (px py)) over the non-zero cells of the B x B part of one row of R2's counts (the
    last entry, the outside count, takes no part), added in row-major order; 0.0 when no sample is inside.  A [K,
    B*B + 1] table gives a float64 [K] array."""
    counts = np.asarray(counts)
    if counts.ndim == 2:
        return np.array([mutual_information(row) for row in counts], dtype=np.float64)
    bins = int(round(np.sqrt(counts.size - 1)))
    if counts.ndim != 1 or bins * bins + 1 != counts.size:
        raise ValueError(f"mutual_information takes [B*B + 1] counts, got {counts.shape}")
    table = counts[:-1].reshape(bins, bins).astype(np.int64)
    total = int(table.sum())
    if total == 0:
        return 0.0
    p = table / np.float64(total)
    px = table.sum(axis=1) / np.float64(total)
    py = table.sum(axis=0) / np.float64(total)
    filled = table > 0
    terms = p[filled] * np.log(p[filled] / (px[:, None] * py[None, :])[filled])
    return float(np.cumsum(terms)[-1])          # cumsum adds left to right


# ---- device side -------------------------------------------------------------------------------------------------

def resample_modalities(volumes, transforms, out_shape, out=None):
    """R1 per modality: float32 [C, OZ, OY, OX] with channel c = volumes[c] ([Z, Y, X] int16 or float32 on its own
    grid) sampled through transforms[c] (3 x 4).  A transform of None leaves that channel of `out` as it is."""
    import torch

    from . import ops

    ox, oy, oz = (int(n) for n in out_shape)
    if len(volumes) != len(transforms) or not volumes:
        raise ValueError("resample_modalities takes one transform per volume")
    if out is None:
        out = torch.empty((len(volumes), oz, oy, ox), dtype=torch.float32, device=volumes[0].device)
    for c, (volume, matrix) in enumerate(zip(volumes, transforms)):
        if matrix is not None:
            ops.affine_resample(volume.contiguous(), matrix, (ox, oy, oz), out=out[c])
    return out


def bin_ranges(fixed, moving, bins):
    """(lo_f, scale_f, lo_m, scale_m) from the smallest and largest finite value of each volume, taken on the device:
    scale = bins / (max - min), 0 for a constant volume."""
    import torch

    out = []
    for v in (fixed, moving):
        if v.is_floating_point():
            ok = torch.isfinite(v)
            big = torch.finfo(v.dtype).max
            pair = torch.stack([torch.where(ok, v, torch.full_like(v, big)).amin(),
                                torch.where(ok, v, torch.full_like(v, -big)).amax()]).to(torch.float64)
        else:
            pair = torch.stack(torch.aminmax(v)).to(torch.float64)
        out.append(pair)
    lo_f, hi_f, lo_m, hi_m = (float(x) for x in torch.cat(out).cpu())
    scale = lambda lo, hi: float(bins) / (hi - lo) if hi > lo else 0.0      # noqa: E731
    return lo_f, scale(lo_f, hi_f), lo_m, scale(lo_m, hi_m)


def joint_histograms(fixed, moving, transforms, stride, bins, ranges, grid_blocks=0):
    """R2: int64 [K, bins^2 + 1] on the device (ops.joint_histogram)."""
    from . import ops

    return ops.joint_histogram(fixed, moving, transforms, stride, bins, ranges, grid_blocks)


@dataclass(frozen=True)
class Registration:
    """What coregister found: params (tx, ty, tz mm, rx, ry, rz degrees), the mutual information there at the last
    level's stride, the number of R2 launches, the fraction of the last level's samples that fell outside the
    moving volume, and the 3 x 4 transform of params."""
    params: tuple
    score: float
    launches: int
    outside_fraction: float
    transform: np.ndarray


def probes(params, step, max_rotate):
    """The 12 neighbours of a compass sweep, in the order +e_0, -e_0, +e_1, ...; rotations clamped to +-max_rotate."""
    out = []
    for k in range(6):
        for sign in (1.0, -1.0):
            q = np.array(params, dtype=np.float64)
            q[k] = q[k] + sign * step
            if k >= 3:
                q[k] = min(max(q[k], -max_rotate), max_rotate)
            out.append(q)
    return out


def compass_search(score_many, levels=DEFAULT_LEVELS, max_rotate=DEFAULT_MAX_ROTATE):
    """The search itself, over score_many(list of params, stride) -> (scores, outside fractions), one launch each
    call.  Per level of stride s: score the current point, then sweeps of 12 probes at step s, s/2, ...: the first
    maximum among the probes is taken when it exceeds the current score, else the step halves; the level ends when
    the step falls below MIN_STEP.  Returns (params, score, launches, outside fraction)."""
    p = np.zeros(6, dtype=np.float64)
    launches, current, outside = 0, 0.0, 0.0
    for stride in levels:
        (current,), (outside,) = score_many([p], stride)
        launches += 1
        step, sweeps = float(stride), 0
        while step >= MIN_STEP and sweeps < MAX_SWEEPS:
            candidates = probes(p, step, max_rotate)
            scores, outsides = score_many(candidates, stride)
            launches += 1
            sweeps += 1
            best = int(np.argmax(scores))
            if scores[best] > current:
                p, current, outside = candidates[best], scores[best], outsides[best]
            else:
                step *= 0.5
    return p, float(current), launches, float(outside)


def coregister(fixed, moving, base_transform, levels=DEFAULT_LEVELS, bins=DEFAULT_BINS, max_rotate=DEFAULT_MAX_ROTATE,
               ranges=None):
    """Rigid refinement of `moving` ([Z, Y, X] int16 or float32 on its own grid) onto `fixed` (float32 [FZ, FY, FX],
    the conformed reference modality).  base_transform(params) -> the 3 x 4 matrix of those params, usually
    functools.partial(header_transform, plan_ref, affine_ref, affine_k).  ranges: bin_ranges(...) when the caller has
    them already.  Returns a Registration."""
    if ranges is None:
        ranges = bin_ranges(fixed, moving, bins)

    def score_many(param_list, stride):
        matrices = np.stack([base_transform(q) for q in param_list])
        counts = joint_histograms(fixed, moving, matrices, stride, bins, ranges).cpu().numpy()    # the sweep's one sync
        samples = counts.sum(axis=1)
        return mutual_information(counts), counts[:, -1] / np.maximum(samples, 1).astype(np.float64)

    p, score, launches, outside = compass_search(score_many, tuple(levels), float(max_rotate))
    return Registration(tuple(float(v) for v in p), score, launches, outside, base_transform(p))


def align_study(volumes, affines, ref, header_only=False, levels=DEFAULT_LEVELS, bins=DEFAULT_BINS,
                max_rotate=DEFAULT_MAX_ROTATE):
    """The study in the reference modality's conformed frame: (float32 [C, OZ, OY, OX], plan of the reference
    modality, one report dict per modality).  volumes: device tensors [Z, Y, X] (int16 or float32), each on its own
    grid; affines: their header affines; ref: the index of the reference modality.  The reference channel goes
    through conform.conform_scan (the same values `--conform` alone gives it); every other channel is one R1
    resample through its header transform, refined by coregister unless header_only."""
    import functools

    import torch

    plan = conform.plan(affines[ref], tuple(int(n) for n in volumes[ref].shape)[::-1])
    fixed = conform.conform_scan(volumes[ref].contiguous()[None], plan)[0].to(torch.float32)
    ox, oy, oz = plan.out_shape
    scan = torch.empty((len(volumes), oz, oy, ox), dtype=torch.float32, device=fixed.device)
    scan[ref] = fixed
    fixed = scan[ref]
    transforms, report = [], []
    for k, volume in enumerate(volumes):
        if k == ref:
            transforms.append(None)
            report.append({"modality": k, "reference": True})
            continue
        family = functools.partial(header_transform, plan, affines[ref], affines[k])
        if header_only:
            transforms.append(family(None))
            report.append({"modality": k, "reference": False, "params": [0.0] * 6, "score": None, "launches": 0,
                           "outside_fraction": None})
            continue
        found = coregister(fixed, volume.contiguous(), family, levels, bins, max_rotate)
        transforms.append(found.transform)
        report.append({"modality": k, "reference": False, "params": list(found.params), "score": found.score,
                       "launches": found.launches, "outside_fraction": found.outside_fraction})
    resample_modalities(volumes, transforms, plan.out_shape, out=scan)
    return scan, plan, report
