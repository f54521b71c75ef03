"""The co-registration kernels on the MI355X (gts/register.py, csrc/gts_register.hip) against
tests/register_ref.py: R1 byte for byte, R2 integer for integer, the search bit for bit, and
`segment_scans --coregister` end to end on a study whose modalities lie on different grids."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import register_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gnn-tumor-seg_amd")
DEV = "cuda"

# (1,1,1); odd; longer than a wave along x; across the 64-wide LDS tile's edge in each tiled axis; more than one
# workgroup of 256 samples at every stride used
SHAPES = [(1, 1, 1), (5, 6, 7), (65, 3, 18), (70, 37, 3), (72, 5, 67)]
SIGNS = [(1, -1, 1), (-1, 1, -1), (1, 1, -1), (-1, -1, 1), (-1, 1, 1), (1, 1, 1)]


def _dev(a):
    """[X, Y, Z] numpy -> device tensor [Z, Y, X] (x fastest)."""
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)


def _host(t):
    return t.cpu().numpy().T


def _values(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        return rng.integers(-30000, 30001, shape).astype(np.int16)
    v = (rng.uniform(-3e4, 3e4, shape) * rng.choice([1.0, 1e-3, 1e-6], shape)).astype(np.float32)
    v.flat[0] = -0.0
    return v


def _about_centre(m3, shape):
    """The 3 x 4 matrix x -> m3 (x - c) + c about the volume's centre."""
    c = (np.array(shape, dtype=np.float64) - 1.0) / 2.0
    return np.hstack([m3, (c - m3 @ c)[:, None]])


def _rotation(axis, degrees):
    a = np.radians(degrees)
    j, k = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[j, j] = m[k, k] = np.cos(a)
    m[j, k], m[k, j] = -np.sin(a), np.sin(a)
    return m


def _permutation(shape, perm, signs):
    """(T, out_shape): output axis perm[j] runs along input axis j, backwards where signs[j] < 0."""
    T = np.zeros((3, 4))
    out = [0, 0, 0]
    for j in range(3):
        T[j, perm[j]] = signs[j]
        T[j, 3] = shape[j] - 1 if signs[j] < 0 else 0.0
        out[perm[j]] = shape[j]
    return T, tuple(out)


def transforms(shape):
    """[(name, T, out_shape)]: what the issue lists.  The identity samples u = X - 1 exactly; so does every flip."""
    eye = np.eye(4)[:3]
    shift = eye.copy()
    shift[0, 3] = 2.0                                   # the high-x face leaves the volume
    half = eye.copy()
    half[:, 3] = 0.5
    gone = eye.copy()
    gone[0, 3] = shape[0] + 5.0
    cases = [("identity", eye, shape), ("shift", shift, shape), ("half", half, shape), ("outside", gone, shape)]
    for perm, signs in zip(itertools.permutations(range(3)), SIGNS):
        T, out = _permutation(shape, perm, signs)
        cases.append((f"perm{perm}{signs}", T, out))
    for axis in range(3):
        cases.append((f"rot{axis}", _about_centre(_rotation(axis, 10.0), shape), shape))
    spacing = (0.9375, 0.9375, 5.0)                      # the input's voxels in mm, 1 mm out, one sample past the end
    out = tuple(int(np.floor((n - 1) * s)) + 2 for n, s in zip(shape, spacing))
    cases.append(("scale", np.hstack([np.diag([1.0 / s for s in spacing]), np.zeros((3, 1))]), out))
    return cases


@pytest.mark.parametrize("shape", SHAPES)
def test_resample_is_byte_equal_to_the_reference(hip_lib, shape):
    from gts import ops

    for dtype in (np.int16, np.float32):
        a = _values(shape, dtype, 1)
        src = _dev(a)
        for name, T, out_shape in transforms(shape):
            want = R.affine_resample(a, T, out_shape)
            if name == "outside":
                assert not want.any()
            for path in (ops.RESAMPLE_AUTO, ops.RESAMPLE_PLAIN, ops.RESAMPLE_TILED):
                got = ops.affine_resample(src, T, out_shape, path=path)
                assert got.dtype == torch.float32 and tuple(got.shape) == tuple(out_shape)[::-1]
                assert _host(got).tobytes() == want.tobytes(), (shape, dtype, name, path)


def test_resample_passes_non_finite_values_through_where_t_is_zero(hip_lib):
    """A sample on a voxel is that voxel: a NaN or Inf neighbour with no weight does not reach it."""
    from gts import ops

    shape = (70, 37, 3)
    a = _values(shape, np.float32, 2)
    a[3, 4, 1], a[4, 4, 1], a[69, 36, 2], a[10, 0, 0] = np.nan, np.inf, -np.inf, np.nan
    src = _dev(a)
    for name, T, out_shape in transforms(shape):
        if name in ("identity", "shift", "outside") or name.startswith("perm"):
            want = R.affine_resample(a, T, out_shape)
            for path in (ops.RESAMPLE_PLAIN, ops.RESAMPLE_TILED):
                assert _host(ops.affine_resample(src, T, out_shape, path=path)).tobytes() == want.tobytes(), name


def test_resample_modalities_writes_channel_slices_and_refuses_bad_operands(hip_lib):
    from gts import _lib, ops, register

    shapes = [(9, 8, 5), (5, 6, 7), (12, 4, 6)]
    vols = [_values(s, np.int16 if k != 1 else np.float32, 3 + k) for k, s in enumerate(shapes)]
    out_shape = (10, 7, 6)
    mats = [_about_centre(_rotation(k, 10.0), s) for k, s in enumerate(shapes)]
    got = register.resample_modalities([_dev(v) for v in vols], mats, out_shape)
    assert tuple(got.shape) == (3, 6, 7, 10) and got.dtype == torch.float32
    for c in range(3):
        assert _host(got[c]).tobytes() == R.affine_resample(vols[c], mats[c], out_shape).tobytes()
    src = _dev(vols[0])
    with pytest.raises(_lib.GtsError):
        ops.affine_resample(src.cpu(), mats[0], out_shape)                   # no CPU route
    with pytest.raises(_lib.GtsError):
        ops.affine_resample(src.to(torch.float64), mats[0], out_shape)
    with pytest.raises(_lib.GtsError):
        ops.affine_resample(src, np.full((3, 4), np.nan), out_shape)
    with pytest.raises(_lib.GtsError):
        ops.affine_resample(src, mats[0], (0, 7, 6))
    with pytest.raises(_lib.GtsError):
        ops.joint_histogram(got[0], src, mats[0], 1, 24, (0.0, 1.0, 0.0, 1.0))
    with pytest.raises(_lib.GtsError):
        ops.joint_histogram(got[0], src, np.stack([mats[0]] * 17), 1, 32, (0.0, 1.0, 0.0, 1.0))


# ---- R1 against conform: the two features share one sampler (csrc/gts_scan.h) ------------------------------------------

# (perm, signs, offsets of the shape): output axis perm[j] runs along input axis j, u_j = signs[j] * i + offsets[j].
# Offsets are an integer shift plus 0, 0.25 or 0.5, so u, floor(u) and u - floor(u) are exact in float64 whether T @ (x,
# y, z, 1) forms them on the device or numpy does for conform's tables: both features must then give the same bits.
# The first map keeps x on x (conform's row kernel, R1's plain lane map), the others move it (the tiled kernels).
DYADIC_MAPS = [((0, 1, 2), (1, 1, 1), lambda n: (0.25, 0.5, 1.0)),
               ((1, 0, 2), (1, -1, 1), lambda n: (1.5, n[1] - 1.25, 0.0)),
               ((2, 0, 1), (-1, 1, -1), lambda n: (n[0] - 1.5, 0.25, n[2] - 2.0)),
               ((2, 1, 0), (1, 1, -1), lambda n: (2.25, 0.0, n[2] - 1.5))]


def _dyadic_map(shape, perm, signs, offsets):
    """(T, out_shape, axes, tables, inside [OX, OY, OZ]) of one map: R1's matrix, and conform's input axis and
    AxisTables per output axis built from the same numbers by R1's rule (i0 = min(floor(u), n - 1), i1 = min(i0 + 1,
    n - 1), t = u - i0).  An index R1 leaves outside gets the table entry (0, 0, 0.0) and is not compared."""
    from gts.conform import AxisTables

    T, out, axes, tables, inside = np.zeros((3, 4)), [0] * 3, [0] * 3, [None] * 3, [None] * 3
    for j in range(3):
        w, n = perm[j], shape[j]
        T[j, w], T[j, 3], out[w], axes[w] = signs[j], offsets[j], n, j
        u = signs[j] * np.arange(n, dtype=np.float64) + offsets[j]
        inside[w] = (u >= 0) & (u <= n - 1)
        i0 = np.where(inside[w], np.minimum(np.floor(u), n - 1), 0.0)
        i1 = np.where(inside[w], np.minimum(i0 + 1, n - 1), 0.0)
        tables[w] = AxisTables(i0.astype(np.int32), i1.astype(np.int32), np.where(inside[w], u - i0, 0.0))
    return T, tuple(out), tuple(axes), tuple(tables), inside[0][:, None, None] & inside[1][None, :, None] & inside[2]


def _check_against_conform(a, perm, signs, offsets):
    from gts import conform, ops

    T, out_shape, axes, tables, inside = _dyadic_map(a.shape, perm, signs, offsets)
    assert inside.any() and not inside.all()
    src = _dev(a)
    want = _host(conform._gather(src, axes, tables, conform.MODE_TRILINEAR, "test"))
    assert want.dtype == np.float32 and want.shape == out_shape
    assert want[inside].tobytes() == R.affine_resample(a, T, out_shape)[inside].tobytes(), (a.shape, a.dtype, perm)
    for path in (ops.RESAMPLE_AUTO, ops.RESAMPLE_PLAIN, ops.RESAMPLE_TILED):
        got = _host(ops.affine_resample(src, T, out_shape, path=path))
        assert got[inside].tobytes() == want[inside].tobytes(), (a.shape, a.dtype, perm, path)
        assert not got[~inside].any()
    return want, inside


@pytest.mark.parametrize("shape", [(5, 6, 7), (65, 3, 18)])
def test_resample_and_conform_give_the_same_bits_on_dyadic_maps(hip_lib, shape):
    for dtype in (np.int16, np.float32):
        a = _values(shape, dtype, 16)
        for perm, signs, offsets in DYADIC_MAPS:
            _check_against_conform(a, perm, signs, offsets(shape))


def test_resample_and_conform_agree_on_a_nan_neighbour_without_weight(hip_lib):
    """Whole offsets along the input's x: every sample lies on a voxel along x, and its other x neighbour, NaN or not,
    carries no weight.  The voxel before the NaN stays finite in both features, the NaN itself is sampled by both."""
    shape = (5, 6, 7)
    a = _values(shape, np.float32, 17)
    a[3, 2, 4] = np.nan
    for perm, signs, offsets in DYADIC_MAPS:
        off = offsets(shape)
        off = (float(np.floor(off[0])),) + tuple(off[1:])
        want, inside = _check_against_conform(a, perm, signs, off)
        reads_x = (signs[0] * np.arange(shape[0]) + off[0]).astype(int)          # input x of output index i along perm[0]
        by_x = np.moveaxis(want, perm[0], 0)
        ok = np.moveaxis(inside, perm[0], 0)
        for i, x in enumerate(reads_x):
            if ok[i].any():
                assert np.isnan(by_x[i][ok[i]]).any() == (x == 3), (perm, i, x)


# ---- R2 --------------------------------------------------------------------------------------------------------------

def _fixed(shape, seed):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.0, 900.0, shape).astype(np.float32)
    f[rng.random(shape) < 0.5] = 0.0                       # half the voxels are background: one crowded row of cells
    return f


def _matrices(shape, fixed_shape, k):
    """k matrices from the fixed grid into the moving one: the listed transforms (those whose output grid is the
    fixed grid's shape or not: any T is valid), cycled."""
    pool = [T for _, T, _ in transforms(shape)]
    order = [0, 10, 2, 3, 11, 1, 12, 13, 4, 5, 6, 7, 8, 9]
    return np.stack([pool[order[i % len(order)]] for i in range(k)])


def _check_counts(fixed, moving, mats, stride, bins, ranges=None, grid_blocks=0):
    from gts import register

    ranges = ranges or R.bin_ranges(fixed, moving, bins)
    want = R.joint_histogram(fixed, moving, mats, stride, bins, ranges)
    got = register.joint_histograms(_dev(fixed), _dev(moving), mats, stride, bins, ranges, grid_blocks)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(mats), bins * bins + 1)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (fixed.shape, moving.shape, stride, bins, len(mats), np.abs(got - want).sum())
    assert np.all(got.sum(axis=1) == R.strided_samples(fixed.shape, stride))
    return got


@pytest.mark.parametrize("shape", SHAPES)
def test_histogram_counts_equal_the_reference(hip_lib, shape):
    for dtype in (np.int16, np.float32):
        moving = _values(shape, dtype, 5)
        fixed = _fixed(shape, 6)
        for stride in (1, 2, 3):
            got = _check_counts(fixed, moving, _matrices(shape, shape, 12), stride, 32)
        assert got[:, -1].max() == R.strided_samples(shape, 3) and got[0, -1] == 0      # all outside; all inside


@pytest.mark.parametrize("bins", [16, 32, 64])
@pytest.mark.parametrize("k", [1, 12, 16])
def test_histogram_bins_and_matrix_counts(hip_lib, bins, k):
    """K = 16 at B = 64 takes four passes of four tables, K = 12 three; the fixed grid differs from the moving one."""
    moving = _values((72, 5, 67), np.int16, 7)
    fixed = _fixed((33, 20, 9), 8)
    _check_counts(fixed, moving, _matrices(moving.shape, fixed.shape, k), 1, bins)


def test_device_bin_ranges_equal_the_reference(hip_lib):
    from gts import register

    for dtype in (np.int16, np.float32):
        moving = _values((9, 8, 5), dtype, 9)
        fixed = _fixed((5, 6, 7), 10)
        fixed[1, 1, 1], fixed[2, 2, 2] = np.nan, np.inf
        assert register.bin_ranges(_dev(fixed), _dev(moving), 32) == R.bin_ranges(fixed, moving, 32)
    flat = np.full((4, 4, 4), 7, dtype=np.int16)
    assert register.bin_ranges(_dev(fixed), _dev(flat), 16)[2:] == (7.0, 0.0)


def test_histogram_with_every_sample_in_one_cell(hip_lib):
    """The contention case: 64 lanes of every wave add to one LDS word."""
    shape = (70, 37, 3)
    fixed = np.full(shape, 3.0, dtype=np.float32)
    moving = np.full(shape, 11, dtype=np.int16)
    eye = np.eye(4)[:3]
    for ranges in ((0.0, 1.0, 0.0, 1.0), R.bin_ranges(fixed, moving, 32)):
        got = _check_counts(fixed, moving, np.stack([eye] * 12), 1, 32, ranges)
        assert np.count_nonzero(got[0]) == 1 and got[0].max() == 70 * 37 * 3


def test_histogram_sends_non_finite_values_to_bin_zero(hip_lib):
    shape = (65, 3, 18)
    moving = _values(shape, np.float32, 11)
    fixed = _fixed(shape, 12)
    rng = np.random.default_rng(13)
    for v in (moving, fixed):
        v[rng.random(shape) < 0.05] = np.nan
        v[rng.random(shape) < 0.05] = np.inf
        v[rng.random(shape) < 0.05] = -np.inf
    for stride in (1, 2):
        got = _check_counts(fixed, moving, _matrices(shape, shape, 12), stride, 32)
    assert got[0, 0] > 0.002 * 65 * 3 * 18                  # both non-finite: cell (0, 0)


def test_histogram_is_deterministic_at_every_grid(hip_lib):
    from gts import register

    shape = (72, 5, 67)
    moving, fixed = _values(shape, np.int16, 14), _fixed(shape, 15)
    mats = _matrices(shape, shape, 12)
    ranges = R.bin_ranges(fixed, moving, 32)
    f, m = _dev(fixed), _dev(moving)
    first = register.joint_histograms(f, m, mats, 1, 32, ranges).cpu()
    assert torch.equal(first, register.joint_histograms(f, m, mats, 1, 32, ranges).cpu())
    for grid in (1, 3, 2048):                               # one workgroup strides over everything; more than needed
        assert torch.equal(first, register.joint_histograms(f, m, mats, 1, 32, ranges, grid_blocks=grid).cpu()), grid
    assert np.array_equal(first.numpy(), R.joint_histogram(fixed, moving, mats, 1, 32, ranges))


# ---- the search ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [5, 11])
def test_gpu_search_equals_the_reference_search_exactly(hip_lib, seed):
    from gts import register
    from tests.test_register_host import displacement, phantom

    fixed, moving, family, brain, carried = phantom(seed)
    params, score, launches, outside = R.search(fixed, moving, family, (2, 1), 32)
    found = register.coregister(_dev(fixed), _dev(moving), family, levels=(2, 1), bins=32)
    print(f"seed {seed}: {found.launches} launches, MI {found.score!r}, params {found.params}, "
          f"mean displacement {displacement(found.transform, carried, brain)[0]:.4f}")
    assert np.array(found.params).tobytes() == np.asarray(params, dtype=np.float64).tobytes()
    assert found.launches == launches
    assert np.float64(found.score).tobytes() == np.float64(score).tobytes()
    assert np.float64(found.outside_fraction).tobytes() == np.float64(outside).tobytes()
    assert found.transform.tobytes() == family(params).tobytes()


# ---- end to end: one child process writes a study on three grids and runs segment_scans --coregister on it ----------

_E2E = r"""
import json, os, sys
import numpy as np, torch
from data_processing import nifti_io
from gts import conform, register, synth_mri
from model.networks import init_graph_net
from utils.hyperparam_helpers import EvalParamSet
from scripts import segment_scans
from tests import conform_ref as C
from tests import register_ref as R
tmp = sys.argv[1]
MODS = ("_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz")
SHAPE = (64, 60, 40)
img, _ = synth_mri.make_sample(31, SHAPE)
frame = [img[..., c].astype(np.int16) for c in range(4)]          # the four modalities in the LPS 1 mm frame
lps = np.array(nifti_io.BRATS_AFFINE, dtype=np.float64); lps[:3, 3] = (31.5, 29.5, -20.0)   # that frame's affine
ras = C.make_affine((0, 1, 2), (1, 1, 1), origin=(-31.5, -29.5, -20.0))                     # the reference grid
to_frame = np.linalg.inv(lps)

def write(root, sid, volumes, affines):
    os.makedirs(os.path.join(root, sid), exist_ok=True)
    for v, ext, a in zip(volumes, MODS, affines):
        nifti_io.save_as_nifti(np.asfortranarray(v), os.path.join(root, sid, sid + ext), affine=a)

def stored(volume, affine, shape):
    # what a scanner that saw `volume` in the frame stores on the grid (affine, shape)
    return np.rint(R.affine_resample(volume, (to_frame @ affine)[:3], shape)).astype(np.int16)

on_ref = lambda v: np.ascontiguousarray(v[::-1, ::-1, :])
a1 = C.make_affine((2, 0, 1), (1, -1, 1), (1.2, 0.8, 3.0), (31.5, -29.5, -20.0))             # S, L, A at 1.2 x 0.8 x 3 mm
shape1 = (34, 80, 20)
centre = np.array([0.0, 0.0, -0.5])
motion = register.rigid((1.5, -2.0, 1.0, 3.0, -2.0, 4.0), centre)                            # the patient moved
header = register.rigid((6.0, 4.0, -3.0, 0.0, 0.0, 12.0), centre)                            # and the series was re-planned
a2 = header @ lps
vol2 = np.rint(R.affine_resample(frame[2], (to_frame @ motion @ a2)[:3], SHAPE)).astype(np.int16)
raw = os.path.join(tmp, "raw")
write(raw, "S", [on_ref(frame[0]), stored(frame[1], a1, shape1), vol2, on_ref(frame[3])], [ras, a1, a2, ras])
same = os.path.join(tmp, "same")
write(same, "R4", [on_ref(frame[0])] * 4, [ras] * 4)
torch.manual_seed(0)
hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
gnn = os.path.join(tmp, "gnn.pt")
torch.save(init_graph_net("GSpool", hp).state_dict(), gnn)
common = ["-o", os.path.join(tmp, "out"), "-g", gnn, "-n", "400"]
report = os.path.join(tmp, "report.json")
rc1 = segment_scans.main(["-d", raw] + common + ["--coregister", "--coregister_report", report])
rc2 = segment_scans.main(["-d", raw, "-o", os.path.join(tmp, "out_conform"), "-g", gnn, "-n", "400", "--conform"])
print("RC", rc1, rc2)

# the aligned scan itself: the reference channel against --conform alone, a header-only channel against the reference
seg = segment_scans.Segmenter(segment_scans.parse_args(["-d", raw] + common + ["--coregister", "--coregister_header_only"]))
scan, plan, _ = seg.align(seg.load(os.path.join(raw, "S")))
alone = segment_scans.Segmenter(segment_scans.parse_args(["-d", same] + common + ["--conform"]))
staged, plan4, _ = alone.load(os.path.join(same, "R4"))
conformed = conform.conform_scan(staged.to(scan.device), plan4)
print("REF_EQUAL", plan.out_shape == plan4.out_shape and torch.equal(scan[0], conformed[0].to(torch.float32)))
# modality 3 lies on the reference grid: its header transform is the flips, every sample on a voxel
print("FRAME_EQUAL", np.array_equal(scan[0].cpu().numpy().T, frame[0].astype(np.float32)),
      np.array_equal(scan[3].cpu().numpy().T, frame[3].astype(np.float32)))
# the affines as the files hold them (a NIfTI-1 header keeps float32 rows): what segment_scans read
affs = {k: nifti_io.read_affine(os.path.join(raw, "S", "S" + MODS[k]))[0] for k in (1, 2, 3)}
t1 = register.header_transform(plan, ras, affs[1])
want1 = R.affine_resample(stored(frame[1], a1, shape1), t1, plan.out_shape)
print("HEADER_ONLY_EQUAL", scan[1].cpu().numpy().T.tobytes() == want1.tobytes())

# how far the found transforms leave the brain's voxels from where they belong, in mm (the frame is 1 mm)
brain = frame[0] > 0
x = np.stack(np.nonzero(brain) + (np.ones(int(brain.sum())),)).astype(np.float64)
def gap(t_found, truth):          # truth: frame index -> stored index of the data; both 4x4
    d = (lps @ np.linalg.inv(truth) @ np.vstack([t_found, [0, 0, 0, 1.0]]) @ x - lps @ x)[:3]
    return float(np.sqrt((d ** 2).sum(axis=0)).mean())
found = json.load(open(report))["scans"]["S"]
truth = {1: np.linalg.inv(a1) @ lps, 2: np.linalg.inv(a2) @ np.linalg.inv(motion) @ lps, 3: np.linalg.inv(ras) @ lps}
data = {1: stored(frame[1], a1, shape1), 2: vol2, 3: on_ref(frame[3])}
import functools
for k in (1, 2, 3):
    family = functools.partial(register.header_transform, plan, ras, affs[k])
    print("GAP", k, gap(family(None), truth[k]), gap(family(np.array(found[k]["params"])), truth[k]))
    p, score, launches, outside = R.search(frame[0].astype(np.float32), data[k], family, (4, 2), 32)
    print("SEARCH_EQUAL", k, found[k]["params"] == p.tolist() and found[k]["score"] == score and
          found[k]["launches"] == launches and found[k]["outside_fraction"] == outside)
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, hip_lib):
    tmp = tmp_path_factory.mktemp("coregister_e2e")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-c", _E2E, str(tmp)], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=500)
    assert r.returncode == 0 and "RC 0 1" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)
    return tmp, r.stdout


def test_e2e_labels_lie_on_the_reference_modalitys_grid(e2e):
    from data_processing import nifti_io

    tmp, out = e2e
    fp = str(tmp / "out" / "S.nii.gz")
    labels, affine = nifti_io.read_nifti_raw(fp), nifti_io.read_affine(fp)[0]
    ref_affine = nifti_io.read_affine(str(tmp / "raw" / "S" / "S_flair.nii.gz"))[0]
    assert labels.dtype == np.int16 and labels.shape == (64, 60, 40) and np.array_equal(affine, ref_affine)
    assert set(np.unique(labels).tolist()) <= {0, 1, 2, 4}
    done = [ln for ln in out.splitlines() if ln.startswith("S: done")]
    assert len(done) == 1 and "conform: RAS -> LPS" in done[0] and "coregister: rigid, largest translation" in done[0]


def test_e2e_report_holds_the_found_parameters(e2e):
    tmp, out = e2e
    with open(tmp / "report.json") as f:
        report = json.load(f)
    assert report["reference"] == "_flair.nii.gz" and list(report["scans"]) == ["S"]
    rows = report["scans"]["S"]
    assert [r["modality"] for r in rows] == [0, 1, 2, 3] and rows[0]["reference"] is True
    for r in rows[1:]:
        assert len(r["params"]) == 6 and all(abs(a) <= 15.0 for a in r["params"][3:])
        assert r["launches"] >= 2 + 2 * 7 and r["score"] > 0.0 and 0.0 <= r["outside_fraction"] < 1.0
    # every search equals the reference search on the same volumes, number for number (json round-trips a float64)
    assert all(f"SEARCH_EQUAL {k} True" in out for k in (1, 2, 3))
    # GAP k: the mean distance in mm, over the brain's voxels, between where a transform puts a voxel and where it
    # belongs: by the headers alone, then as found.  The headers are exact for modalities 1 and 3, which did not
    # move, up to the float32 rows of a NIfTI-1 header (2^-24 of coordinates below 100 mm: under 1e-4 mm); modality 2
    # moved by 2.9 mm, and a search that works at all leaves less than half of that.  (What the
    # search finds for 1 and 3 is the definition's own answer on this phantom, whose modalities differ in the phase
    # of their texture: it is held to the reference above, not to zero.)
    gaps = {int(ln.split()[1]): (float(ln.split()[2]), float(ln.split()[3])) for ln in out.splitlines()
            if ln.startswith("GAP ")}
    assert gaps[1][0] < 1e-4 and gaps[3][0] < 1e-4
    assert gaps[2][0] > 2.0 and gaps[2][1] < 0.5 * gaps[2][0]


def test_e2e_reference_channel_equals_conform_alone(e2e):
    _, out = e2e
    assert "REF_EQUAL True" in out and "FRAME_EQUAL True True" in out and "HEADER_ONLY_EQUAL True" in out


def test_e2e_conform_alone_still_refuses_the_study(e2e):
    tmp, out = e2e
    assert any(ln.startswith("S: skipped") and "must share one shape" in ln for ln in out.splitlines())
    assert not os.path.exists(tmp / "out_conform" / "S.nii.gz")
