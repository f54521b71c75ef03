"""The bias-field kernels on the MI355X (gts/bias.py, csrc/gts_bias.hip) against tests/bias_ref.py:
Z1 to one float32 ulp, Z2 bit for bit, Z3 integer for integer (which pins the field's arithmetic), Z4 and the mean to
rounding bounds derived below, Z5 to one float32 ulp, then the whole loop on the phantom and the command lines.

Volumes are [Z, Y, X] arrays here, as the kernels hold them; the shapes are listed (X, Y, Z)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bias_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gnn-tumor-seg_amd")
DEV = "cuda"
EPS = 2.0 ** -53

# (1,1,1); rows shorter than a wave; one voxel longer than a wave; longer, over more than one workgroup of four rows;
# 67 * 5 rows of 72
SHAPES = [(1, 1, 1), (5, 6, 7), (65, 3, 18), (70, 37, 3), (72, 5, 67)]
# (spans0, levels): one level of 1, 2 and 8 spans (8 exceeds some extents: cells without a voxel), and two sets of three
LATTICES = [(1, 1), (2, 1), (8, 1), (1, 3), (2, 3)]
MASKS = ("half", "single", "none")
GRIDS = (0, 1, 3, 2048)            # the library's choice; one workgroup strides over every row; more than the rows need


@functools.lru_cache(maxsize=None)
def case(shape, spans0, levels, mask):
    """One input, made once and shared: u, its lattices, and what the reference makes of them."""
    rng = np.random.default_rng([*shape, spans0, levels, MASKS.index(mask)])
    zyx = shape[::-1]
    u = (6.0 + 0.5 * rng.standard_normal(zyx)).astype(np.float32)
    if mask == "half":
        u[rng.random(zyx) < 0.5] = np.nan
    elif mask == "single":
        keep = tuple(int(rng.integers(0, n)) for n in zyx)
        value = u[keep]
        u[...] = np.nan
        u[keep] = value
    else:
        u[...] = np.nan
    lattices = [rng.uniform(-0.3, 0.3, (R.points(spans0, k),) * 3) for k in range(levels)]
    d, inside = R.residual_image(u, lattices, spans0)
    lo, hi = R.value_range(d, inside)
    for a in (u, d, inside, *lattices):
        a.setflags(write=False)
    return u, lattices, d, inside, lo, hi


def device_case(shape, spans0, levels, mask):
    from gts import bias

    u, lattices = case(shape, spans0, levels, mask)[:2]
    tab = bias.tables(shape, spans0, levels, DEV)
    lat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in lattices])).to(DEV)
    return torch.from_numpy(u.copy()).to(DEV), tab, lat


def bin_range(lo, hi):
    """The histogram's range for a case: the mask's own where it has one, else one around it."""
    if hi > lo:
        return float(lo), float(hi)
    return (float(lo) - 0.25, float(lo) + 0.5) if np.isfinite(lo) else (-1.0, 1.0)


def assert_within_one_ulp(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    nan, inf = np.isnan(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[inf], want[inf]), what
    ok = ~(nan | inf)
    gap = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    assert (gap <= np.spacing(np.abs(want[ok])).astype(np.float64)).all(), (what, gap.max())


# ---- Z1 --------------------------------------------------------------------------------------------------------------

def _volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    zyx = shape[::-1]
    if dtype == np.int16:
        return rng.integers(-50, 3000, zyx).astype(np.int16)
    v = (rng.uniform(-10.0, 3000.0, zyx) * rng.choice([1.0, 1e-3, 1e-30], zyx)).astype(np.float32)
    flat = v.reshape(-1)
    specials = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42, 37.5, 3.0e38]
    flat[rng.integers(0, flat.size, len(specials))] = specials if flat.size > 1 else specials[:1]
    return v


@pytest.mark.parametrize("shape", SHAPES)
def test_log_image_has_the_exact_mask_and_values_within_one_ulp(hip_lib, shape):
    from gts import ops

    for dtype in (np.int16, np.float32):
        v = _volume(shape, dtype, 1)
        for threshold in (0.0, 37.5):
            want = R.log_image(v, threshold)
            u, count = ops.bias_log(torch.from_numpy(v).to(DEV), threshold)
            assert u.dtype == torch.float32 and tuple(u.shape) == v.shape
            assert_within_one_ulp(u.cpu().numpy(), want, (shape, dtype, threshold))
            assert int(count.item()) == int((~np.isnan(want)).sum())


# ---- Z2, Z3 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_range_is_bit_equal_and_counts_are_integer_equal_at_every_grid(hip_lib, shape):
    from gts import ops

    for spans0, levels in LATTICES:
        for mask in MASKS:
            u, _, d, inside, lo, hi = case(shape, spans0, levels, mask)
            dev_u, tab, lat = device_case(shape, spans0, levels, mask)
            b_lo, b_hi = bin_range(lo, hi)
            want = R.histogram(d, inside, b_lo, b_hi)
            tight = (b_lo + 0.25 * (b_hi - b_lo), b_hi - 0.25 * (b_hi - b_lo))         # both end bins collect a tail
            want_tight = R.histogram(d, inside, *tight)
            assert want.sum() == inside.sum() == want_tight.sum()
            for grid in GRIDS:
                got = ops.bias_range(dev_u, tab, lat, grid_blocks=grid).cpu().numpy()
                assert got.tobytes() == np.array([lo, hi], dtype=np.float64).tobytes(), (spans0, levels, mask, grid)
                counts = ops.bias_histogram(dev_u, tab, lat, b_lo, b_hi, grid_blocks=grid)
                assert counts.dtype == torch.int64 and tuple(counts.shape) == (R.BINS,)
                assert np.array_equal(counts.cpu().numpy(), want), (spans0, levels, mask, grid)
                counts = ops.bias_histogram(dev_u, tab, lat, *tight, grid_blocks=grid).cpu().numpy()
                assert np.array_equal(counts, want_tight), (spans0, levels, mask, grid)


def test_bad_operands_are_refused_before_any_launch(hip_lib):
    from gts import _lib, bias, ops

    shape = (5, 6, 7)
    dev_u, tab, lat = device_case(shape, 2, 1, "half")
    with pytest.raises(_lib.GtsError):
        ops.bias_histogram(dev_u, tab, lat, 1.0, 1.0)                        # hi == lo: the loop has ended
    with pytest.raises(_lib.GtsError):
        ops.bias_histogram(dev_u, tab, lat, float("nan"), 1.0)
    with pytest.raises(_lib.GtsError):
        ops.bias_histogram(dev_u, tab, lat, 0.0, float("inf"))
    table = np.linspace(0.0, 1.0, R.BINS)
    table[17] = np.nan
    with pytest.raises(_lib.GtsError):
        ops.bias_fit(dev_u, tab, lat, 0, 0.0, 1.0, table)
    with pytest.raises(_lib.GtsError):
        ops.bias_fit(dev_u, tab, lat, 1, 0.0, 1.0, np.linspace(0.0, 1.0, R.BINS))    # the set has one level
    with pytest.raises(_lib.GtsError):
        ops.bias_range(dev_u.cpu(), tab, lat)                                # no CPU route
    with pytest.raises(_lib.GtsError):
        ops.bias_range(dev_u, tab, lat[:-1])
    with pytest.raises(_lib.GtsError):
        ops.bias_range(dev_u[:, :, :4].contiguous(), tab, lat)
    with pytest.raises(_lib.GtsError):
        ops.bias_log(dev_u, -1.0)
    with pytest.raises(_lib.GtsError):
        ops.bias_log(dev_u.to(torch.float64))
    with pytest.raises(_lib.GtsError):
        ops.bias_apply(dev_u, tab, lat, float("nan"))
    with pytest.raises(ValueError):
        bias.tables(shape, 8, 4, DEV)                                        # 64 spans
    with pytest.raises(ValueError):
        bias.correct_volume(torch.zeros((7, 6, 5), dtype=torch.int16, device=DEV))      # an empty mask


# ---- Z4 --------------------------------------------------------------------------------------------------------------

def _table(d, inside, lo, hi):
    """The sharpened table of a case; a smooth stand-in where the mask is empty."""
    if inside.any():
        return R.sharpen(R.histogram(d, inside, lo, hi), lo, hi)
    return lo + 0.9 * (hi - lo) * np.linspace(0.0, 1.0, R.BINS) ** 2


@pytest.mark.parametrize("shape", SHAPES)
def test_fit_is_reproducible_and_within_its_rounding_bound(hip_lib, shape):
    """The bound.  Reference and kernel form the residual r of a voxel by the same float64 expression from the same d,
    so every term t = pz py px r of num[c][b][a] has the same inputs on both sides, up to the weights: gts.bias
    tabulates p = ((B B) B) / sum B^2 and the reference B ** 3 / sum B^2, each within 7 roundings of the true value,
    so a product of three differs by at most 42 relative roundings between the two.  Either side then rounds each term's
    three products and adds the n terms of an entry in an order of its own; whatever the order, a sum of n terms
    passes each term through at most n - 1 additions, so each side is within (n + 2) 2^-53 sum|t| of the exact sum (to
    first order; the factor 1.001 covers the higher orders for n < 2^31).  Hence
        |num_gpu - num_ref| <= 1.001 (2 n + 48) 2^-53 sum|t|,
    with n the number of mask voxels on the control point and sum|t| = sum pz py px |r|, both taken from the reference.
    den is the same with t = qz qy qx >= 0, so sum|t| is den itself.  For delta = num / den with errors e_n, e_d within
    those bounds b_n, b_d:  |n_g / d_g - n_r / d_r| = |e_n d_r - n_r e_d| / (d_g d_r) <= (b_n + |delta_r| b_d) / (d_r -
    b_d), plus one rounding of each side's division, 2 * 2^-53 |delta| (1.001 again for the higher orders).  Where no
    mask voxel sits on a control point both sums are empty: num, den and delta are exactly 0."""
    from gts import ops

    for spans0, levels in LATTICES:
        for mask in MASKS:
            u, lattices, d, inside, lo, hi = case(shape, spans0, levels, mask)
            dev_u, tab, lat = device_case(shape, spans0, levels, mask)
            lo, hi = bin_range(lo, hi)
            table = _table(d, inside, lo, hi)
            for level in range(levels):
                want = R.fit(R.residual(d, inside, lo, hi, table), inside, spans0 << level)
                got = ops.bias_fit(dev_u, tab, lat, level, lo, hi, table)
                n = R.points(spans0, level)
                assert got.dtype == torch.float64 and tuple(got.shape) == (3, n, n, n)
                for grid in GRIDS + (0,):
                    again = ops.bias_fit(dev_u, tab, lat, level, lo, hi, table, grid_blocks=grid)
                    assert torch.equal(got.view(torch.int64), again.view(torch.int64)), (spans0, levels, mask, level, grid)
                num, den, delta = got.cpu().numpy()
                where = (shape, spans0, levels, mask, level)
                factor = 1.001 * (2.0 * want["terms"] + 48.0) * EPS
                b_n, b_d = factor * want["abs_num"], factor * want["den"]
                assert (np.abs(num - want["num"]) <= b_n).all(), (where, np.abs(num - want["num"]).max())
                assert (np.abs(den - want["den"]) <= b_d).all(), (where, np.abs(den - want["den"]).max())
                empty = want["terms"] == 0
                assert not num[empty].any() and not den[empty].any() and not delta[empty].any(), where
                if shape == (5, 6, 7) and spans0 << level == 8:
                    assert empty.any(), where                                  # 8 spans over 5 voxels: cells without one
                zero = want["den"] == 0
                assert np.array_equal(den == 0, zero) and not delta[zero].any(), where
                safe = np.where(zero, 1.0, want["den"])
                b_delta = 1.001 * ((b_n + np.abs(want["delta"]) * b_d) / (safe - b_d) + 2.0 * EPS * np.abs(want["delta"]))
                miss = np.abs(delta - want["delta"])[~zero] - b_delta[~zero]
                assert (miss <= 0).all(), (where, miss.max())


# ---- Z5 --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_mean_is_within_its_bound_and_apply_within_one_ulp(hip_lib, shape):
    """The mean's bound: both sides add the same n float64 field values (the field's bits are pinned by Z2 and Z3) in
    their own order, each within (n - 1) 2^-53 sum|f| of the exact sum, so the sums differ by at most 1.001 * 2 n 2^-53
    sum|f|; the mean adds one rounding of each side's division."""
    from gts import ops

    for spans0, levels in LATTICES:
        for mask in MASKS:
            u, lattices, d, inside, lo, hi = case(shape, spans0, levels, mask)
            dev_u, tab, lat = device_case(shape, spans0, levels, mask)
            f = R.field(lattices, u.shape, spans0)
            n = int(inside.sum())
            first = ops.bias_mean(dev_u, tab, lat)
            for grid in GRIDS:
                assert torch.equal(first.view(torch.int64), ops.bias_mean(dev_u, tab, lat, grid_blocks=grid).view(torch.int64))
            total, count, mean = first.cpu().numpy()
            assert count == n
            if n == 0:
                assert total == 0.0 and mean == 0.0
                want_mean = 0.0
            else:
                want_mean = R.mask_mean(f, inside)
                b_sum = 1.001 * 2.0 * n * EPS * np.abs(f[inside]).sum()
                assert abs(total - f[inside].sum()) <= b_sum, (shape, spans0, levels, mask)
                assert abs(mean - want_mean) <= b_sum / n + 2.002 * EPS * abs(want_mean), (shape, spans0, levels, mask)
            for dtype in (np.int16, np.float32):
                v = _volume(shape, dtype, 3)
                want_out, want_field = R.apply(v, f, want_mean)
                for grid in (0, 3):
                    out, field = ops.bias_apply(torch.from_numpy(v).to(DEV), tab, lat, want_mean, want_field=True,
                                                grid_blocks=grid)
                    assert_within_one_ulp(out.cpu().numpy(), want_out, (shape, spans0, levels, dtype, "out"))
                    assert_within_one_ulp(field.cpu().numpy(), want_field, (shape, spans0, levels, dtype, "field"))
                alone = ops.bias_apply(torch.from_numpy(v).to(DEV), tab, lat, want_mean)
                assert torch.equal(alone.view(torch.int32), out.view(torch.int32))


# ---- the loop --------------------------------------------------------------------------------------------------------

# How far the GPU loop's rms residual against the true field may lie from the reference loop's on the same phantom.
# The two loops differ only where last-bit differences of the fit flip a voxel's histogram bin later on.  Measured on
# the MI355X the gap is 0: the float32 field volumes of the two loops are equal voxel for voxel, although the
# control points differ in their last bits.  The smallest gap rounding can then cause is a field value that rounds to
# the neighbouring float32: one ulp of a |log field| below 0.5 is 2^-25 = 3e-8, and the rms moves by no more than the
# largest change of a voxel.  The margin is three such steps (profiles/bias/README.md); a bin flip that mattered
# would move control points by far more and is a finding.
RMS_MARGIN = 1e-7


def test_loop_on_the_phantom_matches_the_reference_loop(hip_lib):
    from gts import bias

    v, clean, truth, classes = R.phantom((36, 40, 48), 0)
    inside = classes > 0
    _, ref_field, ref_report = R.correct_volume(v, levels=3, iterations=30)
    out, field, report = bias.correct_volume(torch.from_numpy(v).to(DEV), levels=3, iterations=30, want_field=True)
    ref_corr, ref_rms = R.score(ref_field, truth, inside)
    corr, rms = R.score(field.cpu().numpy(), truth, inside)
    cv_in, cv_out, cv_clean = R.class_cv(v, classes), R.class_cv(out.cpu().numpy(), classes), R.class_cv(clean, classes)
    print(f"phantom 48x40x36: gpu corr {corr:.6f} rms {rms:.6e}; reference corr {ref_corr:.6f} rms {ref_rms:.6e}; "
          f"gap {abs(rms - ref_rms):.3e}; field difference max {np.abs(field.cpu().numpy() - ref_field)[inside].max():.3e}; "
          f"cv {cv_in} -> {cv_out} (clean {cv_clean}); levels {report['levels']}")
    assert ref_corr >= 0.995 and ref_rms <= 0.01
    assert corr >= 0.995
    assert abs(rms - ref_rms) <= RMS_MARGIN
    assert [r["iterations"] for r in report["levels"]] == [r["iterations"] for r in ref_report]
    assert report["mask_voxels"] == int(inside.sum()) and report["field_ratio_min"] < 1.0 < report["field_ratio_max"]
    assert all(a < b for a, b in zip(cv_out, cv_in))


# ---- the command lines: one child process writes a small biased study and runs the scripts on it ---------------------

MODS = ("_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz")
STUDY_SHAPE = (36, 40, 48)            # [Z, Y, X]
FEW = ["--bias_levels", "3", "--bias_iterations", "10"]


def study_affine():
    from tests import conform_ref as C

    return C.make_affine((0, 1, 2), (1, 1, 1), origin=(-23.5, -19.5, -17.5))     # RAS, 1 mm


_E2E = r"""
import os, sys
import numpy as np, torch
from data_processing import nifti_io
from model.networks import init_graph_net
from utils.hyperparam_helpers import EvalParamSet
from scripts import bias_correct, compute_dataset_stats, preprocess_dataset, segment_scans
from tests import bias_ref as R
from tests import test_gpu_bias as T
tmp = sys.argv[1]
raw = os.path.join(tmp, "raw")
os.makedirs(os.path.join(raw, "S"))
for c, ext in enumerate(T.MODS):
    v = R.phantom(T.STUDY_SHAPE, 40 + c)[0]
    nifti_io.save_as_nifti(np.asfortranarray(np.rint(v).astype(np.int16).T), os.path.join(raw, "S", "S" + ext),
                           affine=T.study_affine())
seg = np.where(R.phantom(T.STUDY_SHAPE, 40)[3] == 3, 4, 0).astype(np.int16)           # the core as tumour, the rest healthy
nifti_io.save_as_nifti(np.asfortranarray(seg.T), os.path.join(raw, "S", "S_seg.nii.gz"), affine=T.study_affine())
torch.manual_seed(0)
hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
gnn = os.path.join(tmp, "gnn.pt")
torch.save(init_graph_net("GSpool", hp).state_dict(), gnn)
j = lambda *p: os.path.join(tmp, *p)
rc1 = bias_correct.main(["-d", raw, "-o", j("corrected"), "--save_field", "--bias_report", j("tool.json")] + T.FEW)
common = ["-d", raw, "-g", gnn, "-n", "400", "--conform"]
rc2 = segment_scans.main(common + ["-o", j("seg_bias"), "--bias_correct", "--bias_report", j("seg.json")] + T.FEW)
rc3 = segment_scans.main(common + ["-o", j("seg_plain")])
# the same command through the code with the flags absent altogether, as a caller from before they existed built it
args = segment_scans.parse_args(common + ["-o", j("seg_absent")])
for name in [n for n in vars(args) if n.startswith("bias")]:
    delattr(args, name)
scans = segment_scans.find_inputs(args.data_dir, args.modality_extensions, args.data_prefix)
rc4 = len(segment_scans.Segmenter(args).run(scans, args.output_dir))
print("RC", rc1, rc2, rc3, rc4)
# the training side takes the same flags: statistics and graphs of the corrected scans
rc5 = compute_dataset_stats.main(["-d", raw, "-l", "_seg.nii.gz", "-o", j("stats_bias.json"), "--bias_correct"] + T.FEW)
rc6 = compute_dataset_stats.main(["-d", raw, "-l", "_seg.nii.gz", "-o", j("stats_plain.json")])
rc7 = preprocess_dataset.main(["-d", raw, "-l", "_seg.nii.gz", "-o", j("ds"), "-n", "400", "--bias_correct",
                               "--bias_report", j("prep.json")] + T.FEW)
print("TRAINING_RC", rc5, rc6, rc7)
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, hip_lib):
    tmp = tmp_path_factory.mktemp("bias_e2e")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-c", _E2E, str(tmp)], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=500)
    assert r.returncode == 0 and "RC 0 0 0 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)
    return tmp, r.stdout


def test_bias_correct_tool_keeps_the_affine_and_evens_out_each_class(e2e):
    from data_processing import nifti_io

    tmp, out = e2e
    for c, ext in enumerate(MODS):
        src, dst = str(tmp / "raw" / "S" / ("S" + ext)), str(tmp / "corrected" / "S" / ("S" + ext))
        assert np.array_equal(nifti_io.read_affine(dst)[0], nifti_io.read_affine(src)[0])
        assert np.array_equal(nifti_io.read_affine(dst)[0], study_affine())
        before, after = nifti_io.read_nifti_raw(src), nifti_io.read_nifti_raw(dst)
        assert after.dtype == np.float32 and after.shape == before.shape == STUDY_SHAPE[::-1]
        classes = R.phantom(STUDY_SHAPE, 40 + c)[3].T
        cv_in, cv_out = R.class_cv(before, classes), R.class_cv(after, classes)
        print(ext, cv_in, "->", cv_out)
        assert all(b < a for a, b in zip(cv_in, cv_out)), (ext, cv_in, cv_out)
        field = nifti_io.read_nifti_raw(str(tmp / "corrected" / "S" / ("S" + ext.split(".")[0] + "_biasfield.nii.gz")))
        inside = before > 0
        assert np.allclose(after[inside] * field[inside], before[inside], rtol=1e-5)
    with open(tmp / "tool.json") as f:
        report = json.load(f)
    assert report["settings"]["levels"] == 3 and list(report["scans"]) == ["S"] and len(report["scans"]["S"]) == 4
    assert all([lv["iterations"] for lv in row["levels"]] == [10, 10, 10] for row in report["scans"]["S"])


def test_segment_scans_with_bias_correct_runs_end_to_end(e2e):
    from data_processing import nifti_io

    tmp, out = e2e
    fp = str(tmp / "seg_bias" / "S.nii.gz")
    labels = nifti_io.read_nifti_raw(fp)
    assert labels.dtype == np.int16 and labels.shape == STUDY_SHAPE[::-1]
    assert np.array_equal(nifti_io.read_affine(fp)[0], study_affine())
    assert set(np.unique(labels).tolist()) <= {0, 1, 2, 4}
    done = [ln for ln in out.splitlines() if ln.startswith("S: done (conform:") and "bias: field x" in ln]
    assert len(done) == 1                       # this run's line carries both notes; the plain runs' carry no bias note
    with open(tmp / "seg.json") as f:
        report = json.load(f)
    rows = report["scans"]["S"]
    assert len(rows) == 4 and all(r["field_ratio_min"] < 1.0 < r["field_ratio_max"] for r in rows)


def test_segment_scans_without_the_flag_writes_the_same_bytes_as_before(e2e):
    tmp, out = e2e
    with open(tmp / "seg_plain" / "S.nii.gz", "rb") as a, open(tmp / "seg_absent" / "S.nii.gz", "rb") as b:
        plain, absent = a.read(), b.read()
    assert plain == absent and len(plain) > 348
    assert not any("bias" in ln for ln in out.splitlines() if ln.startswith("S: done") and "bias: field x" not in ln)


def test_statistics_and_graphs_take_the_same_correction(e2e):
    tmp, out = e2e
    assert "TRAINING_RC 0 0 0" in out
    with open(tmp / "stats_bias.json") as f:
        corrected = json.load(f)
    with open(tmp / "stats_plain.json") as f:
        plain = json.load(f)
    assert corrected != plain                              # the healthy tissue's spread shrinks with the field gone
    with open(tmp / "prep.json") as f:
        report = json.load(f)
    assert list(report["scans"]) == ["S"] and len(report["scans"]["S"]) == 4
    assert os.path.exists(tmp / "ds" / "S" / "S_input.nii.gz") and os.path.exists(tmp / "ds" / "S" / "S_nxgraph.json")
    assert any(ln.startswith("S: done (bias: field x") for ln in out.splitlines())
