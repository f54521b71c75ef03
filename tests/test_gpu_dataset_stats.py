"""Dataset standardization statistics on the MI355X: the D1-D3 kernels (gts.dataset_stats.scan_stats) against
the exact form of the numpy restatement and against the reference fixture, their determinism and errors, and
the three command line tools end to end.

Bounds.  n and the tops are exact (the tops byte-equal to numpy's float32 quantiles).  The mean and the
standard deviation are float64 accumulations of n <= 2^24 non-negative terms: relative error below
n * 2^-53 < 2e-9 for any summation order (the kernels' blocked order passes a value through about 110
additions at BraTS size, so 1.2e-14), the one-pass variance losing about 7 more bits at
var / mean^2 ~ 1e-2.  That is far below half a float32 ulp (6e-8), so after the single rounding to float32
they lie within 1 float32 ulp of the exact form (the 1 ulp allows for the rounding landing on the other side
of a tie).  Against the reference's float32-accumulated
values the triangle inequality gives |gpu - ref| <= |ref - exact| + 1 ulp, with no tolerance of its own.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dataset_stats_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gnn-tumor-seg_amd")
MODS = ["_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"]


def _within_one_ulp(got32, exact64):
    assert got32.dtype == np.float32
    err = np.abs(got32.astype(np.float64) - exact64)
    return bool((err <= R.ulp32(exact64)).all()), err / R.ulp32(exact64)


def _check(vols, lab):
    from gts import dataset_stats

    got = dataset_stats.scan_stats(vols, lab)
    n, top, mean, std = R.exact_form(R.stack(vols), lab)
    print(f"n {got.n} (want {n}); top {got.top} (want {top})")
    assert got.n == n
    assert got.top.dtype == np.float32 and got.top.tobytes() == top.tobytes(), (got.top, top)
    ok_mean, ulps_mean = _within_one_ulp(got.mean, mean)
    ok_std, ulps_std = _within_one_ulp(got.std, std)
    print(f"mean {got.mean} exact {mean} off by {ulps_mean} ulp; std {got.std} exact {std} off by {ulps_std} ulp")
    assert ok_mean, (got.mean, mean, ulps_mean)
    assert ok_std, (got.std, std, ulps_std)
    return got


def _synth(shape, seed):
    from gts import synth_mri

    img, lab = synth_mri.make_sample(seed, shape)
    return [img[..., c] for c in range(4)], lab


def full_size_inputs():
    vols, lab = _synth((240, 240, 155), 7)
    ints = [np.asfortranarray(v.astype(np.int16)) for v in vols]
    rng = np.random.default_rng(7)
    cont = [np.asfortranarray(np.where(v > 0, v + rng.uniform(0, 1, v.shape).astype(np.float32), 0.0)
                              .astype(np.float32)) for v in vols]
    return (ints, lab), (cont, lab)


def odd_shape_inputs():
    rng = np.random.default_rng(11)
    for shape in [(1, 1, 1), (7, 5, 3), (33, 17, 9), (65, 3, 18)]:
        vols = []
        for c in range(4):
            v = rng.uniform(-50.0, 200.0, shape).astype(np.float32)
            v[rng.random(shape) < 0.4] = 0.0
            v.flat[0] = 1.0 + c                    # a member voxel whose every channel is positive
            vols.append(np.asfortranarray(v))
        lab = rng.choice(np.array([0, 0, 1, 2, 4], dtype=np.int16), shape)
        lab.flat[0] = 0
        yield vols, lab
        yield [np.asfortranarray(np.rint(v).astype(np.int16)) for v in vols], lab


def few_member_inputs():
    shape = (9, 7, 5)
    rng = np.random.default_rng(3)
    for n in (1, 2, 3):
        vols = [np.asfortranarray(rng.uniform(1.0, 100.0, shape).astype(np.float32)) for _ in range(4)]
        lab = np.full(shape, 2, dtype=np.int16)
        for k, at in enumerate([(4, 3, 2), (0, 0, 0), (8, 6, 4)][:n]):
            lab[at] = 0
            for c in range(4):
                vols[c][at] = 10.0 * (k + 1) + c           # well separated members
        yield n, vols, lab


def sparse_label_inputs():
    vols, _ = _synth((64, 60, 40), 3)
    rng = np.random.default_rng(4)
    lab = np.where(rng.random((64, 60, 40)) < 0.005, 0, 2).astype(np.int16)     # nonzero almost everywhere
    return [np.asfortranarray(v.astype(np.int16)) for v in vols], lab


def threshold_inputs():
    shape = (16, 12, 10)
    rng = np.random.default_rng(6)
    t = np.float32(0.001)
    around = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), 0.0011, 0.0009, 0.0, -0.002,
                       0.5, 3.0], dtype=np.float32)
    ch0 = rng.choice(around, shape)
    vols = [np.asfortranarray(ch0)] + [np.asfortranarray(rng.uniform(0.5, 9.0, shape).astype(np.float32))
                                       for _ in range(3)]
    lab = rng.choice(np.array([0, 0, 0, 1], dtype=np.int16), shape)
    return vols, lab


def radix_bucket_inputs():
    """test_intake_ranks_in_different_radix_buckets' construction restricted to the members: 200 members whose
    ranks 198 and 199 differ in the top radix digit, among 200 non-members that hold larger values still."""
    from gts import intake

    shape = (10, 10, 4)
    rng = np.random.default_rng(5)
    vols = [np.asfortranarray(rng.uniform(1.0, 100.0, shape).astype(np.float32)) for _ in range(4)]
    lab = np.zeros(shape, dtype=np.int16)
    lab[:, :, 1::2] = 4                                    # every other z plane is outside the mask
    n = 200
    lo, hi = intake.quantile_ranks(n)
    assert (lo, hi) == (198, 199)
    for c, big in enumerate([1e6, 3e4, 2.5e9, 7e5]):
        vols[c][:, :, 1::2] = np.float32(3e30)             # would be the top two ranks if it were counted
        vols[c][0, 0, 0] = np.float32(big)                 # rank hi of the members lands on a big value
    return vols, lab, (lo, hi)


@pytest.mark.timeout(300)
def test_full_size_int16_and_float32(hip_lib):
    for vols, lab in full_size_inputs():
        _check(vols, lab)


@pytest.mark.timeout(300)
def test_small_odd_shapes(hip_lib):
    for vols, lab in odd_shape_inputs():
        _check(vols, lab)


@pytest.mark.timeout(300)
def test_masks_of_one_two_and_three_voxels(hip_lib):
    for n, vols, lab in few_member_inputs():
        assert _check(vols, lab).n == n


@pytest.mark.timeout(300)
def test_labels_nonzero_almost_everywhere(hip_lib):
    vols, lab = sparse_label_inputs()
    got = _check(vols, lab)
    assert 0 < got.n < 0.005 * lab.size


@pytest.mark.timeout(300)
def test_first_channel_straddles_the_threshold(hip_lib):
    vols, lab = threshold_inputs()
    t = np.float32(0.001)
    assert (vols[0] == t).any() and (vols[0] == np.nextafter(t, np.float32(1))).any()
    got = _check(vols, lab)
    assert got.n == int(((vols[0] > t) & (lab == 0)).sum())


@pytest.mark.timeout(300)
def test_ranks_in_different_radix_buckets(hip_lib):
    vols, lab, (lo, hi) = radix_bucket_inputs()
    for c in range(4):
        s = np.sort(vols[c][lab == 0])
        assert len(s) == 200 and (s[lo].view(np.uint32) >> 24) != (s[hi].view(np.uint32) >> 24)
    _check(vols, lab)


@pytest.mark.timeout(300)
def test_two_runs_give_identical_bytes(hip_lib):
    from gts import dataset_stats

    for vols, lab in full_size_inputs():
        sums = []
        a = dataset_stats.scan_stats(vols, lab, sums=sums)
        b = dataset_stats.scan_stats(vols, lab, sums=sums)
        assert a.n == b.n
        for name in ("top", "mean", "std"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        assert sums[0].dtype == np.float64 and sums[0].shape == (4, 4)
        assert sums[0].tobytes() == sums[1].tobytes()          # the device's float64 sums, mean and std


@pytest.mark.timeout(600)
def test_against_the_reference_fixture(hip_lib, golden_dir):
    """|gpu - ref| <= |ref - exact| + 1 ulp for every scan and channel; prints how far the reference's float32
    accumulation drifts from the exact form (the maxima are recorded in DESIGN.md 4l)."""
    from gts import dataset_stats, synth_mri

    fx = np.load(f"{golden_dir}/ref_dataset_stats.npz")
    drift_mean = drift_std = 0.0
    per_scan = []
    for i, (seed, shape) in enumerate(R.FIXTURE_SCANS):
        img, lab = synth_mri.make_sample(seed, shape)
        assert R.digest(img) == str(fx["image_digests"][i])
        vols = [np.asfortranarray(img[..., c].astype(np.int16)) for c in range(4)]
        got = dataset_stats.scan_stats(vols, lab)
        per_scan.append(got)
        _, _, mean, std = R.exact_form(img, lab)
        for name, g, ref, exact in (("mean", got.mean, fx["scan_mean"][i], mean), ("std", got.std, fx["scan_std"][i], std)):
            ref64 = ref.astype(np.float64)
            drift = np.abs(ref64 - exact)
            gap = np.abs(g.astype(np.float64) - ref64)
            print(f"scan {i} {shape} {name}: gpu {g} ref {ref} exact {exact} reference drift {drift / np.abs(exact)} relative")
            assert (gap <= drift + R.ulp32(exact)).all(), (i, name, gap, drift)
        drift_mean = max(drift_mean, float(np.max(np.abs(fx["scan_mean"][i] - mean) / np.abs(mean))))
        drift_std = max(drift_std, float(np.max(np.abs(fx["scan_std"][i] - std) / np.abs(std))))
    print(f"reference float32 drift, maxima over scans and channels: mean {drift_mean:.3e}, std {drift_std:.3e} relative")
    mean, std = dataset_stats.dataset_stats(per_scan)
    assert mean.dtype == np.float32 and mean.shape == (4,) and std.shape == (4,)


@pytest.mark.timeout(300)
def test_errors_raise_and_leave_the_device_usable(hip_lib):
    from gts import dataset_stats

    vols, lab = _synth((33, 17, 9), 12)
    vols = [np.asfortranarray(v) for v in vols]
    with pytest.raises(ValueError, match="no healthy-tissue voxel"):
        dataset_stats.scan_stats(vols, np.ones_like(lab))                    # empty mask
    dark = [v.copy(order="F") for v in vols]
    dark[2][...] = 0.0
    with pytest.raises(ValueError, match="not positive"):
        dataset_stats.scan_stats(dark, lab)                                  # a zero top
    member = tuple(np.argwhere((vols[0] > 0.001) & (lab == 0))[5])
    inside = [v.copy(order="F") for v in vols]
    inside[1][member] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        dataset_stats.scan_stats(inside, lab)                                # a NaN inside the mask
    inside[1][member] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        dataset_stats.scan_stats(inside, lab)
    outside = [v.copy(order="F") for v in vols]
    tumour = tuple(np.argwhere(lab != 0)[0])
    background = tuple(np.argwhere(vols[0] == 0)[0])
    outside[3][tumour] = np.nan
    outside[0][background] = np.nan                                          # NaN > 0.001 is false: not a member
    _check(outside, lab)                                                     # a NaN outside the mask does not
    with pytest.raises(ValueError, match="differ in shape"):
        dataset_stats.scan_stats(vols, lab[:-1])
    torch.cuda.synchronize()
    _check(vols, lab)                                                        # and no error state is left behind


_SMALL_SHAPES = [(48, 40, 32), (40, 48, 36), (36, 40, 32), (44, 36, 40), (40, 40, 40)]

# preprocess_dataset (file and compute) and compute_dataset_stats over 5 small scans, in one process
_CLI = r"""
import io, os, sys
from contextlib import redirect_stdout
from gts import synth_mri
from scripts import compute_dataset_stats, preprocess_dataset
tmp = sys.argv[1]
raw = os.path.join(tmp, "raw")
shapes = %r
for i, shape in enumerate(shapes):
    synth_mri.write_sample(raw, f"BraTS_{i:03d}", 600 + i, shape=shape)
j = lambda *p: os.path.join(tmp, *p)
rc1 = compute_dataset_stats.main(["-d", raw, "-l", "_seg.nii.gz", "-o", j("stats.json")])
with redirect_stdout(io.StringIO()):
    rc2 = preprocess_dataset.main(["-d", raw, "-l", "_seg.nii.gz", "-o", j("ds_file"), "-n", "300", "--stats", j("stats.json")])
    rc3 = preprocess_dataset.main(["-d", raw, "-l", "_seg.nii.gz", "-o", j("ds_compute"), "-n", "300", "--stats", "compute"])
rc4 = preprocess_dataset.main(["-d", raw, "-o", j("ds_refused"), "-n", "300", "--stats", j("stats.json"),
                               "-m", "_t1.nii.gz", "_flair.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"])
print("RC", rc1, rc2, rc3, rc4)
""" % (_SMALL_SHAPES,)


@pytest.mark.timeout(1200)
def test_stats_and_preprocess_cli_end_to_end(hip_lib, tmp_path):
    from data_processing import nifti_io, standardization
    from data_processing.image_processing import determine_brain_crop, normalize_img, standardize_img
    from gts import dataset_stats, synth_mri

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-c", _CLI, str(tmp_path)], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=1100)
    assert r.returncode == 0 and "RC 0 0 0 2" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "same suffixes in the same order" in r.stderr and not os.path.exists(tmp_path / "ds_refused")

    doc = json.load(open(tmp_path / "stats.json"))
    assert doc["n_scans"] == 5 and doc["modality_extensions"] == MODS and doc["quantile"] == 0.995
    exact = []
    for i, shape in enumerate(_SMALL_SHAPES):
        sid = f"BraTS_{i:03d}"
        img, lab = synth_mri.make_sample(600 + i, shape)
        n, top, mean, std = R.exact_form(img, lab)
        exact.append((mean, std))
        scan = doc["scans"][sid]
        assert scan["n"] == n and np.float32(scan["top"]).tobytes() == top.tobytes()
        assert _within_one_ulp(np.float32(scan["mean"]), mean)[0] and _within_one_ulp(np.float32(scan["std"]), std)[0]
    # the medians of values that are each within 1 ulp of the exact ones lie within 1 ulp of the exact medians
    # (for an even count half the sum of two such values; here the count is odd)
    want_mean, want_std = np.median([m for m, _ in exact], axis=0), np.median([s for _, s in exact], axis=0)
    mean, std = standardization.load_stats(str(tmp_path / "stats.json"), MODS)
    assert _within_one_ulp(mean, want_mean)[0] and _within_one_ulp(std, want_std)[0]
    per_scan = [(np.float32(doc["scans"][s]["mean"]), np.float32(doc["scans"][s]["std"])) for s in sorted(doc["scans"])]
    got = dataset_stats.dataset_stats(per_scan)
    assert got[0].tobytes() == mean.tobytes() and got[1].tobytes() == std.tobytes()

    computed = open(tmp_path / "ds_compute" / "standardization.json").read()
    assert computed == open(tmp_path / "stats.json").read()
    for i, shape in enumerate(_SMALL_SHAPES):
        sid = f"BraTS_{i:03d}"
        img, _ = synth_mri.make_sample(600 + i, shape)
        want = standardize_img(normalize_img(img[determine_brain_crop(img)]), mean, std)
        for ds in ("ds_file", "ds_compute"):
            got_img = nifti_io.read_nifti_raw(str(tmp_path / ds / sid / f"{sid}_input.nii.gz"))
            assert got_img.dtype == np.float32 and np.array_equal(got_img, want), (sid, ds)
        for suffix in ("_nxgraph.json", "_label.nii.gz", "_supervoxels.nii.gz", "_crop.npz"):
            a = open(tmp_path / "ds_file" / sid / (sid + suffix), "rb").read()
            assert a == open(tmp_path / "ds_compute" / sid / (sid + suffix), "rb").read(), (sid, suffix)


# The segmenter writes volumes at BraTS size (uncrop_to_brats_size), so its comparison runs on one full-size scan;
# the statistics file is taken over that scan.  One process, as in test_gpu_segment.py.
_SEG = r"""
import io, os, sys
from contextlib import redirect_stdout
import torch
from gts import synth_mri
from model.networks import init_graph_net
from utils.hyperparam_helpers import EvalParamSet
from scripts import compute_dataset_stats, generate_gnn_predictions, preprocess_dataset, segment_scans
tmp = sys.argv[1]
raw = os.path.join(tmp, "raw")
synth_mri.write_sample(raw, "BraTS_000", 700)
j = lambda *p: os.path.join(tmp, *p)
torch.manual_seed(0)
hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
torch.save(init_graph_net("GSpool", hp).state_dict(), j("gnn.pt"))
rc1 = compute_dataset_stats.main(["-d", raw, "-l", "_seg.nii.gz", "-o", j("stats.json")])
with redirect_stdout(io.StringIO()):
    rc2 = preprocess_dataset.main(["-d", raw, "-o", j("ds"), "-n", "6000", "--stats", j("stats.json")])
    generate_gnn_predictions.main(["-d", j("ds") + "/", "-o", j("gnn"), "-w", j("gnn.pt"), "-f", "preds"])
    rc3 = preprocess_dataset.main(["-d", raw, "-o", j("ds_const"), "-n", "6000"])
    generate_gnn_predictions.main(["-d", j("ds_const") + "/", "-o", j("gnn_const"), "-w", j("gnn.pt"), "-f", "preds"])
rc4 = segment_scans.main(["-d", raw, "-o", j("seg"), "-g", j("gnn.pt"), "-n", "6000", "--stats", j("stats.json")])
rc5 = segment_scans.main(["-d", raw, "-o", j("seg_refused"), "-g", j("gnn.pt"), "-n", "6000", "--stats", j("stats.json"),
                          "-M", "_t1.nii.gz", "_flair.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"])
print("RC", rc1, rc2, rc3, rc4, rc5)
"""


@pytest.mark.timeout(1500)
def test_segmenter_with_stats_equals_two_step_pipeline(hip_lib, tmp_path):
    from data_processing import nifti_io

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-c", _SEG, str(tmp_path)], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=1400)
    assert r.returncode == 0 and "RC 0 0 0 0 2" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "same suffixes in the same order" in r.stderr and not os.path.exists(tmp_path / "seg_refused")
    want = nifti_io.read_nifti(str(tmp_path / "gnn" / "BraTS_000.nii.gz"), np.int16)
    got = nifti_io.read_nifti_raw(str(tmp_path / "seg" / "BraTS_000.nii.gz"))
    assert got.dtype == np.int16 and got.shape == (240, 240, 155)
    assert np.array_equal(got, want), int((got != want).sum())
    # the file's values were really used: the inputs differ from the ones standardized with the constants
    a = nifti_io.read_nifti_raw(str(tmp_path / "ds" / "BraTS_000" / "BraTS_000_input.nii.gz"))
    b = nifti_io.read_nifti_raw(str(tmp_path / "ds_const" / "BraTS_000" / "BraTS_000_input.nii.gz"))
    assert a.shape == b.shape and not np.array_equal(a, b)
