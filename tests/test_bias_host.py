"""The host side of the bias-field correction (gts/bias.py) and its numpy reference (tests/bias_ref.py),
without a GPU: the B-spline basis, the histogram sharpening, the reference loop on the phantom, the flags, and the
argument checks of the entry points."""
import ctypes

import numpy as np
import pytest

from tests import bias_ref as R


@pytest.mark.parametrize("n,spans", [(1, 1), (5, 8), (3, 32), (8, 8), (32, 32), (7, 2), (48, 4), (240, 8), (155, 32)])
def test_basis_rows_sum_to_one_and_equal_the_reference_bit_for_bit(n, spans):
    """Extents smaller than, equal to and not divisible by the spans.  The GPU tests compare histogram counts integer
    for integer, so the tables the device gets (gts.bias.basis) and the reference's own must be the same bits."""
    from gts import bias

    cell, w = bias.basis(n, spans)
    assert cell.dtype == np.int32 and w.dtype == np.float64 and w.shape == (n, 4)
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -52
    assert (w >= 0).all() and cell.min() == 0 and cell.max() <= spans - 1 and (np.diff(cell) >= 0).all()
    ref_cell, ref_w = R.basis(n, spans)
    assert np.array_equal(cell, ref_cell) and w.tobytes() == ref_w.tobytes()
    fit = bias.fit_weights(w)
    assert fit.shape == (8, n) and np.array_equal(fit[4:], (w * w).T)
    assert np.allclose(fit[:4], (w ** 3 / (w ** 2).sum(axis=1, keepdims=True)).T, rtol=1e-14, atol=0)


def two_peaks():
    i = np.arange(R.BINS)
    return np.rint(1000 * (np.exp(-(i - 60) ** 2 / (2 * 15.0 ** 2)) + 0.7 * np.exp(-(i - 140) ** 2 / (2 * 12.0 ** 2)))) + 1


def test_sharpen_equals_the_plain_dft_version():
    """numpy.fft against the reference's O(P^2) DFT: 1e-9 of the largest value (the values pass through 0, so the
    error is taken relative to the table's scale)."""
    from gts import bias

    counts = two_peaks()
    got, want = bias.sharpen(counts, -0.4, 0.5), R.sharpen(counts, -0.4, 0.5)
    assert got.shape == (R.BINS,) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # sharpening pulls the values of a blurred peak towards its centre: the table is steeper than the identity there
    centres = -0.4 + np.arange(R.BINS) * (0.9 / (R.BINS - 1))
    assert abs(got[60] - centres[60]) < 0.01 and got[40] > centres[40] and got[80] < centres[80]


def test_sharpen_of_a_one_bin_histogram_is_finite():
    from gts import bias

    one = np.zeros(R.BINS)
    one[37] = 500
    for lo, hi in ((0.0, 1.0), (-3.0, 40.0), (0.0, 1e-6)):
        assert np.isfinite(bias.sharpen(one, lo, hi)).all() and np.isfinite(R.sharpen(one, lo, hi)).all()
    assert np.isfinite(bias.sharpen(np.zeros(R.BINS), 0.0, 1.0)).all()


def test_reference_loop_recovers_the_phantoms_field():
    """48 x 40 x 36, seed 0, 3 levels of 30 rounds, as the definition was prototyped."""
    v, clean, truth, classes = R.phantom((36, 40, 48), 0)
    out, field, report = R.correct_volume(v, levels=3, iterations=30)
    corr, rms = R.score(field, truth, classes > 0)
    print(f"reference on the phantom: correlation {corr:.4f}, rms residual {rms:.4f}, levels {report}")
    assert corr >= 0.995 and rms <= 0.01
    assert all(after < before for after, before in zip(R.class_cv(out, classes), R.class_cv(v, classes)))
    assert np.array_equal(out == 0, classes == 0)


def test_flags_are_off_by_default_and_checked_before_any_scan_is_read(capsys):
    from gts import bias
    from scripts import bias_correct, compute_dataset_stats, preprocess_dataset, segment_scans

    base = ["-d", "/no/such/folder", "-o", "/no/such/out", "-g", "/no/such/weights.pt"]
    off = segment_scans.parse_args(base)
    assert off.bias_correct is False and off.bias is None and off.bias_report is None
    on = segment_scans.parse_args(base + ["--bias_correct"])
    assert on.bias == dict(levels=4, spans0=1, iterations=50, tol=1e-3, threshold=0.0)
    tuned = segment_scans.parse_args(base + ["--bias_correct", "--bias_levels", "2", "--bias_spans", "16",
                                             "--bias_iterations", "7", "--bias_tol", "0.01", "--bias_threshold", "5"])
    assert tuned.bias == dict(levels=2, spans0=16, iterations=7, tol=0.01, threshold=5.0)
    # 1 << 6 = 64 spans, 16 << 2 = 64: refused with status 2; the folder does not exist, so no scan was looked for
    for extra in (["--bias_levels", "7"], ["--bias_spans", "16", "--bias_levels", "3"], ["--bias_spans", "0"],
                  ["--bias_iterations", "0"], ["--bias_threshold", "-1"]):
        assert segment_scans.main(base + ["--bias_correct"] + extra) == 2
        assert "bias" in capsys.readouterr().err
        assert preprocess_dataset.main(["-d", "/no/such/folder", "-o", "/no/such/out", "--bias_correct"] + extra) == 2
        assert bias_correct.main(["-d", "/no/such/folder", "-o", "/no/such/out"] + extra) == 2
        with pytest.raises(SystemExit):
            compute_dataset_stats.main(["-d", "/no/such/folder", "-o", "/no/such/out.json", "-l", "_seg.nii.gz",
                                        "--bias_correct"] + extra)
    assert segment_scans.main(base + ["--bias_levels", "2"]) == 2                 # a setting without the switch
    assert "--bias_levels need --bias_correct" in capsys.readouterr().err
    with pytest.raises(ValueError):
        bias.check_levels(1, 7)
    bias.check_levels(1, 6)
    bias.check_levels(32, 1)


def test_entry_points_refuse_bad_arguments_without_a_gpu(hip_lib):
    from gts import ops

    one = ctypes.c_void_p(16)
    assert (ops.BIAS_BINS, ops.BIAS_MAX_SPANS) == (200, 32)
    assert hip_lib.gts_bias_workspace(240, 240, 155, 8) > 0
    assert hip_lib.gts_bias_workspace(240, 240, 155, 33) == -2 and hip_lib.gts_bias_workspace(0, 1, 1, 1) == -2
    assert hip_lib.gts_bias_workspace(65536, 1, 1, 1) == -2 and hip_lib.gts_bias_workspace(65535, 65535, 1, 1) == -2
    assert hip_lib.gts_bias_log(None, 4, 5, 5, 5, 0.0, one, one, None) == -1
    assert hip_lib.gts_bias_log(one, 2, 5, 5, 5, 0.0, one, one, None) == -3
    assert hip_lib.gts_bias_log(one, 4, 5, 5, 5, -1.0, one, one, None) == -3
    assert hip_lib.gts_bias_log(one, 4, 5, 5, 5, float("nan"), one, one, None) == -3
    assert hip_lib.gts_bias_log(one, 4, 5, 0, 5, 0.0, one, one, None) == -2
    basis = (one, one, one)
    assert hip_lib.gts_bias_range(one, 5, 5, 5, *basis, 8, 4, one, one, 1 << 30, 0, None) == -2       # 64 spans
    assert hip_lib.gts_bias_range(one, 5, 5, 5, *basis, 1, 7, one, one, 1 << 30, 0, None) == -2
    assert hip_lib.gts_bias_range(one, 5, 5, 5, *basis, 1, 4, one, one, 16, 0, None) == -2            # short workspace
    assert hip_lib.gts_bias_range(one, 5, 5, 5, *basis, 1, 4, one, one, 1 << 30, -1, None) == -2
    assert hip_lib.gts_bias_range(one, 5, 5, 5, one, None, one, 1, 4, one, one, 1 << 30, 0, None) == -1
    assert hip_lib.gts_bias_histogram(one, 5, 5, 5, *basis, 1, 4, 1.0, 1.0, one, 0, None) == -3
    assert hip_lib.gts_bias_histogram(one, 5, 5, 5, *basis, 1, 4, 0.0, float("inf"), one, 0, None) == -3
    assert hip_lib.gts_bias_histogram(one, 5, 5, 70000, *basis, 1, 4, 0.0, 1.0, one, 0, None) == -2
    table = (ctypes.c_double * 200)(*np.linspace(0.0, 1.0, 200))
    assert hip_lib.gts_bias_fit(one, 5, 5, 5, *basis, 1, 4, 4, one, 0.0, 1.0, table, one, one, 1 << 30, 0, None) == -2
    assert hip_lib.gts_bias_fit(one, 5, 5, 5, *basis, 1, 4, 0, one, 0.0, 0.0, table, one, one, 1 << 30, 0, None) == -3
    table[100] = float("nan")
    assert hip_lib.gts_bias_fit(one, 5, 5, 5, *basis, 1, 4, 0, one, 0.0, 1.0, table, one, one, 1 << 30, 0, None) == -3
    assert hip_lib.gts_bias_mean(one, 5, 5, 5, *basis, 1, 4, None, one, 1 << 30, 0, None) == -1
    assert hip_lib.gts_bias_apply(one, 16, 5, 5, 5, *basis, 1, 4, float("nan"), one, None, 0, None) == -3
    assert hip_lib.gts_bias_apply(one, 8, 5, 5, 5, *basis, 1, 4, 0.0, one, None, 0, None) == -3
    assert hip_lib.gts_bias_apply(one, 16, 5, 5, 5, *basis, 1, 4, 0.0, None, None, 0, None) == -1
