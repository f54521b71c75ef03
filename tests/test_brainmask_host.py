"""The host side of the brain extraction (gts/brainmask.py) and its numpy / scipy reference
(tests/brainmask_ref.py), without a GPU: the threshold rule, the flags, the argument checks of the entry points, the
head phantom and what the reference makes of it."""
import ctypes
import hashlib

import numpy as np
import pytest

from tests import brainmask_ref as R

PHANTOM_SHAPES = [(64, 72, 56), (96, 96, 80)]
SEEDS = (0, 1, 2)
# the smallest of the six Dice values in test_reference_reaches_the_bound_on_the_phantom's docstring, minus 0.005
DICE_BOUND = 0.9976310731685514 - 0.005


def _counts(kind):
    rng = np.random.default_rng(11)
    c = np.zeros(R.BINS, dtype=np.int64)
    if kind == "one bin":
        c[777] = 12345
    elif kind == "last bin":
        c[R.BINS - 1] = 999
    elif kind == "one voxel":
        c[0] = 1
    elif kind == "two ends":
        c[0], c[R.BINS - 1] = 98, 2               # ceil(0.98 * 100) = 98 is reached in bin 0 exactly
    elif kind == "two ends, one more":
        c[0], c[R.BINS - 1] = 97, 3
    else:
        c[:] = rng.integers(0, 50, R.BINS)
        c[rng.random(R.BINS) < 0.5] = 0
    return c


@pytest.mark.parametrize("kind", ["one bin", "last bin", "one voxel", "two ends", "two ends, one more", "random"])
def test_threshold_from_counts_equals_the_reference_loop_to_the_last_bit(kind):
    from gts import brainmask

    counts = _counts(kind)
    for hi in (1.0, 937.0, 3.4028234663852886e38, float(np.float32(0.3))):
        for f in (0.0, 0.1, 1.0 / 3.0, 1.0):
            got, want = brainmask.threshold_from_counts(counts, hi, f), R.threshold_from_counts(counts, hi, f)
            assert got[1:] == want[1:], (kind, hi, f)
            assert np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes(), (kind, hi, f)
    t0, b2, b98 = brainmask.threshold_from_counts(counts, 4096.0, 0.0)
    t1 = brainmask.threshold_from_counts(counts, 4096.0, 1.0)[0]
    assert (t0, t1) == (float(b2), float(b98)) and b2 <= b98        # f = 0 and f = 1 are the two percentile bins
    if kind == "one bin":
        assert (b2, b98) == (777, 777)
    if kind == "last bin":
        assert (b2, b98) == (R.BINS - 1, R.BINS - 1)
    if kind == "two ends":
        assert (b2, b98) == (0, 0)
    if kind == "two ends, one more":
        assert (b2, b98) == (0, R.BINS - 1)
    for bad in (np.zeros(R.BINS), np.ones(R.BINS - 1), -np.ones(R.BINS)):
        with pytest.raises(ValueError):
            brainmask.threshold_from_counts(bad, 1.0)


def test_radii_become_squared_radii():
    from gts import brainmask

    assert [brainmask.squared_radius(r) for r in (0, 1, 1.5, 2, 2.9, 3.0, 15.9)] == [0, 1, 2, 4, 8, 9, 252]
    assert [R.squared_radius(r) for r in (0, 1, 1.5, 2, 2.9, 3.0, 15.9)] == [0, 1, 2, 4, 8, 9, 252]
    for bad in (-1, 16, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            brainmask.squared_radius(bad)
    assert R.ball(0).shape == (1, 1, 1) and R.ball(3).sum() == 27 and R.ball(2).sum() == 19 and R.ball(1).sum() == 7
    assert R.ball(9).shape == (7, 7, 7) and R.ball(9).sum() == 123


def test_flags_are_off_by_default_and_checked_before_any_scan_is_read(capsys):
    from gts import brainmask
    from scripts import compute_dataset_stats, preprocess_dataset, segment_scans, skull_strip

    base = ["-d", "/no/such/folder", "-o", "/no/such/out", "-g", "/no/such/weights.pt"]
    off = segment_scans.parse_args(base)
    assert off.skull_strip is None and off.strip is None and off.strip_report is None and off.strip_mask_dir is None
    defaults = dict(radius=3.0, close=2.0, fraction=0.1, connectivity=6)
    assert segment_scans.parse_args(base + ["--skull_strip"]).strip == (1, defaults)           # _t1.nii.gz
    assert segment_scans.parse_args(base + ["--skull_strip", "_t2.nii.gz"]).strip == (3, defaults)
    assert segment_scans.parse_args(base + ["--skull_strip", "-M", "_a.nii", "_b.nii"]).strip == (0, defaults)
    tuned = segment_scans.parse_args(base + ["--skull_strip", "--strip_radius", "2.5", "--strip_close", "0",
                                             "--strip_fraction", "0.25", "--strip_connectivity", "26"])
    assert tuned.strip == (1, dict(radius=2.5, close=0.0, fraction=0.25, connectivity=26))
    for extra in (["--strip_radius", "16"], ["--strip_radius", "-1"], ["--strip_close", "nan"],
                  ["--strip_fraction", "1.5"], ["--strip_fraction", "-0.1"]):
        assert segment_scans.main(base + ["--skull_strip"] + extra) == 2
        assert "segment_scans:" in capsys.readouterr().err
        assert preprocess_dataset.main(["-d", "/no/such/folder", "-o", "/no/such/out", "--skull_strip"] + extra) == 2
        assert skull_strip.main(["-d", "/no/such/folder", "-o", "/no/such/out"] + extra) == 2
        with pytest.raises(SystemExit):
            compute_dataset_stats.main(["-d", "/no/such/folder", "-o", "/no/such/out.json", "-l", "_seg.nii.gz",
                                        "--skull_strip"] + extra)
    assert segment_scans.main(base + ["--skull_strip", "_pd.nii.gz"]) == 2          # none of the modalities
    assert "_pd.nii.gz" in capsys.readouterr().err
    assert skull_strip.main(["-d", "/no/such/folder", "-o", "/no/such/out", "--strip_modality", "_pd.nii.gz"]) == 2
    capsys.readouterr()
    for alone in (["--strip_radius", "2"], ["--strip_mask_dir", "/no/such/dir"], ["--strip_report", "r.json"]):
        assert segment_scans.main(base + alone) == 2                                 # a setting without the switch
        assert f"{alone[0]} need --skull_strip" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                                  # argparse's own: status 2
        segment_scans.parse_args(base + ["--skull_strip", "--strip_connectivity", "18"])
    assert brainmask.reference_index(["_t2.nii.gz", "_t1.nii.gz"]) == 1 and brainmask.reference_index(["_x"]) == 0
    note = brainmask.describe({"mask_ml": 1200.5, "mask_fraction": 0.25, "components": 3, "largest": 100, "second": 50})
    assert "check this scan" in note and "1200.5 ml" in note
    assert "check this scan" not in brainmask.describe({"mask_ml": 1.0, "mask_fraction": 0.5, "components": 2,
                                                        "largest": 100, "second": 49})


def test_entry_points_refuse_bad_arguments_without_a_gpu(hip_lib):
    from gts import ops

    one = ctypes.c_void_p(16)
    big = 1 << 40
    assert (ops.BRAIN_BINS, ops.BRAIN_MAX_R2) == (4096, 255)
    n = 240 * 240 * 155
    assert hip_lib.gts_brainmask_workspace(240, 240, 155) >= 9 * n
    assert hip_lib.gts_brainmask_workspace(0, 5, 5) == 0 and hip_lib.gts_brainmask_workspace(5, -1, 5) == 0
    assert hip_lib.gts_brainmask_workspace(1 << 11, 1 << 10, 1 << 10) == 0              # 2^31 voxels
    assert hip_lib.gts_brainmask_workspace((1 << 31) - 1, 1, 1) > 0
    assert hip_lib.gts_brain_range(None, 4, 5, 5, 5, one, 0, None) == -1
    assert hip_lib.gts_brain_range(one, 2, 5, 5, 5, one, 0, None) == -3
    assert hip_lib.gts_brain_range(one, 4, 5, 0, 5, one, 0, None) == -2
    assert hip_lib.gts_brain_range(one, 4, 5, 5, 5, one, -1, None) == -2
    assert hip_lib.gts_brain_range(one, 16, 1 << 16, 1 << 16, 1, one, 0, None) == -2
    assert hip_lib.gts_brain_histogram(one, 4, 5, 5, 5, 1.0, None, 0, None) == -1
    for hi in (0.0, -1.0, float("nan"), float("inf")):
        assert hip_lib.gts_brain_histogram(one, 4, 5, 5, 5, hi, one, 0, None) == -3
    assert hip_lib.gts_brain_histogram(one, 8, 5, 5, 5, 1.0, one, 0, None) == -3
    assert hip_lib.gts_brain_histogram(one, 4, 5, 5, -5, 1.0, one, 0, None) == -2
    assert hip_lib.gts_brain_threshold(one, 4, 5, 5, 5, 1.0, one, None, 0, None) == -1
    assert hip_lib.gts_brain_threshold(one, 4, 5, 5, 5, float("nan"), one, one, 0, None) == -3
    assert hip_lib.gts_brain_threshold(one, 4, 5, 5, 5, -1.0, one, one, 0, None) == -3
    assert hip_lib.gts_brain_threshold(one, 4, 5, 5, 5, 1.0, one, one, 1 << 31, None) == -2
    # mask_in, X, Y, Z, R2, target, outside, mask_out, workspace, workspace_bytes, invert, grid_blocks, stream
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, 9, 1, 0, None, one, big, 0, 0, None) == -1
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, 9, 1, 0, one, None, big, 0, 0, None) == -1
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, 256, 1, 0, one, one, big, 0, 0, None) == -3
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, -1, 1, 0, one, one, big, 0, 0, None) == -3
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, 9, 2, 0, one, one, big, 0, 0, None) == -3
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, 9, 1, -1, one, one, big, 0, 0, None) == -3
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, 9, 1, 0, one, one, big, 2, 0, None) == -3
    assert hip_lib.gts_ball_morph_i16(one, 5, 0, 5, 9, 1, 0, one, one, big, 0, 0, None) == -2
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, 9, 1, 0, one, one, hip_lib.gts_brainmask_workspace(5, 5, 5) - 1, 0, 0,
                                      None) == -2
    assert hip_lib.gts_ball_morph_i16(one, 5, 5, 5, 9, 1, 0, one, one, big, 0, -3, None) == -2
    # mask, X, Y, Z, connectivity, keep_out, stats, workspace, workspace_bytes, grid_blocks, stream
    assert hip_lib.gts_largest_component_i16(one, 5, 5, 5, 6, one, None, one, big, 0, None) == -1
    assert hip_lib.gts_largest_component_i16(one, 5, 5, 5, 18, one, one, one, big, 0, None) == -2
    assert hip_lib.gts_largest_component_i16(one, 5, 5, 5, 26, one, one, one, 255, 0, None) == -2
    assert hip_lib.gts_largest_component_i16(one, 1 << 31, 1, 1, 26, one, one, one, big, 0, None) == -2
    assert hip_lib.gts_fill_holes_i16(one, 5, 5, 5, None, one, one, big, 0, None) == -1
    assert hip_lib.gts_fill_holes_i16(one, 5, 5, 5, one, one, one, 0, 0, None) == -2
    assert hip_lib.gts_fill_holes_i16(one, 5, 5, 0, one, one, one, big, 0, None) == -2
    # src, dtype, C, X, Y, Z, mask, dst, count, grid_blocks, stream
    assert hip_lib.gts_apply_mask(one, 4, 4, 5, 5, 5, None, one, one, 0, None) == -1
    assert hip_lib.gts_apply_mask(one, 64, 4, 5, 5, 5, one, one, one, 0, None) == -3
    assert hip_lib.gts_apply_mask(one, 4, 0, 5, 5, 5, one, one, one, 0, None) == -2
    assert hip_lib.gts_apply_mask(one, 4, 65, 5, 5, 5, one, one, one, 0, None) == -2
    assert hip_lib.gts_apply_mask(one, 16, 4, 5, 5, 5, one, one, one, -1, None) == -2


def test_wrappers_refuse_bad_operands_on_the_host():
    import torch

    from gts import _lib, ops

    mask = torch.zeros((3, 4, 5), dtype=torch.int16)
    with pytest.raises(_lib.GtsError, match="MI355X only"):
        ops.ball_dilate(mask, 4)
    with pytest.raises(_lib.GtsError, match="int16 mask"):
        ops.ball_dilate(mask.float(), 4)
    with pytest.raises(_lib.GtsError, match="three axes"):
        ops.fill_holes(mask[0])
    with pytest.raises(_lib.GtsError, match="dtype"):
        ops.brain_range(mask.to(torch.int32))


def test_make_sample_is_unchanged_and_the_head_phantom_is_what_it_says():
    from gts import synth_mri

    img, labels = synth_mri.make_sample(0, (24, 20, 16))
    assert hashlib.sha256(img.tobytes() + labels.tobytes()).hexdigest() == \
        "30c27d6aaacd11b54500f7dd6fafe490b45d0d7e4471aa95edc3a33e5ab22cbe"
    shape = PHANTOM_SHAPES[0]
    head, head_labels, truth = synth_mri.make_head_sample(0, shape)
    again = synth_mri.make_head_sample(0, shape)
    assert all(np.array_equal(a, b) for a, b in zip((head, head_labels, truth), again))
    assert head.shape == shape + (4,) and head.dtype == np.float32 and truth.dtype == np.bool_ and truth.shape == shape
    assert head_labels.dtype == np.int16 and set(np.unique(head_labels).tolist()) <= {0, 1, 2, 4}
    assert not (head_labels != 0)[~truth].any()                     # the tumour lies inside the brain
    assert np.array_equal(head, np.rint(head)) and head.min() >= 0 and head.max() < 32767      # fits int16 as written
    t1 = head[..., 1]
    assert ((t1 > 0) & ~truth).sum() > truth.sum()                  # skull, scalp and positive air noise
    assert t1[truth].mean() > 5 * np.median(t1[~truth])
    assert not truth[0].any() and not truth[:, 0].any() and not truth[:, :, 0].any()


@pytest.mark.parametrize("shape", PHANTOM_SHAPES)
def test_without_the_erosion_the_scalp_stays_attached(shape):
    """Radius 0: the tissue bridges through the skull keep the scalp in the brain's component.  Dice of the
    reference's mask against the true intracranial mask: 0.5846, 0.5844, 0.5852 at (64, 72, 56) and 0.5850, 0.5849,
    0.5846 at (96, 96, 80), seeds 0-2."""
    for seed in SEEDS:
        t1, truth, _, _ = R.phantom_case(shape, seed)
        mask, _ = R.brain_mask(t1, radius=0.0)
        value = R.dice(mask, truth)
        print(f"radius 0, {shape} seed {seed}: Dice {value:.4f}")
        assert value <= 0.7


@pytest.mark.parametrize("shape", PHANTOM_SHAPES)
def test_reference_reaches_the_bound_on_the_phantom(shape):
    """The defaults (radius 3, close 2, fraction 0.1, connectivity 6).  Dice of the reference's mask against the true
    intracranial mask (brain + CSF shell), measured with this reference:
        (64, 72, 56): seed 0 0.9976310731685514, seed 1 0.9979145748049741, seed 2 0.9981390080103568
        (96, 96, 80): seed 0 0.9993309699397873, seed 1 0.9993283368689858, seed 2 0.9995532223835586
    DICE_BOUND is the smallest of the six minus 0.005 = 0.9926310731685514."""
    for seed in SEEDS:
        _, truth, mask, report = R.phantom_case(shape, seed)
        value = R.dice(mask, truth)
        print(f"defaults, {shape} seed {seed}: Dice {value!r}, {report}")
        assert value >= DICE_BOUND
        assert report["largest"] > 2 * report["second"]             # no "check this scan" on the phantom
