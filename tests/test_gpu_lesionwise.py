"""gts.lesionwise on the MI355X against the scipy reference of the definition (tests/lesionwise_ref.py): the
dilation, every integer table, and every float (per-lesion Dice and HD95, both aggregates) compared for equality.
The device route and the reference perform the same float operations: one division per lesion, np.percentile's
interpolation, and sequential float64 sums in lesion order."""
import numpy as np
import pytest
import torch

from tests import lesionwise_ref as ref

pytestmark = pytest.mark.gpu
INT_FIELDS = ("n_lesions", "n_scored", "n_fp", "n_fn")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int16)).cuda()


def _labels(mask, value=3):
    """A boolean mask as an internal-label volume: `value` is in all three regions when it is 3."""
    return np.where(mask, value, 0).astype(np.int16)


def _same_float(a, b):
    return (a is None and b is None) or (a is not None and b is not None
                                         and np.float64(a).tobytes() == np.float64(b).tobytes())


def _assert_record(got, want, where):
    for f in INT_FIELDS:
        assert got[f] == want[f], (where, f, got[f], want[f])
    assert got["lesion_roots"] == want["lesion_roots"], where
    assert len(got["lesions"]) == len(want["lesions"])
    for k, (g, w) in enumerate(zip(got["lesions"], want["lesions"])):
        assert (g["vol"], g["tp"], g["matched_voxels"], g["scored"]) == \
            (w["vol"], w["tp"], w["matched_voxels"], w["scored"]), (where, k, g, w)
        assert _same_float(g["dice"], w["dice"]) and _same_float(g["hd95"], w["hd95"]), (where, k, g, w)
    for f in ("lw_dice", "lw_hd95", "dice", "hd95"):
        assert _same_float(got[f], want[f]), (where, f, got[f], want[f])


def _check_scores(pred, truth, dilation=3, min_lesion_voxels=50):
    """Device scores == reference scores for all three regions; returns the device's."""
    from gts import lesionwise

    got = lesionwise.lesionwise_scores(_dev(pred), _dev(truth), dilation, min_lesion_voxels)
    want = ref.lesionwise_scores(pred, truth, dilation, min_lesion_voxels)
    assert set(got) == set(ref.REGIONS)
    for region in ref.REGIONS:
        _assert_record(got[region], want[region], region)
    return got


def _check_tables(pred, truth, region="WT", dilation=3):
    from gts import lesionwise

    got = lesionwise.lesion_tables(_dev(pred), _dev(truth), region, dilation)
    want = ref.region_tables(ref.region_mask(pred, region), ref.region_mask(truth, region), dilation)
    for f in ("lesion_roots", "vol", "tp", "matched_voxels", "n_fp", "comp_sizes"):
        assert got[f] == want[f], (region, f)
    return got


def _box(shape, lo, hi):
    vol = np.zeros(shape, dtype=bool)
    vol[tuple(slice(a, b) for a, b in zip(lo, hi))] = True
    return vol


# 1. dilation, bit-equal to scipy
def _dilation_cases(shape, rng):
    x, y, z = shape
    for cx in {0, x - 1}:
        for cy in {0, y - 1}:
            for cz in {0, z - 1}:
                one = np.zeros(shape, dtype=np.int16)
                one[cx, cy, cz] = 3
                yield one
    one = np.zeros(shape, dtype=np.int16)
    one[x // 2, y // 2, z // 2] = 3
    yield one
    for p in (0.002, 0.05, 0.5):
        yield ((rng.random(shape) < p) * rng.integers(1, 4, shape)).astype(np.int16)
    yield np.full(shape, 2, dtype=np.int16)
    yield np.zeros(shape, dtype=np.int16)


@pytest.mark.parametrize("z", [1, 31, 32, 33, 63, 64, 65, 130])
def test_dilation_equals_scipy(hip_lib, z):
    from gts import lesionwise

    rng = np.random.default_rng(z)
    for x in (1, 5, 9):
        for y in (1, 5, 9):
            for c, labels in enumerate(_dilation_cases((x, y, z), rng)):
                dev = _dev(labels)
                region = ref.REGIONS[c % 3]
                mask = ref.region_mask(labels, region)
                for n in (0, 1, 2, 3):
                    got = lesionwise.dilate_region(dev, region, n)
                    assert got.dtype == torch.int16 and got.shape == dev.shape
                    assert np.array_equal(got.cpu().numpy(), ref.dilate(mask, n).astype(np.int16)), ((x, y, z), c, n)


def test_dilation_over_several_tiles_and_words(hip_lib):
    """More than one tile along every axis (8 rows, 8 rows, 4 words) and carries across words and tiles."""
    from gts import lesionwise

    rng = np.random.default_rng(11)
    labels = ((rng.random((19, 21, 600)) < 0.004) * rng.integers(1, 4, (19, 21, 600))).astype(np.int16)
    labels[:, :, 255:257] = np.where(rng.random((19, 21, 2)) < 0.05, 3, 0)
    for region in ref.REGIONS:
        for n in (1, 3):
            got = lesionwise.dilate_region(_dev(labels), region, n).cpu().numpy()
            assert np.array_equal(got, ref.dilate(ref.region_mask(labels, region), n).astype(np.int16)), (region, n)


# 2. where two ground-truth components become one lesion
@pytest.mark.parametrize("direction", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 1, 1)])
def test_merge_edge(hip_lib, direction):
    shape = (30, 30, 30)
    axial = sum(direction) == 1
    for gap in range(4, 10):
        a = (4, 4, 4)
        b = tuple(4 + d * (2 + gap) for d in direction)
        truth = _labels(_box(shape, a, [c + 2 for c in a]) | _box(shape, b, [c + 2 for c in b]))
        pred = _labels(_box(shape, a, [c + 1 for c in a]))
        got = _check_tables(pred, truth)                      # lesion order and vol_k equal the reference's
        if axial:                                             # 6 empty voxels are bridged by 3 + 3, 7 are not
            assert len(got["vol"]) == (1 if gap <= 6 else 2), (direction, gap)
        assert sum(got["vol"]) == 16


# 3. where a predicted component is matched
def test_match_edge(hip_lib):
    shape = (24, 16, 16)
    truth = _labels(_box(shape, (4, 4, 4), (8, 8, 8)))                      # 64 voxels: scored
    near, far = np.zeros(shape, dtype=np.int16), np.zeros(shape, dtype=np.int16)
    near[10, 5, 5] = 3                                                       # 3 voxels off the face x = 7
    far[11, 5, 5] = 3
    got = _check_scores(near, truth)["WT"]
    lesion = got["lesions"][0]
    assert (lesion["tp"], lesion["dice"], lesion["matched_voxels"]) == (0, 0.0, 1) and np.isfinite(lesion["hd95"])
    assert lesion["hd95"] < 374 and (got["n_fp"], got["n_fn"]) == (0, 0)
    got = _check_scores(far, truth)["WT"]
    assert (got["n_fp"], got["n_fn"], got["lw_dice"], got["lw_hd95"]) == (1, 1, 0.0, 374.0)


def test_bar_across_two_lesions_and_unscored_match(hip_lib):
    shape = (40, 16, 16)
    truth = _labels(_box(shape, (4, 4, 4), (8, 8, 8)) | _box(shape, (24, 4, 4), (28, 8, 8)))
    bar = _labels(_box(shape, (5, 5, 5), (27, 6, 6)))
    got = _check_scores(bar, truth)["WT"]
    assert [(s["matched_voxels"], s["tp"]) for s in got["lesions"]] == [(22, 3), (22, 3)] and got["n_fp"] == 0
    # a component matched only to a lesion too small to be scored is no false positive
    speck = _labels(_box(shape, (4, 4, 4), (6, 6, 6)))
    touch = np.zeros(shape, dtype=np.int16)
    touch[8, 5, 5] = 3
    got = _check_scores(touch, speck)["WT"]
    assert (got["n_lesions"], got["n_scored"], got["n_fp"], got["lw_dice"], got["lw_hd95"]) == (1, 0, 0, 1.0, 0.0)


# 4. the threshold: more than min_lesion_voxels
def test_scoring_threshold(hip_lib):
    shape = (20, 40, 12)
    fifty, more = _box(shape, (3, 3, 3), (8, 8, 5)), _box(shape, (3, 23, 3), (8, 28, 5))
    more[8, 23, 3] = True
    truth = _labels(fifty | more)
    got = _check_scores(truth, truth)["WT"]
    assert [(s["vol"], s["scored"]) for s in got["lesions"]] == [(50, False), (51, True)]
    assert (got["n_scored"], got["lw_dice"], got["lw_hd95"]) == (1, 1.0, 0.0)
    got = _check_scores(truth, truth, min_lesion_voxels=49)["WT"]
    assert got["n_scored"] == 2


# 5. the crop: lesions on a face, an edge and a corner of the volume, and one inside
def test_crop_exactness(hip_lib):
    shape = (33, 30, 70)
    spots = [((0, 0, 0), (5, 4, 6)), ((0, 12, 64), (4, 18, 70)), ((28, 0, 30), (33, 5, 36)), ((14, 25, 20), (20, 30, 26)),
             ((14, 12, 40), (19, 17, 46))]
    truth, pred = np.zeros(shape, dtype=np.int16), np.zeros(shape, dtype=np.int16)
    rng = np.random.default_rng(3)
    for lo, hi in spots:
        truth[_box(shape, lo, hi)] = 3
        shift = rng.integers(-2, 3, 3)
        lo2 = [max(a + s, 0) for a, s in zip(lo, shift)]
        hi2 = [min(b + s, e) for b, s, e in zip(hi, shift, shape)]
        pred[_box(shape, lo2, hi2)] = 3
    pred[16, 14, 44:60] = 3                                   # a tail that lengthens one lesion's box
    got = _check_scores(pred, truth)                          # hd95_k == evaluation.hd95 on the full-volume masks
    assert got["ET"]["n_scored"] == 5 and all(0 <= s["hd95"] < 374 for s in got["ET"]["lesions"])


def test_unit_axes(hip_lib):
    """A volume with a unit axis: scipy's erosion then makes every mask voxel a border voxel."""
    for shape in ((1, 30, 40), (20, 1, 70)):
        pred, truth = np.zeros(shape, dtype=np.int16), np.zeros(shape, dtype=np.int16)
        flat = [s for s in shape if s != 1]
        truth.reshape(flat)[3:12, 5:14] = 3
        pred.reshape(flat)[4:14, 5:12] = 3
        pred.reshape(flat)[17, 30] = 1
        assert _check_scores(pred, truth)["WT"]["n_fp"] == 1


# 6. random pairs
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(40, 36, 33), (64, 64, 65)])
def test_random_pairs(hip_lib, shape, seed):
    pred, truth = ref.blobs_and_salt(shape, 100 * shape[0] + seed)
    _check_scores(pred, truth)
    for region in ref.REGIONS:
        _check_tables(pred, truth, region)


@pytest.mark.parametrize("dilation", [0, 1, 2])
def test_other_dilations(hip_lib, dilation):
    pred, truth = ref.blobs_and_salt((40, 36, 33), 7)
    _check_scores(pred, truth, dilation, min_lesion_voxels=10)


# 7. the worst case for the pair list: every second voxel predicted
def test_checkerboard_prediction(hip_lib):
    shape = (24, 24, 24)
    x, y, z = np.indices(shape)
    for board in ((x + y + z) % 2 == 0, (x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0)):      # one component; 1728 of them
        pred = _labels(board, 1)
        truth = _labels(_box(shape, (6, 7, 8), (14, 13, 15)), 2)
        for region in ("WT", "CT"):
            _check_tables(pred, truth, region)
        _check_scores(pred, truth)


# 8. full size
def test_full_size_twice(hip_lib):
    from gts import lesionwise

    pred, truth = ref.blobs_and_salt((240, 240, 155), 9, salt=0.001)
    dev_pred, dev_truth = _dev(pred), _dev(truth)
    first = lesionwise.lesionwise_scores(dev_pred, dev_truth)
    second = lesionwise.lesionwise_scores(dev_pred, dev_truth)
    assert first == second
    assert first["WT"]["n_scored"] >= 2 and first["WT"]["n_fp"] > 1000
    assert 0.0 < first["WT"]["lw_dice"] < first["WT"]["dice"]


def test_mid_size_against_reference(hip_lib):
    pred, truth = ref.blobs_and_salt((96, 96, 64), 4, salt=0.001)
    _check_scores(pred, truth)


# 9. the wrappers' refusals
def test_wrappers_refuse(hip_lib):
    from gts import GtsError, lesionwise

    good = torch.zeros((4, 5, 6), dtype=torch.int16, device="cuda")
    calls = (lambda p, t, **kw: lesionwise.lesionwise_scores(p, t, **kw),
             lambda p, t, **kw: lesionwise.lesion_tables(p, t, "WT", **kw),
             lambda p, t, **kw: lesionwise.dilate_region(p, "CT", **kw))
    for call in calls:
        with pytest.raises(GtsError, match="MI355X only"):
            call(good.cpu(), good.cpu())
        with pytest.raises(GtsError, match="int16"):
            call(good.int(), good.int())
        with pytest.raises(GtsError, match="dilation"):
            call(good, good, dilation=4)
        with pytest.raises(GtsError, match="empty"):
            call(good[:0], good[:0])
    for call in calls[:2]:
        with pytest.raises(GtsError, match="differ"):
            call(good, good[:3])
    with pytest.raises(GtsError, match="region"):
        lesionwise.dilate_region(good, "TC")
    with pytest.raises(GtsError, match=r"\[X, Y, Z\]"):
        lesionwise.dilate_region(good[0], "WT")


def test_abi_refusals(hip_lib):
    one = 16
    assert hip_lib.gts_lesionwise_workspace(0, 4, 4) == 0 and hip_lib.gts_lesionwise_workspace(1 << 11, 1 << 10, 1 << 10) == 0
    assert hip_lib.gts_lesionwise_dilate_i16(None, 4, 4, 4, 0, 3, one, one, 1 << 20, None) == -1
    assert hip_lib.gts_lesionwise_dilate_i16(one, 4, 4, 4, 0, 4, one, one, 1 << 20, None) == -3
    assert hip_lib.gts_lesionwise_dilate_i16(one, 4, 4, 4, 3, 3, one, one, 1 << 20, None) == -3
    assert hip_lib.gts_lesionwise_dilate_i16(one, 4, 4, 4, 0, 3, one, one, 8, None) == -2
    assert hip_lib.gts_lesionwise_dilate_i16(one, 1 << 11, 1 << 10, 1 << 10, 0, 3, one, one, 1 << 40, None) == -2
    assert hip_lib.gts_lesionwise_tables_i16(one, one, one, 4, 4, 4, 0, one, 4, one, 1 << 20, None) == -2


# 10. the command line
def test_cli_scores_written_predictions(hip_lib, tmp_path, capsys):
    import os

    from data_processing import labels, nifti_io
    from scripts import score_predictions as cli

    shape = (24, 22, 21)
    data, preds = tmp_path / "data", tmp_path / "preds"
    preds.mkdir()
    want = {}
    for i, scan in enumerate(["scan_a", "scan_b", "scan_c", "scan_d", "scan_e"]):
        pred, truth = ref.blobs_and_salt(shape, 40 + i)
        folder = data / scan
        folder.mkdir(parents=True)
        brats_truth, brats_pred = labels.swap_labels_to_brats(truth), labels.swap_labels_to_brats(pred)
        if scan == "scan_b":                                   # the 2023 convention: enhancing tumour is 3
            brats_truth = np.where(brats_truth == 4, 3, brats_truth).astype(np.int16)
        nifti_io.save_as_nifti(brats_truth, str(folder / f"{scan}_seg.nii.gz"))
        if scan == "scan_d":                                   # no prediction
            continue
        if scan == "scan_e":                                   # another shape
            brats_pred = brats_pred[:, :, :-1]
        nifti_io.save_as_nifti(brats_pred, str(preds / f"{scan}.nii.gz"))
        if scan != "scan_e":
            want[scan] = cli.row_of(ref.lesionwise_scores(pred, truth, 3, 20))
    out = tmp_path / "scores.csv"
    status = cli.main(["-d", str(data), "-l", "_seg.nii.gz", "-s", str(preds), "-p", "scan", "-o", str(out),
                       "--min_lesion_voxels", "20"])
    assert status == 1
    printed = capsys.readouterr().out
    assert "scan_d: left out" in printed and "scan_e: left out" in printed and "3 scan(s) scored, 2 left out" in printed
    lines = out.read_text().splitlines()
    assert lines[0].split(",") == cli.HEADER and [line.split(",")[0] for line in lines[1:]] == sorted(want) + ["mean"]
    for line in lines[1:4]:
        cells = line.split(",")
        assert [float(c) for c in cells[1:]] == [float(v) for v in want[cells[0]]], cells[0]
    assert [float(c) for c in lines[4].split(",")[1:]] == cli.mean_row([want[s] for s in sorted(want)])
    assert os.listdir(tmp_path / "preds")                      # inputs untouched
