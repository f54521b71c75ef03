"""gts.metrics.hd95s_mm / surface_dices (H3w-H5w) on the GPU against the scipy reference of tests/surface_ref.py,
and against the unit-spacing kernels where the spacing is isotropic.  Every comparison is == on float64 or on
integers: the device arithmetic is exact integers and the host finish performs the reference's float operations.

Shapes: (129, 3, 70) has Z > 64 (several lane chunks in Y and X passes) and X = 129 > 102, the longest line at
which the X pass still has 64 lanes per workgroup (int64 values and uint16 stack: 10 X bytes per lane of 64 KiB);
(700, 3, 66) leaves it 9 lanes; (3, 300, 70) has Y = 300 > 256, the longest line with 64 lanes in the Y pass
(4 Y bytes per lane), which leaves 54."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import lesionwise_ref, surface_ref

pytestmark = pytest.mark.gpu

# spacing in mm -> the integer units the device works in
SPACINGS = {(1, 1, 5): (1.0, 1.0, 5.0), (15, 15, 80): (0.9375, 0.9375, 5.0), (47, 47, 150): (0.47, 0.47, 1.5),
            (10000, 9400, 33333): (1.0, 0.94, 3.3333)}
TOLERANCES = (0.5, 1.0, 2.0, 5.0)


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int16, order="C")).cuda()        # a copy: the shared pairs are read-only


@functools.lru_cache(maxsize=None)
def _pair(shape):
    """One blobs pair per shape, shared by the tests (read-only)."""
    rng = np.random.default_rng(sum(shape))
    pred, truth = surface_ref.blobs(shape, rng), surface_ref.blobs(shape, rng)
    pred.setflags(write=False)
    truth.setflags(write=False)
    return pred, truth


def _check(pred, truth, spacing, tolerances=TOLERANCES):
    """Device HD95 (mm) and surface Dice == the scipy reference, for the three regions; returns both."""
    from gts.metrics import hd95s_mm, surface_dices

    want_hd, want_nsd = surface_ref.scores(pred, truth, spacing, tolerances)
    p, t = _dev(pred), _dev(truth)
    got_hd, got_nsd = hd95s_mm(p, t, spacing), surface_dices(p, t, spacing, tolerances)
    assert all(isinstance(v, float) for v in got_hd)
    print(pred.shape, spacing, "hd95", got_hd, want_hd, "nsd", got_nsd, want_nsd)
    assert got_hd == want_hd, (pred.shape, spacing, got_hd, want_hd)
    assert got_nsd == want_nsd, (pred.shape, spacing, got_nsd, want_nsd)
    return got_hd, got_nsd


# 1. isotropic spacings against the unit-spacing kernels
def _check_unit_spacing(pred, truth):
    from gts.metrics import hd95_order_stats, hd95s, hd95s_mm, surface_stats

    p, t = _dev(pred), _dev(truth)
    voxels = hd95s(p, t)
    assert hd95s_mm(p, t, (1, 1, 1)) == voxels
    assert torch.equal(surface_stats(p, t, (1, 1, 1))[:, :4].cpu(), hd95_order_stats(p, t).cpu())
    assert torch.equal(surface_stats(p, t, (0.5, 0.5, 0.5))[:, :4].cpu(), hd95_order_stats(p, t).cpu())
    present = [v not in (0.0, 300.0) for v in voxels]
    half = hd95s_mm(p, t, (0.5, 0.5, 0.5))
    assert [h for h, on in zip(half, present) if on] == [0.5 * v for v, on in zip(voxels, present) if on]
    return voxels


@pytest.mark.parametrize("shape", [(37, 50, 61), (129, 3, 70), (16, 16, 16)])
def test_unit_spacing_equals_the_voxel_path(shape):
    _check_unit_spacing(*_pair(shape))


def test_unit_spacing_on_the_reference_fixtures(golden_dir):
    d = np.load(os.path.join(golden_dir, "ref_evaluation.npz"))
    for i in range(3):
        voxels = _check_unit_spacing(d[f"pred{i}"], d[f"true{i}"])
        assert voxels == [float(v) for v in d[f"brats{i}"][3:]]


# 2. anisotropic spacings against scipy
@pytest.mark.parametrize("units", sorted(SPACINGS))
@pytest.mark.parametrize("shape", [(37, 50, 61), (5, 90, 33), (129, 3, 70), (700, 3, 66), (3, 300, 70), (37, 1, 50),
                                   (1, 1, 90)])
def test_against_scipy(shape, units):
    from gts.metrics import spacing_units

    spacing = SPACINGS[units]
    assert spacing_units(spacing)[0] == units
    _check(*_pair(shape), spacing)


@pytest.mark.parametrize("units", sorted(SPACINGS))
def test_lone_voxel(units):
    spacing = SPACINGS[units]
    three, two = np.full((1, 1, 1), 3, np.int16), np.full((1, 1, 1), 2, np.int16)
    assert _check(three, three, spacing) == ([0.0] * 3, [[1.0] * 3] * 4)
    assert _check(two, three, spacing) == ([0.0, 0.0, 300.0], [[1.0, 1.0, 0.0]] * 4)


def test_tie_at_the_tolerance():
    """Two single voxels one 5 mm slice apart: D2 = 25 = T at 5.0 mm, within; T = 4 at 2.0 mm, outside."""
    from gts.metrics import surface_dices

    one, other = np.zeros((6, 7, 9), np.int16), np.zeros((6, 7, 9), np.int16)
    one[2, 3, 4], other[2, 3, 5] = 3, 3
    got_hd, got_nsd = _check(one, other, (1, 1, 5), (5.0, 2.0))
    assert got_hd == [5.0] * 3 and got_nsd == [[1.0] * 3, [0.0] * 3]
    other = np.zeros_like(one)
    other[3, 3, 4] = 3                                    # one in-plane voxel: 1 mm
    assert surface_dices(_dev(one), _dev(other), (1, 1, 5), (1.0, 0.9999)) == [[1.0] * 3, [0.0] * 3]
    _check(one, other, (0.9375, 0.9375, 5), (0.9375, 0.9374))


# 3. absent regions and extremes
def test_absent_regions_and_extremes():
    shape = (20, 24, 28)
    spacing = SPACINGS[(15, 15, 80)]
    rng = np.random.default_rng(3)
    a = surface_ref.blobs(shape, rng, labels=(1, 2))      # no ET: absent from one side below, from both here
    b = surface_ref.blobs(shape, rng, labels=(1, 2))
    hd, nsd = _check(a, b, spacing)
    assert hd[2] == 0.0 and [row[2] for row in nsd] == [1.0] * 4
    c = surface_ref.blobs(shape, rng)
    c[c == 0] = 1                                         # ... ET present in truth only
    hd, nsd = _check(a, c, spacing)
    assert c[c == 3].size and hd[2] == 300.0 and [row[2] for row in nsd] == [0.0] * 4
    empty = np.zeros(shape, np.int16)
    assert _check(empty, empty, spacing) == ([0.0] * 3, [[1.0] * 3] * 4)
    assert _check(empty, c, spacing) == ([300.0] * 3, [[0.0] * 3] * 4)
    one, other = np.zeros(shape, np.int16), np.zeros(shape, np.int16)
    one[3, 5, 7], other[19, 0, 27] = 3, 3                 # single voxels
    _check(one, other, spacing)
    assert _check(one, one, spacing) == ([0.0] * 3, [[1.0] * 3] * 4)
    full = np.full(shape, 3, np.int16)                    # a region filling the volume
    _check(full, c, spacing)
    _check(full, full, SPACINGS[(10000, 9400, 33333)])


# 4. the only full-size test: two calls give one table
def test_brats_size_pair_is_repeatable():
    from gts.metrics import surface_stats

    shape = (240, 240, 155)
    rng = np.random.default_rng(11)
    pred, truth = np.zeros(shape, np.int16), np.zeros(shape, np.int16)
    sub = (slice(70, 170), slice(60, 180), slice(30, 125))
    sub_shape = tuple(s.stop - s.start for s in sub)
    pred[sub], truth[sub] = surface_ref.blobs(sub_shape, rng, n_blobs=5), surface_ref.blobs(sub_shape, rng, n_blobs=5)
    pred[200:204, 20:23, 140:150] = 1                     # a stray false positive far from the tumour
    p, t = _dev(pred), _dev(truth)
    first = surface_stats(p, t, SPACINGS[(15, 15, 80)], TOLERANCES).cpu()
    assert torch.equal(first, surface_stats(p, t, SPACINGS[(15, 15, 80)], TOLERANCES).cpu())
    assert (first[:, 3] == 3).all() and (first[:, 1] > 0).all() and (first[:, 2] >= first[:, 1]).all()
    within = first[:, 4:].reshape(3, 2, 4)
    assert (within[:, :, 1:] >= within[:, :, :-1]).all() and (within.sum(dim=1)[:, 3] <= first[:, 0]).all()


# 5. lesion-wise scores in millimetres
def _lesion_volume():
    """48 x 40 x 24: two truth lesions (one of them missed by the prediction) and one false-positive island."""
    shape = (48, 40, 24)
    truth, pred = np.zeros(shape, np.int16), np.zeros(shape, np.int16)
    truth[6:16, 8:18, 5:12] = 1
    truth[8:13, 10:15, 7:10] = 3
    truth[30:38, 20:30, 10:18] = 2                        # missed
    pred[7:17, 7:16, 6:13] = 1
    pred[9:13, 10:14, 8:11] = 3
    pred[40:44, 4:8, 2:6] = 3                             # matched to no lesion
    return pred, truth


def _same_float(a, b):
    return (a is None and b is None) or (a is not None and b is not None
                                         and np.float64(a).tobytes() == np.float64(b).tobytes())


def test_lesionwise_scores_in_millimetres():
    from gts import lesionwise

    pred, truth = _lesion_volume()
    spacing, tolerances = (1.0, 1.0, 5.0), (1.0,)
    got = lesionwise.lesionwise_scores(_dev(pred), _dev(truth), 3, 50, spacing_mm=spacing, nsd_tolerances_mm=tolerances)
    want = surface_ref.lesionwise_scores(pred, truth, spacing, tolerances, 3, 50)
    assert (want["WT"]["n_scored"], want["WT"]["n_fn"], want["WT"]["n_fp"]) == (2, 1, 1)
    for region in surface_ref.REGIONS:
        g, w = got[region], want[region]
        shown = ("hd95", "lw_hd95", "nsd", "lw_nsd")
        print(region, {k: g[k] for k in shown}, {k: w[k] for k in shown})
        assert set(g) == set(w)
        for f in ("n_lesions", "n_scored", "n_fp", "n_fn", "lesion_roots"):
            assert g[f] == w[f], (region, f)
        for f in ("dice", "hd95", "lw_dice", "lw_hd95"):
            assert _same_float(g[f], w[f]), (region, f, g[f], w[f])
        assert g["nsd"] == w["nsd"] and g["lw_nsd"] == w["lw_nsd"], (region, g["nsd"], w["nsd"], g["lw_nsd"], w["lw_nsd"])
        assert len(g["lesions"]) == len(w["lesions"])
        for gl, wl in zip(g["lesions"], w["lesions"]):
            assert set(gl) == set(wl) and gl["nsd"] == wl["nsd"], (region, gl, wl)
            assert _same_float(gl["hd95"], wl["hd95"]) and _same_float(gl["dice"], wl["dice"]), (region, gl, wl)
    missed = got["WT"]["lesions"][1]
    assert missed["hd95"] == 374.0 and missed["nsd"] == [0.0]
    # a spacing without tolerances adds no key
    plain_mm = lesionwise.lesionwise_scores(_dev(pred), _dev(truth), spacing_mm=spacing)
    assert "nsd" not in plain_mm["WT"] and "nsd" not in plain_mm["WT"]["lesions"][0]
    assert plain_mm["WT"]["hd95"] == got["WT"]["hd95"] and plain_mm["WT"]["lw_hd95"] == got["WT"]["lw_hd95"]


def test_lesionwise_scores_without_a_spacing_are_unchanged():
    from gts import lesionwise

    pred, truth = _lesion_volume()
    got = lesionwise.lesionwise_scores(_dev(pred), _dev(truth), 3, 50, spacing_mm=None, nsd_tolerances_mm=())
    assert got == lesionwise.lesionwise_scores(_dev(pred), _dev(truth), 3, 50)
    want = lesionwise_ref.lesionwise_scores(pred, truth, 3, 50)
    keys = {"dice", "hd95", "lw_dice", "lw_hd95", "n_lesions", "n_scored", "n_fp", "n_fn", "lesions", "lesion_roots"}
    for region in lesionwise_ref.REGIONS:
        assert set(got[region]) == keys == set(want[region])
        assert got[region] == want[region], region
        assert all(set(s) == {"vol", "tp", "matched_voxels", "scored", "dice", "hd95"} for s in got[region]["lesions"])
    with pytest.raises(lesionwise._lib.GtsError, match="spacing_mm"):
        lesionwise.lesionwise_scores(_dev(pred), _dev(truth), nsd_tolerances_mm=(1.0,))


# 6. the command line
def test_cli_in_millimetres(tmp_path, capsys):
    from data_processing import labels, nifti_io
    from gts import lesionwise
    from scripts import score_predictions as cli

    affine = np.diag([0.9375, 0.9375, 5.0, 1.0])
    spacing = (0.9375, 0.9375, 5.0)
    data, preds = tmp_path / "data", tmp_path / "preds"
    preds.mkdir()
    pairs = {"scan_a": lesionwise_ref.blobs_and_salt((24, 22, 21), 40), "scan_b": _lesion_volume()}
    for scan, (pred, truth) in pairs.items():
        (data / scan).mkdir(parents=True)
        nifti_io.save_as_nifti(labels.swap_labels_to_brats(truth), str(data / scan / f"{scan}_seg.nii.gz"), affine)
        nifti_io.save_as_nifti(labels.swap_labels_to_brats(pred), str(preds / f"{scan}.nii.gz"), affine)
    common = ["-d", str(data), "-l", "_seg.nii.gz", "-s", str(preds), "-p", "scan", "--min_lesion_voxels", "20"]

    out = tmp_path / "mm.csv"
    assert cli.main(common + ["-o", str(out), "--nsd_tolerance", "1", "2"]) == 0      # implies --mm
    lines = out.read_text().splitlines()
    assert lines[0].split(",") == cli.header_for([1.0, 2.0]) and len(lines[0].split(",")) == len(cli.HEADER) + 12
    assert [line.split(",")[0] for line in lines[1:]] == ["scan_a", "scan_b", "mean"]
    want = {scan: cli.row_of(surface_ref.lesionwise_scores(pred, truth, spacing, (1.0, 2.0), 3, 20), 2)
            for scan, (pred, truth) in pairs.items()}
    for line in lines[1:3]:
        cells = line.split(",")
        assert [float(c) for c in cells[1:]] == [float(v) for v in want[cells[0]]], cells[0]
    assert [float(c) for c in lines[3].split(",")[1:]] == cli.mean_row([want[s] for s in sorted(want)])
    only_mm = tmp_path / "only_mm.csv"
    assert cli.main(common + ["-o", str(only_mm), "--mm"]) == 0
    assert [line.split(",") for line in only_mm.read_text().splitlines()] == \
        [line.split(",")[:len(cli.HEADER)] for line in lines]

    # without flags: the bytes of the unchanged code path (voxel units, HEADER's columns)
    plain = tmp_path / "plain.csv"
    assert cli.main(common + ["-o", str(plain)]) == 0
    rows = {scan: cli.row_of(lesionwise.lesionwise_scores(_dev(pred), _dev(truth), 3, 20))
            for scan, (pred, truth) in pairs.items()}
    expected = [",".join(cli.HEADER)] + [cli.format_row(s, rows[s]) for s in sorted(rows)] + \
        [cli.format_row("mean", cli.mean_row([rows[s] for s in sorted(rows)]))]
    assert plain.read_bytes() == ("\n".join(expected) + "\n").encode()
    assert rows["scan_b"] == cli.row_of(lesionwise_ref.lesionwise_scores(*pairs["scan_b"], 3, 20))

    # a prediction whose header says 1 mm is left out
    capsys.readouterr()
    nifti_io.save_as_nifti(labels.swap_labels_to_brats(pairs["scan_a"][0]), str(preds / "scan_a.nii.gz"))
    refused = tmp_path / "refused.csv"
    assert cli.main(common + ["-o", str(refused), "--mm"]) == 1
    printed = capsys.readouterr().out
    assert "scan_a: left out" in printed and "spacing" in printed and "1 scan(s) scored, 1 left out" in printed
    assert [line.split(",")[0] for line in refused.read_text().splitlines()] == ["id", "scan_b", "mean"]
    assert cli.main(common + ["-o", str(tmp_path / "voxels.csv")]) == 0               # without --mm the header is not read
