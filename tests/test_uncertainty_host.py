"""Uncertainty maps and their QU score, the parts that need no GPU: qu_from_histogram on hand-computed cases and
against the mask-based restatement, the file names, the command-line flags and the argument checks of the C entry
points that come before any launch."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import uncertainty_ref as R

TP, FP, FN, TN = range(4)


def _hist():
    return np.zeros((3, 4, 102), dtype=np.int64)


# ------------------------------------------------------------------------------------------------ qu_from_histogram
def test_perfect_prediction_with_certain_maps_scores_one():
    from gts.uncertainty import qu_from_histogram

    hist = _hist()
    hist[:, TP, 0] = (50, 30, 10)
    hist[:, TN, 0] = (950, 970, 990)
    for region, s in qu_from_histogram(hist).items():
        assert s["qu"] == 1.0 and s["dice_auc"] == 1.0 and s["ftp_auc"] == 0.0 and s["ftn_auc"] == 0.0, region
        assert s["dice"] == [1.0] * 4 and s["ftp"] == [0.0] * 4 and s["ftn"] == [0.0] * 4


def test_everything_filtered_below_100():
    """All voxels at u = 100, 40 TP, 10 FP, 10 FN, 940 TN.  Below 100 nothing is kept: Dice 1 (empty), both ratios
    1; at 100 Dice is 80 / 100 and the ratios 0.  Thresholds 25, 50, 75, 100 over a span of 0.75:
    dice AUC = (0.25 + 0.25 + 0.25 * 0.9) / 0.75, ratio AUCs = (0.25 + 0.25 + 0.125) / 0.75."""
    from gts.uncertainty import qu_from_histogram

    hist = _hist()
    hist[:, TP, 100], hist[:, FP, 100], hist[:, FN, 100], hist[:, TN, 100] = 40, 10, 10, 940
    for s in qu_from_histogram(hist).values():
        assert s["dice"] == [1.0, 1.0, 1.0, 0.8] and s["ftp"] == [1.0, 1.0, 1.0, 0.0] == s["ftn"]
        assert abs(s["dice_auc"] - 0.725 / 0.75) < 1e-12
        assert abs(s["ftp_auc"] - 0.625 / 0.75) < 1e-12 and abs(s["ftn_auc"] - 0.625 / 0.75) < 1e-12
        assert abs(s["qu"] - (0.725 / 0.75 + 2 * (1 - 0.625 / 0.75)) / 3) < 1e-12


def test_empty_region_on_both_sides():
    """No voxel of the region in prediction or truth, every voxel TN with u spread over 0..100: Dice is 1 at every
    threshold, the filtered-TP ratio 0 (TP_100 = 0), the filtered-TN ratio what the spread says."""
    from gts.uncertainty import qu_from_histogram

    hist = _hist()
    hist[:, TN, 0], hist[:, TN, 60], hist[:, TN, 100] = 50, 25, 25
    s = qu_from_histogram(hist)["ET"]
    assert s["dice"] == [1.0] * 4 and s["ftp"] == [0.0] * 4 and s["ftn"] == [0.5, 0.5, 0.25, 0.0]
    assert s["dice_auc"] == 1.0 and s["ftp_auc"] == 0.0
    assert abs(s["ftn_auc"] - (0.25 * 0.5 + 0.25 * 0.375 + 0.25 * 0.125) / 0.75) < 1e-12
    empty = qu_from_histogram(_hist())["WT"]                       # no voxels at all
    assert empty["qu"] == 1.0 and empty["ftn"] == [0.0] * 4


def test_a_single_threshold_is_its_own_auc():
    from gts.uncertainty import qu_from_histogram

    hist = _hist()
    hist[:, TP, 10], hist[:, TP, 90] = 30, 10
    hist[:, FP, 10], hist[:, FN, 90] = 5, 5
    hist[:, TN, 0], hist[:, TN, 70] = 900, 100
    s = qu_from_histogram(hist, thresholds=[50])["CT"]
    assert s["dice"] == [60 / 65] and s["ftp"] == [0.25] and s["ftn"] == [0.1]
    assert s["dice_auc"] == 60 / 65 and s["ftp_auc"] == 0.25 and s["ftn_auc"] == 0.1
    assert abs(s["qu"] - (60 / 65 + 0.75 + 0.9) / 3) < 1e-12


@pytest.mark.parametrize("thresholds", [(25, 50, 75, 100), (0,), (100,), (0, 1, 2, 50, 99, 100),
                                        (10, 20, 30, 40, 50, 60, 70, 80)])
@pytest.mark.parametrize("seed", [0, 1])
def test_histogram_route_equals_the_mask_route(seed, thresholds):
    from gts.uncertainty import qu_from_histogram

    pred, truth, unc = R.random_case(4099, seed)
    if seed:
        pred[pred == 3] = 0                                        # no predicted enhancing tumour
        truth[truth == 3] = 2
    got = qu_from_histogram(R.histogram(pred, truth, unc), thresholds)
    want = R.qu_scores(pred, truth, unc, thresholds)
    assert list(got) == ["WT", "CT", "ET"]
    for region in got:
        assert set(got[region]) == {"qu", "dice_auc", "ftp_auc", "ftn_auc", "dice", "ftp", "ftn"}
        for field, value in got[region].items():
            assert np.allclose(value, want[region][field], rtol=0, atol=1e-12), (region, field)
    assert 0.0 < got["WT"]["qu"] < 1.0


def test_histogram_and_thresholds_are_checked():
    from gts.uncertainty import MAX_THRESHOLDS, check_thresholds, qu_from_histogram

    assert MAX_THRESHOLDS == 8 and check_thresholds([0, 100]) == (0, 100)
    for bad in ((), tuple(range(9)), (101,), (-1,), (50, 50), (75, 25), (2.5,)):
        with pytest.raises(ValueError):
            check_thresholds(bad)
    for shape in ((3, 4, 100), (2, 4, 102), (3, 4)):
        with pytest.raises(ValueError):
            qu_from_histogram(np.zeros(shape, dtype=np.int64))
    torch_hist = torch.zeros(3, 4, 102, dtype=torch.int64)
    assert qu_from_histogram(torch_hist)["WT"]["qu"] == 1.0


def test_row_formula_of_the_reference_on_hand_cases():
    """T = 16, region sums 1, 3, 5, 7: 200 * min(p, 1 - p) = 12.5, 37.5, 62.5, 87.5, round-half-to-even."""
    sums = np.array([[15, 0, 0, 1], [13, 0, 0, 3], [11, 0, 0, 5], [9, 0, 0, 7], [8, 8, 0, 0], [0, 0, 0, 16],
                     [np.nan, 0, 0, 1], [0, np.nan, 4, 4]], dtype=np.float32)
    u = R.row_uncertainty(sums, 16)
    assert u[2].tolist() == [12, 38, 62, 88, 0, 0, 12, 50]
    assert u[0].tolist() == [12, 38, 62, 88, 100, 0, 12, 100] and u[1].tolist() == [12, 38, 62, 88, 0, 0, 12, 100]


# ------------------------------------------------------------------------------------------------ files and flags
def test_map_file_names():
    from gts.uncertainty import map_file_names

    assert map_file_names("BraTS_007") == ("BraTS_007_unc_whole.nii.gz", "BraTS_007_unc_core.nii.gz",
                                           "BraTS_007_unc_enhance.nii.gz")


def test_uncertainty_flag_runs_a_one_member_ensemble():
    from scripts import ensemble_flags, generate_gnn_predictions, generate_joint_predictions, segment_scans

    args = segment_scans.build_parser().parse_args(["-d", "in", "-o", "out", "-g", "g.pt", "-c", "c.pt",
                                                    "--uncertainty_dir", "~/maps"])
    members = ensemble_flags.from_args(args, "g.pt", "c.pt")
    assert (members.gnn, members.cnn, members.axes) == (["g.pt"], ["c.pt"], "")
    assert members.describe() == "1 member(s) x 1 view(s)"
    assert ensemble_flags.uncertainty_dir(args).endswith("/maps") and "~" not in ensemble_flags.uncertainty_dir(args)
    args = segment_scans.build_parser().parse_args(["-d", "in", "-o", "out", "-g", "g.pt", "--uncertainty_dir", "m"])
    members = ensemble_flags.from_args(args, "g.pt", "")
    assert members.gnn == ["g.pt"] and members.cnn is None
    args = generate_joint_predictions.build_parser().parse_args(["-g", "g.pt", "-c", "c.pt", "--uncertainty_dir", "m",
                                                                 "--tta_mirror", "x"])
    assert ensemble_flags.from_args(args, "g.pt", "c.pt").axes == "x"
    args = generate_gnn_predictions.build_parser().parse_args(["-w", "g.pt", "--uncertainty_dir", "m"])
    assert ensemble_flags.from_args(args, "g.pt", None, "preds").cnn is None
    plain = segment_scans.build_parser().parse_args(["-d", "in", "-o", "out", "-g", "g.pt", "-c", "c.pt"])
    assert plain.uncertainty_dir is None and ensemble_flags.uncertainty_dir(plain) is None
    assert ensemble_flags.from_args(plain, "g.pt", "c.pt") is None


SEGMENT = ["-d", "nowhere", "-o", "nowhere_out", "-g", "g0.pt"]
SCORE = ["-d", "nowhere", "-s", "nowhere_preds", "-o", "nowhere.csv"]
BAD_FLAGS = [
    ("segment_scans", SEGMENT + ["--conform", "--uncertainty_dir", "maps"], "--conform"),
    ("segment_scans", SEGMENT + ["-c", "c0.pt", "--tta_mirror", "x", "--conform", "--uncertainty_dir", "maps"],
     "--conform"),
    ("generate_gnn_predictions", ["-d", "nowhere/", "-o", "nowhere_out", "-w", "g0.pt", "-f", "logits",
                                  "--uncertainty_dir", "maps"], "-f preds"),
    ("score_predictions", SCORE + ["--uncertainty_dir", "maps", "--qu_thresholds"] + [str(t) for t in range(9)],
     "between 1 and 8"),
    ("score_predictions", SCORE + ["--uncertainty_dir", "maps", "--qu_thresholds", "50", "101"], "0..100"),
    ("score_predictions", SCORE + ["--uncertainty_dir", "maps", "--qu_thresholds", "50", "50"], "ascending"),
    ("score_predictions", SCORE + ["--uncertainty_dir", "maps", "--qu_thresholds", "75", "25"], "ascending"),
    ("score_predictions", SCORE + ["--qu_thresholds", "25", "75"], "--uncertainty_dir"),
]


@pytest.mark.parametrize("cli,argv,word", BAD_FLAGS)
def test_flag_errors_come_before_any_scan_is_read(cli, argv, word, capsys, tmp_path, monkeypatch):
    """Exit status 2 and one line on stderr; the paths do not exist, nothing is created and torch.cuda never asked."""
    import os

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU was asked for"))
    module = importlib.import_module(f"scripts.{cli}")
    assert module.main(argv) == 2
    err = capsys.readouterr().err
    assert err.startswith(f"{cli}: ") and word in err and len(err.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


def test_the_flag_errors_are_flag_errors():
    from scripts import ensemble_flags, score_predictions, segment_scans

    args = segment_scans.build_parser().parse_args(SEGMENT + ["--conform", "--uncertainty_dir", "maps"])
    with pytest.raises(ensemble_flags.FlagError):
        ensemble_flags.from_args(args, "g0.pt", "")
    for values in ([str(t) for t in range(9)], ["101"], ["50", "50"], ["75", "25"]):
        args = score_predictions.build_parser().parse_args(SCORE + ["--uncertainty_dir", "m", "--qu_thresholds"]
                                                           + values)
        with pytest.raises(ensemble_flags.FlagError):
            score_predictions.qu_thresholds(args)
    args = score_predictions.build_parser().parse_args(SCORE + ["--uncertainty_dir", "m"])
    assert score_predictions.qu_thresholds(args) == (25, 50, 75, 100)
    assert score_predictions.qu_thresholds(score_predictions.build_parser().parse_args(SCORE)) is None


def test_csv_header_with_and_without_the_flag(tmp_path):
    from scripts import score_predictions as sp

    qu = ["WT_qu", "WT_qu_dice_auc", "WT_qu_ftp_auc", "WT_qu_ftn_auc", "CT_qu", "CT_qu_dice_auc", "CT_qu_ftp_auc",
          "CT_qu_ftn_auc", "ET_qu", "ET_qu_dice_auc", "ET_qu_ftp_auc", "ET_qu_ftn_auc"]
    assert sp.header_for() == sp.HEADER and sp.header_for((1.0,)) == sp.header_for((1.0,), qu=False)
    assert sp.header_for(qu=True) == sp.HEADER + qu
    assert sp.header_for((1.0, 2.0), qu=True) == sp.header_for((1.0, 2.0)) + qu
    row = [0.5, 1.0, 0.5, 2.0, 3, 1, 0] * 3
    sp.write_csv(str(tmp_path / "plain.csv"), {"a": row})
    sp.write_csv(str(tmp_path / "qu.csv"), {"a": row + [0.75, 0.5, 0.125, 0.25] * 3}, qu=True)
    plain = open(tmp_path / "plain.csv").read().splitlines()
    with_qu = open(tmp_path / "qu.csv").read().splitlines()
    assert plain[0] == ",".join(sp.HEADER) and with_qu[0] == ",".join(sp.HEADER + qu)
    for a, b in zip(plain, with_qu):
        assert b.startswith(a + ",")
    assert with_qu[1].endswith(",0.75,0.5,0.125,0.25") and len(with_qu) == 3


def test_uint8_maps_are_pasted_at_the_crop():
    from data_processing.image_processing import uncrop_maps_to_brats_size

    mask = np.zeros((240, 240, 155), dtype=bool)
    mask[3:5, 7:10, 150:155] = True
    crop = np.ix_(mask.any(axis=(1, 2)), mask.any(axis=(0, 2)), mask.any(axis=(0, 1)))
    maps = np.arange(3 * 2 * 3 * 5, dtype=np.uint8).reshape(3, 2, 3, 5) + 1
    full = uncrop_maps_to_brats_size(crop, maps)
    assert full.dtype == np.uint8 and full.shape == (3, 240, 240, 155)
    assert np.array_equal(full[:, 3:5, 7:10, 150:155], maps) and int((full != 0).sum()) == maps.size
    with pytest.raises(ValueError):
        uncrop_maps_to_brats_size(crop, maps.astype(np.int16))


# ------------------------------------------------------------------------------------------------ operand checks
def test_wrappers_and_entry_points_check_operands_before_a_launch(hip_lib):
    import gts
    from gts import _lib, ops

    assert _lib.ABI_VERSION == 34 and hip_lib.gts_abi_version() == 34 and ops.UNCERTAINTY_BINS == 102
    box = ops.CropBox([0, 2], [1], [0, 1, 3], (3, 2, 4), "cpu")
    with pytest.raises(gts.GtsError, match="MI355X only"):
        ops.region_uncertainty_rows(torch.zeros(6, 4), 2, box)
    for bad in (torch.zeros(6, 3), torch.zeros(5, 4), torch.zeros(6, 4).double(), torch.zeros(2, 1, 3, 5)):
        with pytest.raises(gts.GtsError):
            ops.region_uncertainty_rows(bad, 2, box)
    for terms in (0, -1, 1.5, 2 ** 31 + 1):
        with pytest.raises(gts.GtsError, match="terms"):
            ops.region_uncertainty_rows(torch.zeros(6, 4), terms, box)
    svs = torch.zeros(2, 3, dtype=torch.int16)
    with pytest.raises(gts.GtsError, match="MI355X only"):
        ops.region_uncertainty_nodes(svs, torch.zeros(5, 4), 1)
    for bad_svs, bad_total in ((svs.int(), torch.zeros(5, 4)), (svs, torch.zeros(5, 3)), (svs, torch.zeros(20, 1, 4))):
        with pytest.raises(gts.GtsError):
            ops.region_uncertainty_nodes(bad_svs, bad_total, 1)
    pred, unc = torch.zeros(10, dtype=torch.int16), torch.zeros(3, 10, dtype=torch.uint8)
    with pytest.raises(gts.GtsError, match="MI355X only"):
        ops.uncertainty_histogram(pred, pred, unc)
    for p, t, u in ((pred.int(), pred, unc), (pred, pred[:9], unc), (pred, pred, unc.int()), (pred, pred, unc[:2]),
                    (pred, pred, torch.zeros(3, 9, dtype=torch.uint8))):
        with pytest.raises(gts.GtsError):
            ops.uncertainty_histogram(p, t, u)
    # the C entry points reject what they cannot run, and accept an empty problem, without a device
    lib, one = hip_lib, ctypes.c_void_p(16)
    rows = lib.gts_region_uncertainty_rows_u8
    assert rows(one, one, one, one, one, 2, 2, 2, 4, 4, 4, 3, 8, None) == -2          # three classes
    assert rows(one, one, one, one, one, 2, 2, 2, 4, 4, 4, 5, 8, None) == -2
    assert rows(one, one, one, one, one, -1, 2, 2, 4, 4, 4, 4, 8, None) == -2         # negative extents
    assert rows(one, one, one, one, one, 2, 2, -2, 4, 4, 4, 4, 8, None) == -2
    assert rows(one, one, one, one, one, 2, 5, 2, 4, 4, 4, 4, 8, None) == -2          # a box wider than the volume
    assert rows(one, one, one, one, one, 5, 2, 2, 4, 4, 4, 4, 8, None) == -2
    assert rows(one, one, one, one, one, 2048, 1024, 1024, 4096, 4096, 4096, 4, 8, None) == -2    # 2^31 rows
    assert rows(one, one, one, one, one, 2, 2, 2, 4, 4, 4, 4, 0, None) == -2          # T < 1
    assert rows(one, one, one, one, one, 2, 2, 2, 4, 4, 4, 4, -3, None) == -2
    assert rows(None, one, one, one, one, 2, 2, 2, 4, 4, 4, 4, 8, None) == -1
    assert rows(one, one, None, one, one, 2, 2, 2, 4, 4, 4, 4, 8, None) == -1
    assert rows(one, one, one, one, None, 2, 2, 2, 4, 4, 4, 4, 8, None) == -1
    assert rows(None, None, None, None, None, 0, 2, 2, 4, 4, 4, 4, 8, None) == 0      # an empty box
    nodes = lib.gts_region_uncertainty_nodes_u8
    assert nodes(one, one, one, 10, 5, 3, 2, None) == -2
    assert nodes(one, one, one, -1, 5, 4, 2, None) == -2
    assert nodes(one, one, one, 10, -1, 4, 2, None) == -2
    assert nodes(one, one, one, 10, 32769, 4, 2, None) == -2
    assert nodes(one, one, one, 10, 5, 4, 0, None) == -2
    assert nodes(None, one, one, 10, 5, 4, 2, None) == -1
    assert nodes(one, None, one, 10, 5, 4, 2, None) == -1
    assert nodes(one, one, None, 10, 5, 4, 2, None) == -1
    assert nodes(None, None, None, 0, 5, 4, 2, None) == 0
    hist = lib.gts_uncertainty_histogram
    assert hist(one, one, one, one, -1, None) == -2
    assert hist(one, one, one, one, 2 ** 40 + 1, None) == -2
    for k in range(4):
        operands = [one] * 4
        operands[k] = None
        assert hist(*operands, 10, None) == -1
    assert hist(None, None, None, None, 0, None) == 0
