"""The host side of the lesion-wise scorer: the scipy reference of the definition (tests/lesionwise_ref.py) on
cases worked out by hand, the closed-form dilation footprint, and the CSV and label rules of
scripts/score_predictions.py.  No GPU."""
import numpy as np
import pytest

from tests import lesionwise_ref as ref


# 1. the footprint the device dilates by in one pass == n iterations of scipy's 18-neighbour structure
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_closed_form_footprint_equals_iterated_dilation(n):
    assert int(ref.closed_form_footprint(n).sum()) == (1, 19, 93, 263)[n]
    seed = np.zeros((2 * n + 5,) * 3, dtype=bool)
    seed[n + 2, n + 2, n + 2] = True
    want = ref.dilate(seed, n)
    assert np.array_equal(want[2:-2, 2:-2, 2:-2], ref.closed_form_footprint(n))
    rng = np.random.default_rng(n)
    for shape, p in (((9, 8, 11), 0.02), ((6, 13, 7), 0.2), ((1, 5, 9), 0.1), ((4, 1, 1), 0.5)):
        mask = rng.random(shape) < p
        assert np.array_equal(ref.dilate_closed_form(mask, n), ref.dilate(mask, n))      # clipped at the faces too


def _cube(shape, corner, side=4):
    vol = np.zeros(shape, dtype=bool)
    vol[tuple(slice(c, c + side) for c in corner)] = True
    return vol


# 2. one 4^3 cube and its copy shifted by one voxel along x
def test_cube_and_its_shifted_copy_by_hand():
    truth, pred = _cube((16, 16, 16), (4, 4, 4)), _cube((16, 16, 16), (5, 4, 4))
    got = ref.region_scores(pred, truth)
    # 3 of the 4 planes overlap: tp = 48, dice = 2 * 48 / (64 + 64)
    assert got["lesions"] == [dict(vol=64, tp=48, matched_voxels=64, scored=True, dice=0.75, hd95=1.0)]
    # borders: 56 voxels each (the cube less its inner 2^3).  Of the shifted cube's border, the 16 voxels of the
    # plane that left the cube and the 4 that now lie over the other's inner voxels are at distance 1, the other
    # 36 at 0, and the same the other way round: 72 zeros and 40 ones, whose 95th percentile is 1.
    assert (got["lw_dice"], got["lw_hd95"]) == (0.75, 1.0)
    assert (got["n_lesions"], got["n_scored"], got["n_fp"], got["n_fn"]) == (1, 1, 0, 0)
    assert got["lesion_roots"] == [1 + np.ravel_multi_index((1, 1, 4), truth.shape)]      # D reaches 3 out along x, y; not z too
    # a second predicted cube far away is a false positive: both sums gain one term
    far = pred | _cube((16, 16, 16), (12, 12, 12), 2)
    got = ref.region_scores(far, truth)
    assert (got["n_fp"], got["lw_dice"], got["lw_hd95"]) == (1, 0.75 / 2, (1.0 + 374.0) / 2)


# 3. the empty cases
def test_empty_cases():
    shape = (12, 12, 12)
    nothing = np.zeros(shape, dtype=bool)
    blob, speck = _cube(shape, (3, 3, 3)), _cube(shape, (3, 3, 3), 2)        # 64 voxels scored, 8 not
    both = ref.region_scores(nothing, nothing)
    assert (both["lw_dice"], both["lw_hd95"], both["n_lesions"], both["n_fp"]) == (1.0, 0.0, 0, 0)
    fp = ref.region_scores(speck, nothing)
    assert (fp["lw_dice"], fp["lw_hd95"], fp["n_fp"], fp["n_scored"]) == (0.0, 374.0, 1, 0)
    fn = ref.region_scores(nothing, blob)
    assert (fn["lw_dice"], fn["lw_hd95"], fn["n_fn"], fn["n_scored"]) == (0.0, 374.0, 1, 1)
    assert fn["lesions"][0]["dice"] == 0.0 and fn["lesions"][0]["hd95"] == 374.0
    unscored = ref.region_scores(nothing, speck)
    assert (unscored["lw_dice"], unscored["lw_hd95"], unscored["n_lesions"], unscored["n_scored"]) == (1.0, 0.0, 1, 0)
    assert unscored["lesions"][0]["scored"] is False and unscored["lesions"][0]["dice"] is None


def test_all_three_regions_and_the_legacy_numbers():
    from model import evaluation

    pred, truth = ref.blobs_and_salt((24, 22, 21), 5)
    got = ref.lesionwise_scores(pred, truth)
    legacy = evaluation.calculate_brats_metrics(pred, truth)
    assert [got[r]["dice"] for r in ref.REGIONS] == [float(v) for v in legacy[:3]]
    assert [got[r]["hd95"] for r in ref.REGIONS] == [float(v) for v in legacy[3:]]
    assert got["WT"]["n_lesions"] >= got["ET"]["n_lesions"] >= 1


# 4. the labels a file may hold
def test_label_conventions():
    from data_processing import labels

    old = np.array([[0, 1, 2, 4], [4, 4, 0, 2]], dtype=np.int16)
    new = np.where(old == 4, 3, old)
    want = labels.swap_labels_from_brats(old)
    assert want.tolist() == [[0, 2, 1, 3], [3, 3, 0, 1]]
    for given in (old, new):
        got = labels.swap_labels_from_brats_any(given)
        assert got.dtype == np.int16 and np.array_equal(got, want)
    for bad in ([0, 3, 4], [0, 5], [-1, 0], [0, 1, 2, 3, 4]):
        with pytest.raises(RuntimeError, match="unexpected label"):
            labels.swap_labels_from_brats_any(np.array(bad, dtype=np.int16))


# 5. the CSV
def test_csv_rows_and_mean(tmp_path):
    from scripts import score_predictions as cli

    assert cli.HEADER[:8] == ["id", "WT_dice", "WT_hd95", "WT_lw_dice", "WT_lw_hd95", "WT_n_scored", "WT_n_fp", "WT_n_fn"]
    assert len(cli.HEADER) == 22

    def record(dice, lw, n_fp):
        return dict(dice=dice, hd95=2.5, lw_dice=lw, lw_hd95=374.0, n_scored=2, n_fp=n_fp, n_fn=0, lesions=[])

    rows = {"b": cli.row_of({r: record(0.5, 0.25, 1) for r in cli.REGIONS}),
            "a": cli.row_of({r: record(1, 0.75, 2) for r in cli.REGIONS})}
    path = tmp_path / "out" / "scores.csv"
    cli.write_csv(str(path), rows)
    lines = path.read_text().splitlines()
    assert lines[0] == ",".join(cli.HEADER) and [line.split(",")[0] for line in lines[1:]] == ["a", "b", "mean"]
    assert lines[1].split(",")[1:8] == ["1.0", "2.5", "0.75", "374.0", "2", "2", "0"]
    assert lines[3].split(",")[1:8] == ["0.75", "2.5", "0.5", "374.0", "2", "1.5", "0"]
    assert all(float(v) == w for v, w in zip(lines[2].split(",")[1:], rows["b"]))      # floats round-trip
    cli.write_csv(str(path), {})
    assert path.read_text().splitlines() == [",".join(cli.HEADER)]


def test_cli_arguments():
    from scripts import score_predictions as cli

    args = cli.build_parser().parse_args(["-d", "D", "-s", "P", "-o", "S.csv"])
    assert (args.label_extension, args.data_prefix, args.dilation, args.min_lesion_voxels) == ("_seg.nii.gz", "", 3, 50)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["-d", "D", "-s", "P", "-o", "S.csv", "--dilation", "4"])
