"""Uncertainty maps on the MI355X: U1 / U1n (region_uncertainty_rows / _nodes) bit for bit against the numpy
formula of tests/uncertainty_ref.py, U2 (uncertainty_histogram) against numpy counts, qu_scores against the
mask-based score, the predictor's maps, and the command lines.  Every comparison is exact unless it says 1e-12."""
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from gts import ops
from tests import uncertainty_ref as R
from tests.dataset_util import write_dataset
from tests.test_gpu_joint import _box, _nets

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gnn-tumor-seg_amd")
ROWS = (1, 63, 64, 65, 257, 4099)
TERMS = (1, 8, 24, 40)


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _e1_sums(rows, terms, seed):
    """fp32 [rows, 4]: what E1 leaves for `terms` random logit sets."""
    gen = torch.Generator().manual_seed(seed)
    sets = [(3.0 * torch.randn(rows, 4, generator=gen)).to(DEV) for _ in range(terms)]
    return ops.softmax_accumulate(sets).cpu().numpy()


def _planted(terms):
    """Rows at the edges of the formula for `terms` terms."""
    t = np.float32(terms)
    above = np.nextafter(t, np.float32(np.inf))
    return np.array([[0, 0, 0, 0],                      # all zero: certain healthy
                     [0, 0, 0, t], [0, t, 0, 0],        # exactly T in one class: p = 1 where the class counts
                     [0, 0, 0, above], [0, above, 0, 0],                 # p just above 1: clamped
                     [0, np.nan, 0, 1], [np.nan, 0, 0, np.nan], [0, 0, np.inf, -np.inf],      # NaN: 100
                     [t / 2, 0, 0, t / 2], [t / 2, t / 4, t / 4, 0],     # p = 1/2
                     [t + 1, 0, 0, -1], [0, 0, np.inf, 0]], dtype=np.float32)


def _line_box(rows):
    """A box over a [rows, 1, 1] volume that takes every voxel: the maps are then the rows in order."""
    return ops.CropBox(np.arange(rows), [0], [0], (rows, 1, 1), DEV)


def _u1(sums, terms, box=None):
    box = box or _line_box(len(sums))
    return ops.region_uncertainty_rows(torch.from_numpy(sums).to(DEV), terms, box).cpu().numpy()


# ------------------------------------------------------------------------------------------------ U1
@pytest.mark.parametrize("terms", TERMS)
def test_rows_equal_the_numpy_formula_bit_for_bit(terms):
    for rows in ROWS:
        sums = _e1_sums(rows, terms, seed=rows * 100 + terms)
        planted = _planted(terms)
        at = np.arange(len(planted)) * max(1, rows // len(planted)) % rows
        if rows > len(planted):
            sums[at] = planted
        got = _u1(sums, terms)
        assert got.dtype == np.uint8 and got.shape == (3, rows, 1, 1)
        assert np.array_equal(got.reshape(3, rows), R.row_uncertainty(sums, terms)), (rows, terms)
        assert got.max() <= 100
    planted = _planted(terms)
    got = _u1(planted, terms).reshape(3, -1)
    assert np.array_equal(got, R.row_uncertainty(planted, terms))
    assert not got[:, :5].any() and not got[:, 10:].any()            # certain, p = 1, and the clamps on both sides
    assert got[0, 5] == 100 and got[1, 5] == got[2, 5] == int(np.rint(200.0 * min(1 / terms, 1 - 1 / terms)))
    assert got[:, 6].tolist() == [100, 100, 100] and got[:, 7].tolist() == [100, 100, 0]      # -inf alone clamps to 0
    assert got[:, 8].tolist() == [100, 100, 100] and got[:, 9].tolist() == [100, 50, 0]


def test_round_half_even_ties_at_16_terms():
    """Region sums 1, 3, 5, 7 of 16: 200 * min(p, 1 - p) = 12.5, 37.5, 62.5, 87.5 -> 12, 38, 62, 88."""
    sums = np.array([[15, 0, 0, 1], [13, 0, 0, 3], [11, 0, 0, 5], [9, 0, 0, 7],
                     [15, 1, 0, 0], [13, 1, 1, 1], [11, 0, 5, 0], [9, 2, 2, 3]], dtype=np.float32)
    got = _u1(sums, 16).reshape(3, -1)
    assert got[:, :4].tolist() == [[12, 38, 62, 88]] * 3
    assert got[0, 4:].tolist() == [12, 38, 62, 88] and got[1, 4:].tolist() == [0, 25, 62, 62]
    assert np.array_equal(got, R.row_uncertainty(sums, 16))


@pytest.mark.parametrize("rows", [1, 65, 4099])
def test_unaligned_sums_give_the_same_bytes(rows):
    """16-byte loads when the pointer allows them; a tensor that starts 4 bytes into its buffer goes through scalar
    loads."""
    sums = torch.from_numpy(_e1_sums(rows, 8, seed=rows)).to(DEV)
    shifted = torch.empty(rows * 4 + 1, device=DEV)[1:].view(rows, 4)
    shifted.copy_(sums)
    assert sums.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    box = _line_box(rows)
    aligned = ops.region_uncertainty_rows(sums, 8, box)
    assert torch.equal(aligned, ops.region_uncertainty_rows(shifted, 8, box))
    assert np.array_equal(aligned.cpu().numpy().reshape(3, rows), R.row_uncertainty(sums.cpu().numpy(), 8))


def test_boxes_scatter_and_leave_zero_outside():
    small = ops.CropBox([0, 2, 3, 6], [3], [1, 2, 4, 8], (7, 5, 9), DEV)        # gaps and an extent of 1
    large = _box((33, 17, 70), seed=9)
    assert large.shape[0] * large.shape[1] * large.shape[2] > 4 * 256 and large.shape != (33, 17, 70)
    for box, terms in ((small, 8), (large, 24)):
        rows = box.shape[0] * box.shape[1] * box.shape[2]
        sums = _e1_sums(rows, terms, seed=rows)
        want = np.zeros((3,) + box.volume_shape, dtype=np.uint8)
        ref = R.row_uncertainty(sums, terms)
        assert ref.any()
        for r in range(3):
            want[r][box.as_ix()] = ref[r].reshape(box.shape)
        got = ops.region_uncertainty_rows(torch.from_numpy(sums).to(DEV), terms, box)
        assert np.array_equal(got.cpu().numpy(), want)
        four_d = ops.region_uncertainty_rows(torch.from_numpy(sums).to(DEV).view(*box.shape, 4), terms, box)
        assert torch.equal(got, four_d)


# ------------------------------------------------------------------------------------------------ U1n
@pytest.mark.parametrize("n_nodes", [1, 5, 300])
def test_node_maps_follow_the_partitioning(n_nodes):
    rng = np.random.default_rng(n_nodes)
    for shape, terms in (((9, 7, 11), 3), ((1, 1, 1), 1), ((33, 17, 5), 8)):
        svs = rng.integers(-(n_nodes + 3), n_nodes + 3, size=shape).astype(np.int16)    # background and stray ids
        svs.reshape(-1)[0] = -1
        sums = _e1_sums(n_nodes, terms, seed=n_nodes + terms)
        ids = svs.astype(np.int64)
        row = np.where(ids < 0, ids + n_nodes + 1, ids)
        valid = (row >= 0) & (row < n_nodes)
        want = np.zeros((3,) + shape, dtype=np.uint8)
        want[:, valid] = R.row_uncertainty(sums, terms)[:, row[valid]]
        for table in (torch.from_numpy(sums).to(DEV), None):
            if table is None:                           # 4 bytes into its buffer: the scalar loads
                table = torch.empty(n_nodes * 4 + 1, device=DEV)[1:].view(n_nodes, 4)
                table.copy_(torch.from_numpy(sums))
            got = ops.region_uncertainty_nodes(torch.from_numpy(svs).to(DEV), table, terms)
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (shape, terms)
        labels = ops.project_argmax(torch.from_numpy(svs).to(DEV), torch.from_numpy(sums).to(DEV)).cpu().numpy()
        assert not labels[~valid].any()                 # the same voxels are background for K12


# ------------------------------------------------------------------------------------------------ U2
def _cases(n):
    random = R.random_case(n, seed=n)
    calm = (np.zeros(n, np.int16), np.zeros(n, np.int16), np.zeros((3, n), np.uint8))
    one_bin = (np.full(n, 3, np.int16), np.full(n, 3, np.int16), np.full((3, n), 37, np.uint8))
    return {"random": random, "all TN at 0": calm, "one bin": one_bin}


def _hist(pred, truth, unc):
    return ops.uncertainty_histogram(torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV),
                                     torch.from_numpy(unc).to(DEV))


# the issue's sizes, and two multiples of 8: only those take the 16-byte groups
@pytest.mark.parametrize("n", [1, 63, 4099, 70001, 4104, 70008])
def test_histogram_equals_numpy_counts(n):
    for name, (pred, truth, unc) in _cases(n).items():
        got = _hist(pred, truth, unc)
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, 4, 102)
        want = R.histogram(pred, truth, unc)
        assert np.array_equal(got.cpu().numpy(), want), (n, name)
        assert int(got.sum()) == 3 * n
        assert torch.equal(got, _hist(pred, truth, unc))                               # two runs
    assert int(_hist(*_cases(n)["one bin"])[:, 0, 37].sum()) == 3 * n
    assert int(_hist(*_cases(n)["all TN at 0"])[:, 3, 0].sum()) == 3 * n


def test_histogram_of_unaligned_operands():
    """Label arrays that start 2 bytes into their buffers: one voxel per lane instead of the 16-byte groups."""
    pred, truth, unc = R.random_case(4104, seed=5)
    want = R.histogram(pred, truth, unc)
    p = torch.empty(4105, dtype=torch.int16, device=DEV)[1:]
    p.copy_(torch.from_numpy(pred))
    assert p.data_ptr() % 16 == 2
    got = ops.uncertainty_histogram(p, torch.from_numpy(truth).to(DEV), torch.from_numpy(unc).to(DEV))
    assert np.array_equal(got.cpu().numpy(), want)
    volume = ops.uncertainty_histogram(p.view(27, 152), torch.from_numpy(truth).to(DEV).view(27, 152),
                                       torch.from_numpy(unc).to(DEV).view(3, 27, 152))
    assert torch.equal(got, volume)


def test_histogram_refuses_bad_values():
    from gts import GtsError

    pred, truth, unc = R.random_case(4099, seed=1)
    high = unc.copy()
    high[1, 4000] = 101
    with pytest.raises(GtsError, match="above 100"):
        _hist(pred, truth, high)
    for side in (0, 1):
        labels = [pred.copy(), truth.copy()]
        labels[side][17] = 4
        with pytest.raises(GtsError, match="outside 0..3"):
            _hist(labels[0], labels[1], unc)
    negative = pred.copy()
    negative[0] = -1
    with pytest.raises(GtsError, match="outside 0..3"):
        _hist(negative, truth, unc)


@pytest.mark.parametrize("thresholds", [(25, 50, 75, 100), (50,), (0, 10, 20, 30, 40, 60, 80, 100)])
def test_qu_scores_against_the_mask_route(thresholds):
    from gts.uncertainty import qu_scores

    pred, truth, unc = R.random_case(70001, seed=len(thresholds))
    got = qu_scores(torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV), torch.from_numpy(unc).to(DEV),
                    thresholds)
    want = R.qu_scores(pred, truth, unc, thresholds)
    for region in R.REGIONS:
        for field, value in want[region].items():
            assert np.allclose(got[region][field], value, rtol=0, atol=1e-12), (region, field)


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def members():
    return [_nets(0), _nets(1)]


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    from data_processing.data_loader import ImageGraphDataset

    data = str(tmp_path_factory.mktemp("uncertainty") / "data") + "/"
    write_dataset(data, 2)
    with redirect_stdout(io.StringIO()):
        ds = ImageGraphDataset(data, "BraTS_", read_image=True, read_graph=True, read_label=False)
        return [(graph, np.asarray(feats), np.ascontiguousarray(img),
                 np.ascontiguousarray(ds.get_supervoxel_partitioning(mri))) for mri, graph, feats, img in ds]


@pytest.mark.parametrize("kind", ["two members", "eight views"])
def test_predict_joint_returns_the_maps_of_its_probabilities(members, samples, kind):
    """T = 2 and T = 8: the division by T in fp32 is exact, so probabilities * T are the sums the maps were made of."""
    from gts.ensemble import EnsemblePredictor, mirror_views

    if kind == "two members":
        predictor = EnsemblePredictor([g for g, _ in members], [c for _, c in members])
    else:
        predictor = EnsemblePredictor([members[0][0]], [members[0][1]], mirror_views("xyz"))
    terms = predictor.terms
    assert terms == (2 if kind == "two members" else 8)
    seen = 0
    for graph, feats, img, svs in samples:
        plain = predictor.predict_joint(graph, feats, img, svs)
        labels, unc = predictor.predict_joint(graph, feats, img, svs, return_uncertainty=True)
        assert np.array_equal(labels, plain) and labels.dtype == np.int16
        assert isinstance(unc, np.ndarray) and unc.dtype == np.uint8 and unc.shape == (3,) + svs.shape
        labels2, unc2, probs, box = predictor.predict_joint(graph, feats, img, svs, return_probabilities=True,
                                                            return_uncertainty=True)
        assert np.array_equal(labels2, plain) and np.array_equal(unc2, unc)
        _, probs_only, _ = predictor.predict_joint(graph, feats, img, svs, return_probabilities=True)
        assert torch.equal(probs, probs_only)
        sums = (probs.view(-1, 4) * terms).cpu().numpy()
        want = np.zeros_like(unc)
        ref = R.row_uncertainty(sums, terms)
        for r in range(3):
            want[r][box.as_ix()] = ref[r].reshape(box.shape)
        assert np.array_equal(unc, want)
        seen += int(unc.any())
    assert seen                                         # random nets are unsure somewhere


def test_predict_gnn_returns_the_maps_of_its_node_probabilities(members, samples):
    from gts.ensemble import EnsemblePredictor
    from scripts.cleanup import Cleanup

    predictor = EnsemblePredictor([g for g, _ in members])
    for graph, feats, img, svs in samples:
        plain = predictor.predict_gnn(graph, feats, svs)
        labels, unc = predictor.predict_gnn(graph, feats, svs, return_uncertainty=True)
        assert np.array_equal(labels, plain) and unc.dtype == np.uint8 and unc.shape == (3,) + svs.shape
        sums = (predictor.node_probabilities(graph, feats) * 2).cpu().numpy()
        n = len(sums)
        ids = svs.astype(np.int64)
        row = np.where(ids < 0, ids + n + 1, ids)
        valid = (row >= 0) & (row < n)
        want = np.zeros_like(unc)
        want[:, valid] = R.row_uncertainty(sums, 2)[:, row[valid]]
        assert np.array_equal(unc, want) and unc.any() and not unc[:, ~valid].any()
        relabel = torch.tensor([0, 2, 1, 4], dtype=torch.int16, device=DEV)
        cleaned, unc_cleaned = predictor.predict_gnn(graph, feats, svs, relabel,
                                                     cleanup=Cleanup(min_component_voxels=200), return_uncertainty=True)
        assert np.array_equal(unc_cleaned, unc)         # the clean-up changes labels only
        assert np.array_equal(cleaned, predictor.predict_gnn(graph, feats, svs, relabel,
                                                             cleanup=Cleanup(min_component_voxels=200)))


# ------------------------------------------------------------------------------------------------ command lines
def _save_full_size_nets(folder, seed):
    from model.networks import CnnRefinementNet, init_graph_net
    from utils.hyperparam_helpers import EvalParamSet

    torch.manual_seed(seed)
    gnn, cnn = os.path.join(folder, f"gnn_f{seed}.pt"), os.path.join(folder, f"cnn_f{seed}.pt")
    torch.save(init_graph_net("GSpool", EvalParamSet(20, 4, [256] * 4, None, None)).state_dict(), gnn)
    torch.save(CnnRefinementNet(8, 4, [16]).state_dict(), cnn)
    return gnn, cnn


def _read_maps(folder, scan_id):
    from data_processing import nifti_io
    from gts.uncertainty import map_file_names

    return np.stack([nifti_io.read_nifti(os.path.join(folder, name), np.uint8) for name in map_file_names(scan_id)])


def _stored_dtype_code(path):
    import gzip
    import struct

    with gzip.open(path, "rb") as f:
        return struct.unpack_from("<h", f.read(72), 70)[0]


def test_prediction_clis_write_the_predictors_maps(tmp_path):
    """generate_joint_predictions and generate_gnn_predictions with --uncertainty_dir on the synthetic dataset: the
    maps are the predictor's, pasted at the crop; the label files are byte-identical to a run without the flag."""
    from data_processing.data_loader import ImageGraphDataset
    from data_processing.image_processing import uncrop_maps_to_brats_size
    from data_processing.labels import INTERNAL_TO_BRATS
    from gts.uncertainty import map_file_names
    from scripts import ensemble_flags
    from scripts import generate_gnn_predictions as gen
    from scripts import generate_joint_predictions as joint

    data = str(tmp_path / "data") + "/"
    write_dataset(data, 1)
    g0, c0 = _save_full_size_nets(str(tmp_path), 1)
    j = lambda *p: str(tmp_path.joinpath(*p))          # noqa: E731
    base = ["-d", data, "-p", "BraTS_", "-g", g0, "-c", c0, "--tta_mirror", "x"]
    with redirect_stdout(io.StringIO()):
        assert joint.main(base + ["-o", j("with"), "--uncertainty_dir", j("maps")]) == 0
        assert joint.main(base + ["-o", j("without")]) == 0
        assert gen.main(["-d", data, "-p", "BraTS_", "-w", g0, "-o", j("gnn"), "--uncertainty_dir", j("gnn_maps")]) == 0
        ds = ImageGraphDataset(data, "BraTS_", read_image=True, read_graph=True, read_label=False)
        predictor = ensemble_flags.Members([g0], [c0], "x").predictor("GSpool")
        gnn_only = ensemble_flags.Members([g0], None, "").predictor()
    relabel = torch.from_numpy(INTERNAL_TO_BRATS).to(DEV)
    for mri, graph, feats, img in ds:
        assert open(j("with", f"{mri}.nii.gz"), "rb").read() == open(j("without", f"{mri}.nii.gz"), "rb").read()
        assert sorted(os.listdir(j("maps"))) == sorted(map_file_names(mri))
        assert all(_stored_dtype_code(j("maps", name)) == 2 for name in map_file_names(mri))          # uint8
        svs, crop = ds.get_supervoxel_partitioning(mri), ds.get_crop(mri)
        _, unc = predictor.predict_joint(graph, feats, img, svs, relabel, return_uncertainty=True)
        got = _read_maps(j("maps"), mri)
        assert got.shape == (3, 240, 240, 155) and got.max() <= 100 and got.any()
        assert np.array_equal(got, uncrop_maps_to_brats_size(crop, unc))
        _, unc = gnn_only.predict_gnn(graph, feats, svs, relabel, return_uncertainty=True)
        assert np.array_equal(_read_maps(j("gnn_maps"), mri), uncrop_maps_to_brats_size(crop, unc))


def test_score_cli_appends_the_qu_columns(tmp_path, capsys):
    from data_processing import labels, nifti_io
    from gts.uncertainty import map_file_names
    from scripts import score_predictions as cli
    from tests import lesionwise_ref

    shape = (24, 22, 21)
    data, preds, maps = tmp_path / "data", tmp_path / "preds", tmp_path / "maps"
    preds.mkdir(), maps.mkdir()
    want = {}
    for i, scan in enumerate(["scan_a", "scan_b", "scan_c", "scan_d", "scan_e"]):
        pred, truth = lesionwise_ref.blobs_and_salt(shape, 60 + i)
        unc = R.random_case(pred.size, seed=i)[2].reshape((3,) + shape)
        (data / scan).mkdir(parents=True)
        nifti_io.save_as_nifti(labels.swap_labels_to_brats(truth), str(data / scan / f"{scan}_seg.nii.gz"))
        nifti_io.save_as_nifti(labels.swap_labels_to_brats(pred), str(preds / f"{scan}.nii.gz"))
        if scan == "scan_d":
            unc[2, 3, 3, 3] = 101                                  # a value above 100
        for r, name in enumerate(map_file_names(scan)):
            if scan == "scan_c" and r == 1:                        # a missing map
                continue
            volume = unc[r][:, :, :-1] if scan == "scan_e" and r == 2 else unc[r]        # a wrongly shaped map
            nifti_io.save_as_nifti(np.ascontiguousarray(volume), str(maps / name))
        if scan in ("scan_a", "scan_b"):
            want[scan] = R.qu_scores(pred, truth, unc, (10, 50, 100))
    common = ["-d", str(data), "-s", str(preds), "-p", "scan", "--min_lesion_voxels", "20"]
    assert cli.main(common + ["-o", str(tmp_path / "plain.csv")]) == 0
    capsys.readouterr()
    status = cli.main(common + ["-o", str(tmp_path / "qu.csv"), "--uncertainty_dir", str(maps), "--qu_thresholds",
                                "10", "50", "100"])
    printed = capsys.readouterr().out
    assert status == 1 and "2 scan(s) scored, 3 left out" in printed and "QU score" in printed
    for scan in ("scan_c", "scan_d", "scan_e"):
        assert f"{scan}: left out" in printed
    plain = {line.split(",")[0]: line for line in (tmp_path / "plain.csv").read_text().splitlines()}
    lines = (tmp_path / "qu.csv").read_text().splitlines()
    assert lines[0].split(",") == cli.header_for(qu=True) and lines[0].startswith(plain["id"] + ",")
    assert [line.split(",")[0] for line in lines[1:]] == ["scan_a", "scan_b", "mean"]
    for line in lines[1:3]:
        scan = line.split(",")[0]
        assert line.startswith(plain[scan] + ",")                  # the other columns are those of a run without
        cells = [float(c) for c in line.split(",")[len(cli.HEADER):]]
        ref = [want[scan][region][field] for region in R.REGIONS for field in ("qu", "dice_auc", "ftp_auc", "ftn_auc")]
        assert np.allclose(cells, ref, rtol=0, atol=1e-12), scan
    assert (tmp_path / "plain.csv").read_text().splitlines()[0] == ",".join(cli.HEADER)


# segment_scans on one synthetic raw scan with and without --uncertainty_dir, then score_predictions over what it
# wrote; one process, bounded by the subprocess timeout.
_E2E = r"""
import io, os, sys
import torch
from gts import synth_mri
from model.networks import CnnRefinementNet, init_graph_net
from utils.hyperparam_helpers import EvalParamSet
from scripts import score_predictions, segment_scans
tmp = sys.argv[1]
j = lambda *p: os.path.join(tmp, *p)
raw = j("raw")
synth_mri.write_sample(raw, "BraTS_000", 300)
torch.manual_seed(0)
hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
torch.save(init_graph_net("GSpool", hp).state_dict(), j("gnn.pt"))
torch.save(CnnRefinementNet(8, 4, [16]).state_dict(), j("cnn.pt"))
base = ["-d", raw, "-g", j("gnn.pt"), "-c", j("cnn.pt"), "-n", "6000", "--tta_mirror", "x"]
rc1 = segment_scans.main(base + ["-o", j("with"), "--uncertainty_dir", j("maps")])
rc2 = segment_scans.main(base + ["-o", j("without")])
rc3 = score_predictions.main(["-d", raw, "-s", j("with"), "-o", j("qu.csv"), "--uncertainty_dir", j("maps")])
rc4 = score_predictions.main(["-d", raw, "-s", j("without"), "-o", j("plain.csv")])
print("RC", rc1, rc2, rc3, rc4)
"""


@pytest.mark.timeout(600)
def test_segment_scans_writes_maps_that_score_predictions_scores(tmp_path):
    from data_processing import labels, nifti_io
    from gts.uncertainty import map_file_names
    from scripts import score_predictions as cli

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-c", _E2E, str(tmp_path)], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=550)
    assert r.returncode == 0 and "RC 0 0 0 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    with_flag = open(tmp_path / "with" / "BraTS_000.nii.gz", "rb").read()
    assert len(with_flag) > 0 and with_flag == open(tmp_path / "without" / "BraTS_000.nii.gz", "rb").read()
    assert sorted(os.listdir(tmp_path / "maps")) == sorted(map_file_names("BraTS_000"))
    assert all(_stored_dtype_code(str(tmp_path / "maps" / name)) == 2 for name in map_file_names("BraTS_000"))
    unc = _read_maps(str(tmp_path / "maps"), "BraTS_000")
    pred_file = nifti_io.read_nifti(str(tmp_path / "with" / "BraTS_000.nii.gz"), np.int16)
    assert unc.shape == (3,) + pred_file.shape and unc.max() <= 100 and unc.any()
    for name in map_file_names("BraTS_000"):
        assert np.array_equal(nifti_io.read_affine(str(tmp_path / "maps" / name))[0],
                              nifti_io.read_affine(str(tmp_path / "with" / "BraTS_000.nii.gz"))[0])
    pred = labels.swap_labels_from_brats_any(pred_file)
    truth = labels.swap_labels_from_brats_any(nifti_io.read_in_labels(str(tmp_path / "raw" / "BraTS_000"),
                                                                      "_seg.nii.gz"))
    want = R.qu_scores(pred, truth, unc)
    plain = (tmp_path / "plain.csv").read_text().splitlines()
    lines = (tmp_path / "qu.csv").read_text().splitlines()
    assert lines[0].split(",") == cli.header_for(qu=True) and len(lines) == 3
    for with_qu, without in zip(lines, plain):
        assert with_qu.startswith(without + ",")                   # the other columns equal a run without the flag
    cells = [float(c) for c in lines[1].split(",")[len(cli.HEADER):]]
    ref = [want[region][field] for region in R.REGIONS for field in ("qu", "dice_auc", "ftp_auc", "ftn_auc")]
    assert np.allclose(cells, ref, rtol=0, atol=1e-12)
