"""Dataset standardization statistics, host side: the numpy restatement against the reference fixture, the
statistics file, the command line flags and the medians (no GPU)."""
import ctypes
import json

import numpy as np
import pytest

from data_processing import standardization
from gts import dataset_stats, synth_mri
from scripts import compute_dataset_stats, preprocess_dataset, segment_scans
from tests import dataset_stats_ref as R

BRATS = ["_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"]
CONSTANTS = ([0.4645, 0.6625, 0.4064, 0.3648], [0.1593, 0.1703, 0.1216, 0.1627])


def test_reference_form_equals_the_reference_fixture(golden_dir):
    fx = np.load(f"{golden_dir}/ref_dataset_stats.npz")
    assert len(fx["seeds"]) == len(R.FIXTURE_SCANS) == 5
    means, stds = [], []
    for i, (seed, shape) in enumerate(R.FIXTURE_SCANS):
        assert (int(fx["seeds"][i]), tuple(fx["shapes"][i])) == (seed, shape)
        img, lab = synth_mri.make_sample(seed, shape)
        assert R.digest(img) == str(fx["image_digests"][i]) and R.digest(lab) == str(fx["label_digests"][i])
        mu, sigma = R.reference_form(img, lab)
        assert mu.dtype == np.float32 and sigma.dtype == np.float32
        assert mu.tobytes() == fx["scan_mean"][i].tobytes(), (i, mu, fx["scan_mean"][i])
        assert sigma.tobytes() == fx["scan_std"][i].tobytes(), (i, sigma, fx["scan_std"][i])
        means.append(mu)
        stds.append(sigma)
    mean, std = dataset_stats.dataset_stats(list(zip(means, stds)))
    assert mean.tobytes() == fx["dataset_mean"].tobytes() and std.tobytes() == fx["dataset_std"].tobytes()


def test_dataset_stats_is_the_median_for_odd_and_even_counts():
    rng = np.random.default_rng(0)
    for count in (1, 4, 5):
        rows = [dataset_stats.ScanStats(10, np.ones(4, np.float32), rng.random(4).astype(np.float32),
                                        rng.random(4).astype(np.float32)) for _ in range(count)]
        mean, std = dataset_stats.dataset_stats(rows)
        assert mean.dtype == np.float32 and std.dtype == np.float32
        assert np.array_equal(mean, np.median([r.mean for r in rows], axis=0))
        assert np.array_equal(std, np.median([r.std for r in rows], axis=0))
    even = [(np.float32([1, 2, 3, 4]), np.float32([1, 1, 1, 1])), (np.float32([3, 2, 1, 0]), np.float32([2, 2, 2, 2]))]
    mean, std = dataset_stats.dataset_stats(even)
    assert mean.tolist() == [2, 2, 2, 2] and std.tolist() == [1.5] * 4
    with pytest.raises(ValueError):
        dataset_stats.dataset_stats([])


def _scan(seed):
    rng = np.random.default_rng(seed)
    return dataset_stats.ScanStats(int(rng.integers(1, 10**6)), *(rng.random(4).astype(np.float32) + 0.1 for _ in range(3)))


def test_stats_file_round_trip(tmp_path):
    per_scan = {f"s{i}": _scan(i) for i in range(3)}
    mean, std = dataset_stats.dataset_stats(list(per_scan.values()))
    path = str(tmp_path / "stats.json")
    standardization.save_stats(path, mean, std, BRATS, 0.995, per_scan)
    got_mean, got_std = standardization.load_stats(path, BRATS)
    assert got_mean.dtype == np.float32 and got_mean.tobytes() == mean.tobytes() and got_std.tobytes() == std.tobytes()
    assert standardization.load_stats(path)[0].tobytes() == mean.tobytes()      # no list given: not compared
    doc = json.load(open(path))
    assert set(doc) == {"mean", "std", "modality_extensions", "quantile", "n_scans", "scans"}
    assert doc["modality_extensions"] == BRATS and doc["quantile"] == 0.995 and doc["n_scans"] == 3
    for sid, s in per_scan.items():
        assert doc["scans"][sid]["n"] == s.n
        for name in ("top", "mean", "std"):
            assert np.float32(doc["scans"][sid][name]).tobytes() == getattr(s, name).tobytes()


def _write(tmp_path, **changes):
    doc = {"mean": CONSTANTS[0], "std": CONSTANTS[1], "modality_extensions": BRATS, "quantile": 0.995, "n_scans": 0,
           "scans": {}}
    doc.update(changes)
    path = str(tmp_path / "stats.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    return path


def test_load_stats_rejections(tmp_path):
    assert standardization.load_stats(_write(tmp_path), BRATS)[0].tolist() == np.float32(CONSTANTS[0]).tolist()
    cases = [
        (dict(mean=[0.1, 0.2, 0.3]), "exactly 4 modalities"),
        (dict(std=[0.1, 0.2, 0.3, 0.4, 0.5]), "exactly 4 modalities"),
        (dict(mean=[[0.1, 0.2, 0.3, 0.4]]), "exactly 4 modalities"),
        (dict(mean=[0.1, float("nan"), 0.3, 0.4]), "non-finite"),
        (dict(std=[0.1, float("inf"), 0.3, 0.4]), "non-finite"),
        (dict(std=[0.1, 0.0, 0.3, 0.4]), "must be positive"),
        (dict(std=[0.1, -0.2, 0.3, 0.4]), "must be positive"),
        (dict(mean="abcd"), "not a list of numbers"),
        (dict(modality_extensions=BRATS[::-1]), "same suffixes in the same order"),
        (dict(modality_extensions=BRATS[:3]), "same suffixes in the same order"),
        (dict(modality_extensions=["_a.nii", "_b.nii", "_c.nii", "_d.nii"]), "same suffixes in the same order"),
    ]
    for changes, message in cases:
        with pytest.raises(ValueError, match=message):
            standardization.load_stats(_write(tmp_path, **changes), BRATS)
    path = str(tmp_path / "broken.json")
    open(path, "w").write("{not json")
    with pytest.raises(ValueError, match="not a JSON"):
        standardization.load_stats(path, BRATS)
    open(path, "w").write(json.dumps({"mean": CONSTANTS[0]}))
    with pytest.raises(ValueError, match="needs 'mean' and 'std'"):
        standardization.load_stats(path, BRATS)


def test_parser_flags_and_defaults():
    args = compute_dataset_stats.build_parser().parse_args([])
    assert (args.data_dir, args.label_extension, args.data_prefix, args.output) == (None, None, "", None)
    assert args.modality_extensions == BRATS
    short = compute_dataset_stats.build_parser().parse_args(["-d", "x", "-l", "_seg.nii.gz", "-m", "_a", "_b", "-p",
                                                             "BraTS", "-o", "s.json"])
    assert (short.data_dir, short.label_extension, short.modality_extensions, short.data_prefix, short.output) == \
        ("x", "_seg.nii.gz", ["_a", "_b"], "BraTS", "s.json")
    assert preprocess_dataset.build_parser().parse_args([]).stats is None
    assert preprocess_dataset.build_parser().parse_args(["--stats", "compute"]).stats == "compute"
    assert preprocess_dataset.build_parser().parse_args(["--stats", "f.json"]).stats == "f.json"
    need = ["-d", "x", "-o", "y", "-g", "w.pt"]
    assert segment_scans.build_parser().parse_args(need).stats is None
    assert segment_scans.build_parser().parse_args(need + ["--stats", "f.json"]).stats == "f.json"


def test_compute_cli_needs_labels_and_four_modalities(tmp_path, capsys):
    with pytest.raises(SystemExit) as exc:
        compute_dataset_stats.main(["-d", str(tmp_path), "-o", str(tmp_path / "s.json")])
    assert exc.value.code != 0 and "need the label volumes (-l)" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        compute_dataset_stats.main(["-d", str(tmp_path), "-l", "_seg.nii.gz", "-m", "_a", "_b", "-o", str(tmp_path / "s.json")])
    assert exc.value.code != 0 and "exactly 4" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        compute_dataset_stats.main(["-d", str(tmp_path), "-l", "_seg.nii.gz"])
    assert not (tmp_path / "s.json").exists()


def test_preprocessor_statistics_sources(tmp_path):
    gen = preprocess_dataset.DataPreprocessor(preprocess_dataset.build_parser().parse_args(["-d", "/nonexistent/"]))
    assert gen.mean.dtype == np.float32 and gen.std.dtype == np.float32
    assert gen.mean.tobytes() == np.array(CONSTANTS[0], dtype=np.float32).tobytes()
    assert gen.std.tobytes() == np.array(CONSTANTS[1], dtype=np.float32).tobytes()
    path = _write(tmp_path, mean=[0.5, 0.6, 0.7, 0.8], std=[0.1, 0.2, 0.3, 0.4])
    gen = preprocess_dataset.DataPreprocessor(preprocess_dataset.build_parser().parse_args(
        ["-d", "/nonexistent/", "--stats", path]))
    assert gen.mean.tolist() == np.float32([0.5, 0.6, 0.7, 0.8]).tolist()
    assert gen.std.tolist() == np.float32([0.1, 0.2, 0.3, 0.4]).tolist()
    # another modality order behind -m: refused before anything is written
    out = tmp_path / "out"
    rc = preprocess_dataset.main(["-d", "/nonexistent/", "-o", str(out), "--stats", path, "-m", *BRATS[::-1]])
    assert rc not in (0, None) and not out.exists()


def test_argument_errors_do_not_need_a_gpu(hip_lib):
    one = ctypes.c_void_p(16)
    ws = hip_lib.gts_dataset_stats_workspace(240, 240, 155)
    vol = 240 * 240 * 155
    assert ws >= hip_lib.gts_intake_select_workspace() + vol // 8
    assert hip_lib.gts_dataset_stats_workspace(4097, 4, 4) == -2 and hip_lib.gts_dataset_stats_workspace(0, 4, 4) == -2
    small = hip_lib.gts_dataset_stats_workspace(8, 8, 8)
    mask, order, moments = hip_lib.gts_dataset_stats_mask, hip_lib.gts_dataset_stats_order_stats, \
        hip_lib.gts_dataset_stats_moments
    assert mask(None, 4, one, 8, 8, 8, one, one, small, None) == -1
    assert mask(one, 4, None, 8, 8, 8, one, one, small, None) == -1
    assert mask(one, 4, one, 8, 8, 8, None, one, small, None) == -1
    assert mask(one, 4, one, 8, 8, 8, one, None, small, None) == -1
    assert mask(one, 8, one, 8, 8, 8, one, one, small, None) == -3            # int32 volumes are not taken
    assert mask(one, 4, one, 4097, 8, 8, one, one, 1 << 40, None) == -2
    assert mask(one, 4, one, 8, 8, 8, one, one, small - 1, None) == -2
    assert order(None, 4, 8, 8, 8, 10, 0, 1, one, one, small, None) == -1
    assert order(one, 4, 8, 8, 8, 10, 0, 1, None, one, small, None) == -1
    assert order(one, 5, 8, 8, 8, 10, 0, 1, one, one, small, None) == -3
    assert order(one, 4, 8, 8, 8, 10, 0, 10, one, one, small, None) == -2       # rank past the members
    assert order(one, 4, 8, 8, 8, 0, 0, 0, one, one, small, None) == -2
    assert order(one, 4, 8, 8, 8, 10, 0, 1, one, one, small - 1, None) == -2
    assert order(one, 4, 8, 8, 4097, 10, 0, 1, one, one, 1 << 40, None) == -2
    top = (ctypes.c_float * 4)(1, 1, 1, 1)
    assert moments(None, 4, 8, 8, 8, 10, top, one, one, small, None) == -1
    assert moments(one, 4, 8, 8, 8, 10, None, one, one, small, None) == -1
    assert moments(one, 4, 8, 8, 8, 10, top, None, one, small, None) == -1
    assert moments(one, 3, 8, 8, 8, 10, top, one, one, small, None) == -3
    assert moments(one, 4, 8, 8, 8, 513, top, one, one, small, None) == -2      # more members than voxels
    assert moments(one, 4, 8, 8, 8, 10, top, one, one, small - 1, None) == -2
