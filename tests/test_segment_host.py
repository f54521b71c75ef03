"""Host side of the raw-scan segmenter (scripts/segment_scans.py, gts/intake.py): the quantile formula
that turns I2's order statistics into normalize_img's tops, the raw NIfTI reader, scan discovery, the
CLI's defaults and the argument checks of the I1-I3 entry points.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

from data_processing import nifti_io
from gts import intake

SIZES = [1, 2, 3, 199, 200, 201, 10 ** 5, 8_928_000]


def _check_quantile(x):
    n = x.size
    lo, hi = intake.quantile_ranks(n)
    s = np.sort(x)
    got = intake.quantile_from_order_stats(s[lo], s[hi], n)
    want = np.quantile(x, 0.995).astype(np.float32)
    assert got.dtype == np.float32
    assert got.tobytes() == want.tobytes(), (n, got, want)


@pytest.mark.parametrize("n", SIZES)
def test_quantile_matches_numpy_continuous(n):
    rng = np.random.default_rng(n)
    _check_quantile((rng.standard_normal(n) * 300.0 + 500.0).astype(np.float32))
    _check_quantile(rng.uniform(0.0, 1e-3, n).astype(np.float32))


@pytest.mark.parametrize("n", SIZES)
def test_quantile_matches_numpy_integer_ties(n):
    rng = np.random.default_rng(1000 + n)
    x = rng.integers(0, 7, n).astype(np.float32) * 311.0
    x[rng.random(n) < 0.5] = 0.0                    # half the voxels are background
    _check_quantile(x)
    _check_quantile(rng.integers(0, 4000, n).astype(np.float32))


def test_quantile_ranks_are_numpys():
    for n in SIZES:
        vi = (n - 1) * np.float32(0.995)            # np.quantile casts q to the data's float32
        lo, hi = intake.quantile_ranks(n)
        assert lo == (n - 1 if n == 1 else int(np.floor(vi))) and hi == min(lo + 1, n - 1)


def test_raw_reader_agrees_with_read_nifti(tmp_path):
    rng = np.random.default_rng(0)
    vol16 = rng.integers(-100, 3000, (13, 7, 5)).astype(np.int16)
    vol32 = rng.standard_normal((13, 7, 5)).astype(np.float32)
    for name, vol in (("a.nii.gz", vol16), ("b.nii.gz", vol32), ("c.nii", vol16)):
        fp = str(tmp_path / name)
        nifti_io.save_as_nifti(vol, fp)
        raw = nifti_io.read_nifti_raw(fp)
        assert raw.dtype == vol.dtype and raw.shape == vol.shape
        assert np.array_equal(raw, vol)
        assert np.array_equal(raw.astype(np.float32), nifti_io.read_nifti(fp, np.float32))
        assert raw.T.flags.c_contiguous                      # x fastest, as the file stores it
    fp = str(tmp_path / "u8.nii.gz")                          # any other dtype converts to float32
    nifti_io.save_as_nifti(vol16.astype(np.uint8), fp)
    assert nifti_io.read_nifti_raw(fp).dtype == np.float32


def test_raw_reader_falls_back_for_scaled_files(tmp_path):
    import gzip
    import struct

    vol = np.arange(60, dtype=np.int16).reshape(5, 4, 3)
    fp = str(tmp_path / "s.nii.gz")
    nifti_io.save_as_nifti(vol, fp)
    with gzip.open(fp, "rb") as f:
        raw = bytearray(f.read())
    struct.pack_into("<ff", raw, 112, 2.0, 1.5)
    with gzip.open(fp, "wb") as f:
        f.write(bytes(raw))
    got = nifti_io.read_nifti_raw(fp)
    assert got.dtype == np.float32
    assert np.array_equal(got, vol.astype(np.float32) * 2.0 + 1.5)
    assert np.array_equal(got, nifti_io.read_nifti(fp, np.float32))


def test_stage_scan_layout():
    rng = np.random.default_rng(3)
    vols = [np.asfortranarray(rng.integers(0, 100, (6, 5, 4)).astype(np.int16)) for _ in range(4)]
    host = intake.stage_scan(vols, pin=False).numpy()
    assert host.dtype == np.int16 and host.shape == (4, 4, 5, 6)
    for c in range(4):
        assert np.array_equal(host[c], vols[c].T)
    mixed = intake.stage_scan(vols[:3] + [vols[3].astype(np.float32)], pin=False).numpy()
    assert mixed.dtype == np.float32 and np.array_equal(mixed[0], vols[0].T.astype(np.float32))
    with pytest.raises(ValueError):
        intake.stage_scan(vols[:3], pin=False)


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").close()


def test_both_input_layouts_are_discovered(tmp_path):
    from scripts import segment_scans

    exts = ["_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"]
    one = tmp_path / "docker_input"
    for ext in exts:
        _touch(str(one / ("BraTS2021_00012" + ext)))
    assert segment_scans.find_inputs(str(one), exts) == {"BraTS2021_00012": str(one)}
    many = tmp_path / "many"
    for sid in ("BraTS_001", "BraTS_002", "Other_003"):
        for ext in exts:
            _touch(str(many / sid / (sid + ext)))
    found = segment_scans.find_inputs(str(many), exts)
    assert sorted(found) == ["BraTS_001", "BraTS_002", "Other_003"]
    assert os.path.normpath(found["BraTS_002"]) == str(many / "BraTS_002")
    assert sorted(segment_scans.find_inputs(str(many), exts, "BraTS")) == ["BraTS_001", "BraTS_002"]
    paths = nifti_io.find_modality_files(found["BraTS_001"], exts)
    assert [os.path.basename(p) for p in paths] == ["BraTS_001" + e for e in exts]
    os.remove(paths[2])
    with pytest.raises(FileNotFoundError):
        nifti_io.find_modality_files(found["BraTS_001"], exts)


def test_parser_defaults_follow_preprocess_dataset():
    from scripts import preprocess_dataset, segment_scans

    seg = segment_scans.build_parser().parse_args(["-d", "in", "-o", "out", "-g", "g.pt"])
    pre = preprocess_dataset.build_parser().parse_args([])
    for name in ("num_nodes", "boxiness", "num_neighbors", "modality_extensions", "data_prefix"):
        assert getattr(seg, name) == getattr(pre, name), name
    assert seg.gnn_type == "GSpool" and seg.cnn_weights == ""
    args = segment_scans.build_parser().parse_args(
        ["-d", "in", "-o", "out", "-g", "g.pt", "-c", "c.pt", "-m", "GSmean", "-n", "900", "-b", "0.25", "-k", "0",
         "-M", "_a.nii", "_b.nii", "_c.nii", "_d.nii", "-p", "X"])
    assert (args.num_nodes, args.boxiness, args.num_neighbors, args.gnn_type) == (900, 0.25, 0, "GSmean")
    assert args.modality_extensions == ["_a.nii", "_b.nii", "_c.nii", "_d.nii"] and args.data_prefix == "X"


def test_intake_entries_reject_bad_arguments(hip_lib):
    one = ctypes.c_void_p(16)
    p3 = (one, one, one)
    # I1: NULL, shape, dtype
    assert hip_lib.gts_intake_occupancy(None, 4, 8, 8, 8, *p3, one, None) == -1
    assert hip_lib.gts_intake_occupancy(one, 4, 0, 8, 8, *p3, one, None) == -2
    assert hip_lib.gts_intake_occupancy(one, 4, 5000, 8, 8, *p3, one, None) == -2
    assert hip_lib.gts_intake_occupancy(one, 4, 4096, 4096, 4096, *p3, one, None) == -2
    assert hip_lib.gts_intake_occupancy(one, 2, 8, 8, 8, *p3, one, None) == -3
    ws = int(hip_lib.gts_intake_select_workspace())
    assert ws > 0
    # I2: NULL, crop larger than the volume, ranks outside [0, n), short workspace, dtype
    args = lambda **kw: [kw.get("src", one), kw.get("dt", 16), 8, 8, 8, one, kw.get("cx", 4), one, 4, one, 4,
                         kw.get("lo", 0), kw.get("hi", 63), one, one, kw.get("ws", ws), None]
    assert hip_lib.gts_intake_order_stats(*args(src=None)) == -1
    assert hip_lib.gts_intake_order_stats(*args(cx=9)) == -2
    assert hip_lib.gts_intake_order_stats(*args(cx=0)) == -2
    assert hip_lib.gts_intake_order_stats(*args(hi=64)) == -2
    assert hip_lib.gts_intake_order_stats(*args(lo=-1)) == -2
    assert hip_lib.gts_intake_order_stats(*args(lo=5, hi=4)) == -2
    assert hip_lib.gts_intake_order_stats(*args(ws=ws - 1)) == -2
    assert hip_lib.gts_intake_order_stats(*args(dt=8)) == -3
    # I3: NULL params, crop, dtype
    assert hip_lib.gts_intake_standardize(one, 4, 8, 8, 8, one, 4, one, 4, one, 4, None, one, None) == -1
    assert hip_lib.gts_intake_standardize(one, 4, 8, 8, 8, one, 4, one, 9, one, 4, one, one, None) == -2
    assert hip_lib.gts_intake_standardize(one, 64, 8, 8, 8, one, 4, one, 4, one, 4, one, one, None) == -3
