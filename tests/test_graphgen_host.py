"""Graph generation, host side (no GPU): the SLIC grid, the host C connectivity pass and kNN greedy
of libgts_hip.so against the numpy restatement / reference fixtures, argument checks through the
C ABI, and the preprocess_dataset CLI surface."""
import ctypes
import os

import numpy as np
import pytest
from scipy.spatial.distance import cdist

from tests import graphgen_ref as R
from gts import graphgen as gg

GRID_CASES = [((40, 48, 36), 300), ((240, 240, 155), 15000), ((140, 170, 140), 15000), ((2, 100, 100), 500),
              ((1, 50, 60), 100), ((3, 4, 200), 50), ((5, 5, 5), 200), ((96, 112, 80), 1500), ((7, 300, 9), 40)]


@pytest.mark.parametrize("shape,n", GRID_CASES)
def test_regular_grid_matches_the_restatement(shape, n):
    assert gg.regular_grid(shape, n) == R.regular_grid(shape, n)
    coords, step, window = gg.slic_grid(shape, n)
    assert coords.shape[1] == 3 and step == float(max(R._steps(R.regular_grid(shape, n))))
    assert window == R._steps(R.regular_grid(shape, coords.shape[0]))


# (shape, n) -> per-axis (start, step), worked out by hand from the algorithm:
# step = (prod / n) ** (1/3) unless a sorted dimension is below it, then the walk over the sorted
# dimensions; start = floor(float step / 2), step = round(float step), axes unsorted again
GRID_PINS = [
    ((40, 48, 36), 300, [(3, 6), (3, 6), (3, 6)]),            # 230.4 ** (1/3) = 6.13
    ((240, 240, 155), 15000, [(4, 8), (4, 8), (4, 8)]),       # 595.2 ** (1/3) = 8.41
    ((2, 100, 100), 500, [(1, 2), (2, 4), (2, 4)]),           # thin axis: 2, then sqrt(20) = 4.47
    ((1, 50, 60), 100, [(0, 1), (2, 5), (2, 5)]),             # 1, then sqrt(30) = 5.48
    ((3, 4, 200), 50, [(1, 3), (2, 4), (2, 4)]),              # 3, then sqrt(16) = 4
    ((7, 300, 9), 40, [(3, 7), (4, 8), (4, 8)]),              # 7, then sqrt(67.5) = 8.22; axes unsorted
    ((100, 2, 3), 10, [(5, 10), (1, 2), (1, 3)]),             # two walk steps: 2, 3, then 100 / 10
    ((5, 5, 5), 200, [(None, None)] * 3),                     # fewer voxels than points: every voxel
]


@pytest.mark.parametrize("shape,n,want", GRID_PINS)
def test_regular_grid_pinned_values(shape, n, want):
    got = [(None if s.start is None else int(s.start), None if s.step is None else int(s.step))
           for s in gg.regular_grid(shape, n)]
    assert got == want


def _blocky_labels(rng, shape, block, n_labels, noise):
    coarse = rng.integers(0, n_labels, size=tuple(-(-s // block) for s in shape))
    lab = np.kron(coarse, np.ones((block,) * 3, dtype=np.int64))[:shape[0], :shape[1], :shape[2]]
    flip = rng.random(shape) < noise
    lab[flip] = rng.integers(0, n_labels, size=int(flip.sum()))
    return lab.astype(np.int32)


@pytest.mark.parametrize("seed,shape,block,n_labels,noise,min_size,max_size", [
    (1, (12, 14, 10), 3, 6, 0.05, 5, 40),     # truncation at max_size splits big regions
    (2, (10, 11, 9), 2, 3, 0.2, 12, 30),      # many small components merge (chains through relabelled ones)
    (3, (8, 9, 10), 4, 4, 0.0, 100, 1000),    # the first component is small: it "merges" into label 0
    (4, (16, 6, 13), 5, 8, 0.1, 1, 7),
    (5, (9, 9, 9), 1, 2, 0.0, 3, 3),
])
def test_connectivity_matches_the_restatement(hip_lib, seed, shape, block, n_labels, noise, min_size, max_size):
    lab = _blocky_labels(np.random.default_rng(seed), shape, block, n_labels, noise)
    got, n = gg.enforce_connectivity(lab, min_size, max_size)
    want = R.connectivity_ref(lab, min_size, max_size)
    assert np.array_equal(got, want)
    assert n == want.max() + 1


@pytest.mark.parametrize("case", [c.name for c in R.CASES])
def test_connectivity_on_the_fixture_slic_labels(hip_lib, golden_dir, case):
    f = np.load(os.path.join(golden_dir, f"ref_graphgen_{case}.npz"))
    got, n = gg.enforce_connectivity(f["slic_labels"], int(f["min_size"]), int(f["max_size"]))
    assert np.array_equal(got, f["conn_labels"]) and n == int(f["n_sv"])


@pytest.mark.parametrize("case", [c.name for c in R.CASES])
def test_knn_greedy_matches_the_reference(hip_lib, golden_dir, case):
    f = np.load(os.path.join(golden_dir, f"ref_graphgen_{case}.npz"))
    pos = f["node_centroids"]
    order = np.argsort(cdist(pos, pos), axis=1, kind="stable")
    n = len(pos)
    for k, key in ((10, "knn10"), (int(f["k_big"]), "knn_big")):
        cand = np.full((n, k), -1, dtype=np.int32)
        for i in range(n):
            js = order[i][order[i] > i][:k]
            cand[i, :len(js)] = js
        picks = gg.knn_greedy(cand, k)
        rows = np.repeat(np.arange(n), k).reshape(n, k)
        got = sorted(zip(rows[picks >= 0].tolist(), picks[picks >= 0].tolist()))
        assert got == sorted(map(tuple, f[key].tolist()))


def test_graphgen_arguments_are_checked_before_any_launch(hip_lib):
    one = ctypes.c_void_p(16)
    assert hip_lib.gts_gg_knn_candidates_f64(one, 100, 33, one, None) == -2            # k above GTS_GG_MAX_K
    assert hip_lib.gts_gg_knn_candidates_f64(one, 32768, 10, one, None) == -2          # more than 32767 nodes
    assert hip_lib.gts_gg_knn_candidates_f64(None, 100, 10, one, None) == -1
    assert hip_lib.gts_gg_sv_stats(one, one, None, 4, 4, 4, 4, 32768, one, one, one, one, None) == -2
    assert hip_lib.gts_gg_discard_f64(one, one, one, 32768, 20, one, 64, one, one, one, one, one, one, one, None) == -2
    assert hip_lib.gts_gg_touching_count_i16(one, 4, 4, 4, 40000, one, one, None) == -2
    assert hip_lib.gts_gg_touching_workspace(32768) == -2
    # beyond int32 voxel indexing
    assert hip_lib.gts_gg_gaussian_f64(one, one, one, one, 4, 1.0, 1024, 1024, 1024, 4, None) == -2
    assert hip_lib.gts_gg_slic_assign_f64(one, one, 10, 2048, 1024, 1024, 1, 2, 2, 2, 0.1, one, one, one, None) == -2
    assert hip_lib.gts_gg_slic_assign_f64(one, one, 10, 8, 8, 8, 9, 2, 2, 2, 0.1, one, one, one, None) == -2
    assert hip_lib.gts_gg_gaussian_f64(one, one, one, one, 17, 1.0, 8, 8, 8, 1, None) == -2
    n = ctypes.c_int32()
    lab = np.zeros((2, 2, 2), dtype=np.int32)
    assert hip_lib.gts_gg_enforce_connectivity(lab.ctypes.data, lab.ctypes.data, 2, 2, 2, 1, 0, one, ctypes.byref(n)) == -2
    bad = np.array([[1], [0]], dtype=np.int32)                   # row 1 names j = 0 <= i
    picks = np.empty_like(bad)
    e = ctypes.c_int64()
    got = np.empty(2, dtype=np.int32)
    assert hip_lib.gts_gg_knn_greedy(bad.ctypes.data, 2, 1, picks.ctypes.data, got.ctypes.data, ctypes.byref(e)) == -2
    assert hip_lib.gts_gg_knn_greedy(bad.ctypes.data, 2, 1, picks.ctypes.data, None, ctypes.byref(e)) == -1
    with pytest.raises(ValueError):
        gg.knn_candidates(np.zeros((4, 3)), 33)


def test_preprocess_cli_flags_match_the_reference():
    from scripts import preprocess_dataset as cli

    args = cli.build_parser().parse_args([])
    assert (args.data_dir, args.num_nodes, args.num_neighbors, args.boxiness, args.output_dir) == (None, 15000, 10, 0.5, None)
    assert args.modality_extensions == ["_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"]
    assert (args.label_extension, args.data_prefix) == (None, "")
    short = cli.build_parser().parse_args(["-d", "x", "-n", "7", "-k", "0", "-b", "0.2", "-o", "y", "-m", "_a", "_b",
                                           "-l", "_seg.nii.gz", "-p", "BraTS"])
    assert (short.data_dir, short.num_nodes, short.num_neighbors, short.boxiness, short.output_dir) == ("x", 7, 0, 0.2, "y")
    assert short.modality_extensions == ["_a", "_b"] and (short.label_extension, short.data_prefix) == ("_seg.nii.gz", "BraTS")
    assert cli.STANDARDIZATION_STATS == ([0.4645, 0.6625, 0.4064, 0.3648], [0.1593, 0.1703, 0.1216, 0.1627])
    assert cli.LABEL_MAP == {4: 3, 2: 1, 1: 2}
    assert np.array_equal(cli.swap_labels_from_brats(np.array([0, 1, 2, 4])), [0, 2, 1, 3])
    import Filepaths

    gen = cli.DataPreprocessor(cli.build_parser().parse_args(["-d", "/nonexistent/"]))
    assert gen.output_dir == f"{Filepaths.PROCESSED_DATA_DIR}_15000_0.5_10"


def test_normalize_and_standardize_follow_the_reference():
    from data_processing.image_processing import normalize_img, standardize_img

    img = np.random.default_rng(0).random((6, 5, 4, 3)).astype(np.float32)
    maxes = np.quantile(img, 0.995, axis=(0, 1, 2)).astype(np.float32)
    assert np.array_equal(normalize_img(img), img / maxes) and normalize_img(img).dtype == np.float32
    flat = img.reshape(-1, 3)
    assert np.array_equal(normalize_img(flat, is_flat=True), flat / np.quantile(flat, 0.995, axis=0).astype(np.float32))
    mean, std = np.float32([0.1, 0.2, 0.3]), np.float32([1.5, 2.0, 0.5])
    assert np.array_equal(standardize_img(img, mean, std), (img - mean) / std)


def test_nifti_patient_sample_round_trip(tmp_path):
    from data_processing import nifti_io
    from gts import synth_mri

    img, lab = synth_mri.make_sample(3, shape=(20, 18, 12))
    folder = synth_mri.write_sample(str(tmp_path), "BraTS_x", 3, shape=(20, 18, 12))
    got = nifti_io.read_in_patient_sample(folder, list(synth_mri.MODALITY_EXTS))
    assert got.dtype == np.float32 and np.array_equal(got, img)
    assert np.array_equal(nifti_io.read_in_labels(folder, "_seg.nii.gz"), lab)
    assert set(np.unique(lab)) <= {0, 1, 2, 4}
    with pytest.raises(FileNotFoundError):
        nifti_io.read_in_labels(folder, "_missing.nii.gz")
