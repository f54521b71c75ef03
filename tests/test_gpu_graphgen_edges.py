"""The graph-generation kernels (G1-G8 of csrc/gts_graphgen.hip) one stage at a time, at the shapes
where each takes a path the seeded volumes of test_gpu_graphgen.py never reach.  Every stage has a
bit-for-bit contract against numpy/scipy or the SLIC restatement (tests/graphgen_ref.py), so every
comparison is np.array_equal: there is no tolerance here.  tests/test_graphgen_ref_host.py shows, on
the references alone, that these inputs tell the contract from its nearest wrong neighbour."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import graphgen_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gg(hip_lib):
    from gts import graphgen

    return graphgen


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype).contiguous()


def _stream():
    from gts import _lib

    return _lib.current_stream()


# ---- G1 Gaussian -----------------------------------------------------------------------------------

GAUSS_SHAPES = [(1, 2, 3), (2, 1, 5, 3), (3, 7, 1, 2), (1, 1, 1), (17, 3, 2)]


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("sigma", [0.5, 1.0, 4.0])
@pytest.mark.parametrize("shape", GAUSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gaussian_on_lines_shorter_than_the_radius(gg, shape, sigma, scale):
    x = np.random.default_rng(len(shape) * 100 + shape[0]).standard_normal(shape)
    want = ndimage.gaussian_filter(x, [sigma] * 3 + [0] * (len(shape) - 3)) * scale
    got = gg.gaussian(x, sigma, scale)
    assert got.dtype == np.float64 and got.shape == shape
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", GAUSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gaussian_sigma_zero_only_scales(gg, shape):
    x = np.random.default_rng(5).standard_normal(shape)
    assert np.array_equal(gg.gaussian(x, 0, 2.0), x * 2.0)
    assert np.array_equal(gg.gaussian(x, 0.0, 1.0), x)


def test_gaussian_refuses_a_radius_of_17(gg):
    with pytest.raises(ValueError):
        gg.gaussian(np.zeros((4, 4, 4)), 4.2)
    gg.gaussian(np.zeros((4, 4, 4)), 4.0)       # radius 16 is the last one served


# ---- G3 SLIC update through the C ABI --------------------------------------------------------------

@pytest.mark.parametrize("c", [1, 3, 8])
@pytest.mark.parametrize("w", [65, 128, 130, 300])
def test_slic_update_on_boxes_wider_than_a_wave(hip_lib, w, c):
    """Segments interleave along x over the whole width, so every bounding box spans several runs
    of 64 lanes and most runs hold voxels of other segments; a label in the middle of the range
    owns nothing (its box stays unset, its row must still be written: NaN) and some voxels carry -1
    or n (nobody's)."""
    rng = np.random.default_rng(w * 10 + c)
    d, h = 3 + w % 2, 4 - w % 3
    n = 3 + (w + c) % 3 + 1                                     # 3-5 owning segments and the empty one
    dead = n // 2
    owners = np.array([k for k in range(n) if k != dead], dtype=np.int32)
    z, y, x = np.mgrid[:d, :h, :w]
    labels = owners[(x // 7 + y) % (n - 1)]
    labels[rng.random((d, h, w)) < 0.05] = -1
    labels[rng.random((d, h, w)) < 0.05] = n
    labels[:, :, 0] = labels[:, :, -1] = owners[np.arange(d * h) % (n - 1)].reshape(d, h)  # every box spans all of x
    assert (labels == -1).any() and (labels == n).any()
    img = rng.standard_normal((d, h, w, c))
    want = R.update_ref(img, labels, n)
    for k in owners:
        xs = np.flatnonzero((labels == k).any(axis=(0, 1)))
        rows = (np.diff((labels == k).astype(np.int8), axis=2, prepend=0) == 1).sum(axis=2)
        assert xs[-1] - xs[0] + 1 > 64 and rows.max() > 1       # wider than a wave, broken up inside a row
    centres = torch.full((n, 3 + c), 123.0, dtype=torch.float64, device="cuda")
    bbox = torch.empty(6 * n, dtype=torch.int32, device="cuda")
    img_t, labels_t = _dev(img, torch.float64), _dev(labels, torch.int32)
    code = hip_lib.gts_gg_slic_update_f64(img_t.data_ptr(), labels_t.data_ptr(), centres.data_ptr(), n, d, h, w, c,
                                          bbox.data_ptr(), _stream())
    assert code == 0
    got = centres.cpu().numpy()
    empty = np.isnan(want[:, 0])
    assert 0 < dead < n - 1 and empty.tolist() == [k == dead for k in range(n)]
    assert np.array_equal(got[~empty], want[~empty])
    assert np.isnan(want[empty]).all() and np.array_equal(got[empty], want[empty], equal_nan=True)


# ---- G2 SLIC assignment through the C ABI ----------------------------------------------------------

def _assign_case(name):
    """(scaled [D,H,W,C], centres [n, 3+C], window, spatial_weight, labels before)."""
    rng = np.random.default_rng(sorted(ASSIGN_CASES).index(name))
    if name == "uncovered":
        shape, c, window = (4, 4, 40), 2, (2, 2, 2)
        centres = np.array([[1.5, 1.5, 3.5], [1.5, 1.5, 36.0]])
    elif name == "ties":
        # a constant image, so every distance is spatial.  The exact ties: centres 0/1 and 5/6 are duplicates
        # (equal everywhere), 2/3 (x = 10, 14) are equidistant from the voxels at x = 12, and 7/8 from every voxel
        # of their mirror plane z + y = 5.  3/4 (x = 14, 17) mirror about x = 15.5, where no voxel lies: no tie
        shape, c, window = (5, 7, 30), 1, (2, 3, 4)
        centres = np.array([[2, 3, 6], [2, 3, 6], [2, 3, 10], [2, 3, 14], [2, 3, 17], [2, 3, 24], [2, 3, 24],
                            [1, 2, 20.5], [3, 4, 20.5]], dtype=np.float64)
    elif name == "borders":
        # fractional centres within one step of both borders of every axis, and a dead one
        shape, c, window = (9, 11, 23), 3, (2, 3, 5)
        centres = np.array([[0.25, 0.5, 0.75], [8.75, 10.4, 22.3], [1.9, 2.9, 4.9], [6.1, 7.2, 17.6],
                            [np.nan, np.nan, np.nan], [4.5, 5.5, 11.5], [0.0, 10.0, 3.3], [8.0, 0.1, 19.9]])
    elif name == "c8":
        shape, c, window = (6, 10, 12), 8, (2, 2, 2)
        centres = np.stack(np.meshgrid([1.3, 4.1], [2.2, 7.6], [2.5, 6.0, 9.4], indexing="ij"), -1).reshape(-1, 3)
    elif name == "one-centre":
        shape, c, window = (5, 6, 7), 1, (1, 1, 2)
        centres = np.array([[2.4, 2.6, 3.1]])
    scaled = np.full(shape + (c,), 0.375) if name == "ties" else rng.random(shape + (c,))
    colours = np.full((len(centres), c), 0.5) if name == "ties" else rng.random((len(centres), c))
    if name == "borders":
        colours[4] = np.nan
    before = np.full(shape, 7 if name == "uncovered" else 1000, dtype=np.int32)
    return scaled, np.concatenate([centres, colours], axis=1), window, 1.0 / max(window) ** 2, before


ASSIGN_CASES = ("uncovered", "ties", "borders", "c8", "one-centre")


@pytest.mark.parametrize("name", ASSIGN_CASES)
def test_slic_assign_windows_ties_and_channel_edges(hip_lib, name):
    scaled, centres, window, sw, before = _assign_case(name)
    want = R.assign_ref(scaled, centres, window, sw, before)
    # the reference itself shows that the case reaches what it is for
    if name == "uncovered":
        assert (want[:, :, 8:32] == 7).all() and (want[:, :, :8] == 0).all() and (want[:, :, 32:] == 1).all()
    if name == "ties":
        assert set(np.unique(want)) == {0, 2, 3, 4, 5, 7, 8}     # a duplicate never wins
        assert want[2, 3, 12] == 2 and want[2, 3, 20] == 7        # the lower index takes the tied voxels
        assert want[2, 3, 15] == 3 and want[2, 3, 16] == 4        # no tie: each side to its nearer centre
    if name == "borders":
        assert 4 not in want and (want == 1000).any() and {0, 1, 6, 7}.issubset(np.unique(want).tolist())
    if name == "one-centre":
        assert set(np.unique(want)) == {0, 1000}
    d, h, w, c = scaled.shape
    labels = _dev(before, torch.int32)
    best = torch.empty(d * h * w, dtype=torch.int64, device="cuda")
    winner = torch.empty(d * h * w, dtype=torch.int32, device="cuda")
    scaled_t, centres_t = _dev(scaled, torch.float64), _dev(centres, torch.float64)
    code = hip_lib.gts_gg_slic_assign_f64(scaled_t.data_ptr(), centres_t.data_ptr(), len(centres), d, h, w, c, *window,
                                          sw, labels.data_ptr(), best.data_ptr(), winner.data_ptr(), _stream())
    assert code == 0
    assert np.array_equal(labels.cpu().numpy(), want)


# ---- whole SLIC on wide segments -------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.WIDE_SLIC))
def test_slic_with_few_segments_on_a_long_axis(gg, name):
    shape, n, c, compactness = R.WIDE_SLIC[name]
    vol = R.striped_volume(name)
    scaled = ndimage.gaussian_filter(vol, [1, 1, 1, 0]) * (1.0 / compactness)
    want = R.slic_rounds_ref(scaled, n, 10)
    got, n_centres = gg.slic_rounds(gg.gaussian(vol, 1.0, 1.0 / compactness), n, 10)
    assert n_centres == want.max() + 1
    assert np.array_equal(got.cpu().numpy(), want)
    lo, hi = R.connectivity_sizes(shape, n)
    whole = gg.slic(vol, n_segments=n, compactness=compactness, sigma=1.0)
    assert np.array_equal(whole, R.connectivity_ref(want, lo, hi))


# ---- G5 statistics -----------------------------------------------------------------------------------

def _same_stats(got, want):
    for g, w_ in zip(got, want):
        assert g.dtype == w_.dtype and np.array_equal(g, w_, equal_nan=True)


def test_statistics_at_the_sort_sizes_with_absent_labels(gg):
    """Segments of 1, 2, 3, 5, 255-257, 4095, 4096 (last LDS size), 4097 and 9000 voxels (two spilled
    segments side by side in the global scratch), an absent label in the middle and at the end."""
    part, img, lab, n_sv = R.stats_edge_case()
    want = R.stats_ref(part, img, lab, n_sv)
    feats, cents, svl = want
    for k in (R.STATS_ABSENT, n_sv - 1):                         # the n == 0 contract, stated outright
        assert (feats[k] == -1.0).all() and np.isnan(cents[k]).all() and svl[k] == -1
    _same_stats(gg.supervoxel_statistics(part, img, lab, n_sv), want)
    _same_stats(gg.supervoxel_statistics(part, img, None, n_sv), R.stats_ref(part, img, None, n_sv))


@pytest.mark.parametrize("shape,n_sv", [((13, 16, 20), 1025), ((13, 16, 20), 2049), ((32, 32, 32), 32767)])
def test_statistics_beyond_one_scan_element_per_thread(gg, shape, n_sv):
    rng = np.random.default_rng(n_sv)
    n_vox = int(np.prod(shape))
    if n_sv == 32767:
        part = np.arange(n_vox, dtype=np.int32)
        part[-1] = 0                                             # voxel v owns label v; the last joins label 0
    else:
        part = rng.integers(0, n_sv, n_vox).astype(np.int32)     # about 2 or 4 voxels per label, some absent
        assert len(np.unique(part)) < n_sv and part.max() == n_sv - 1
    part = part.reshape(shape)
    img = rng.standard_normal(shape + (2,)).astype(np.float32)
    lab = rng.integers(-2, 3, shape).astype(np.int16)
    _same_stats(gg.supervoxel_statistics(part, img, lab, n_sv), R.stats_ref_grouped(part, img, lab, n_sv))


# ---- G6 discard --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_feat", [5, 20])
@pytest.mark.parametrize("pattern", ["all-but-min", "all-equal", "threshold"])
@pytest.mark.parametrize("n_sv", [1, 1024, 1025, 32767])
def test_discard_threshold_and_renumbering(gg, n_sv, pattern, n_feat):
    rng = np.random.default_rng(n_sv + n_feat)
    feats = rng.standard_normal((n_sv, n_feat))
    thr = 0.3 + 0.01
    if pattern == "all-but-min":
        feats[:, 4] = 1.0 + rng.random(n_sv)
        feats[n_sv // 3, 4] = 0.5
    elif pattern == "all-equal":
        feats[:, 4] = 0.25
    else:
        col = np.where(rng.random(n_sv) < 0.5, 0.3 + 0.0099 * rng.random(n_sv), thr + rng.random(n_sv))
        col[rng.random(n_sv) < 0.2] = thr                        # exactly min + 0.01 as fp64 forms it: kept
        col[rng.random(n_sv) < 0.2] = np.nextafter(thr, -np.inf)  # one ulp below: dropped
        col[n_sv // 2] = 0.3
        if n_sv > 2:
            col[0], col[n_sv - 1] = thr, np.nextafter(thr, -np.inf)
        feats[:, 4] = col
    cents = rng.random((n_sv, 3))
    labels = rng.integers(-1, 4, n_sv).astype(np.int32)
    part = rng.integers(-1, n_sv + 1, (6, 7, 9)).astype(np.int32)
    part.flat[:3] = [0, n_sv - 1, n_sv // 2]
    want = R.discard_ref(part, feats, cents, labels)
    kept = int((feats[:, 4] >= feats[:, 4].min() + 0.01).sum())
    assert len(want[1]) == kept
    if pattern == "threshold" and n_sv > 2:
        assert 0 < kept < n_sv and want[0].flat[0] == 0 and want[0].flat[1] == -1
    got = gg.discard_empty_svs(part, feats, cents, labels)
    assert got[1].shape == (kept, n_feat) and got[0].dtype == np.int16
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)


# ---- G7 kNN --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("n", [1, 2, 9, 33, 65, 700])
def test_knn_on_a_tie_lattice_at_every_list_size(gg, n, k):
    pos = R.lattice_positions(n)
    want = R.knn_candidates_ref(pos, k)
    assert (want[n - 1] == -1).all()
    if 2 < n <= k:                                               # rows that run out part of the way through
        assert all(want[i, n - 2 - i] >= 0 and want[i, n - 1 - i] == -1 for i in range(n - 1))
    got = gg.knn_candidates(pos, k)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    picks = gg.knn_greedy(want, k)
    rows = np.repeat(np.arange(n, dtype=np.int64), k).reshape(n, k)
    er, ec = gg.knn_edges(pos, k)
    assert np.array_equal(er, rows[picks >= 0]) and np.array_equal(ec, picks[picks >= 0])


# ---- G8 face adjacency ---------------------------------------------------------------------------------

TOUCHING = [((9, 10, 11), 3, 1), ((9, 10, 11), 2, 31), ((9, 10, 11), 2, 32), ((9, 10, 11), 2, 33), ((12, 9, 14), 2, 100),
            ((20, 24, 22), 2, 2100), ((1, 9, 11), 2, 20), ((2, 2, 2), 1, 100)]


@pytest.mark.parametrize("shape,block,n", TOUCHING, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_touching_at_word_edges_thin_volumes_and_foreign_labels(gg, shape, block, n):
    part = R.blocky_partition(shape, block, n, seed=n)
    if shape == (2, 2, 2):
        part = np.array([[[0, 1], [99, -1]], [[100, 57], [57, 0]]], dtype=np.int16)    # n = 100 > 8 voxels
    else:
        assert (part == -1).any() and (part >= n).any() and ((part >= 0) & (part < n)).any()
    want = R.touching_ref(part, n)
    assert [p for p in want if p[0] == p[1]] == [(i, i) for i in range(n)]
    rows, cols = gg.touching_edges(part, n)
    assert list(zip(rows.tolist(), cols.tolist())) == want      # row-major: ascending columns inside each row
