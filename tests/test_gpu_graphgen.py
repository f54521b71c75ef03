"""Graph generation on the MI355X (G1-G8 of csrc/gts_graphgen.hip) against the numpy restatement of
SLIC (tests/graphgen_ref.py) and the reference-generated fixtures (tests/golden/ref_graphgen_*.npz)."""
import os

import numpy as np
import pytest
import torch

from tests import graphgen_ref as R

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in R.CASES}


@pytest.fixture(scope="module")
def gg(hip_lib):
    from gts import graphgen

    return graphgen


def _fixture(golden_dir, name):
    f = dict(np.load(os.path.join(golden_dir, f"ref_graphgen_{name}.npz")))
    img, labels = R.make_volume(CASES[name])
    assert R.digest(img) == str(f["image_digest"]) and R.digest(labels) == str(f["labels_digest"])
    return f, img, labels


def _pairs(rows, cols):
    return sorted(zip(np.asarray(rows).tolist(), np.asarray(cols).tolist()))


@pytest.mark.parametrize("name", list(CASES))
def test_gaussian_is_bit_exact_against_scipy(gg, golden_dir, name):
    f, img, _ = _fixture(golden_dir, name)
    sm = gg.gaussian(img.astype(np.float64), 1.0)
    assert sm.shape == img.shape and sm.dtype == np.float64
    sm4 = sm if sm.ndim == 4 else sm[..., None]
    assert np.array_equal(sm4[CASES[name].shape[0] // 2, ::4, ::4], f["smoothed_probe"])
    assert R.digest(sm) == str(f["smoothed_digest"])


@pytest.mark.parametrize("name", list(CASES))
def test_slic_labels_are_bit_exact_against_the_restatement(gg, golden_dir, name):
    f, img, _ = _fixture(golden_dir, name)
    case = CASES[name]
    scaled = gg.gaussian(img.astype(np.float64), 1.0, 1.0 / case.compactness)
    labels, _ = gg.slic_rounds(scaled, case.n_segments, 10)
    assert np.array_equal(labels.cpu().numpy(), f["slic_labels"])
    whole = gg.slic(img, n_segments=case.n_segments, compactness=case.compactness, sigma=1.0)
    assert np.array_equal(whole, f["conn_labels"])


def test_emptied_segments_never_capture_again(gg, golden_dir):
    """The 'empty' fixture loses segments in the restatement (0/0 centres, skimage's divide); the
    GPU rounds skip those centres from then on and give the same labels."""
    f, img, _ = _fixture(golden_dir, "empty")
    case = CASES["empty"]
    assert f["emptied_per_update"][-1] > 0
    scaled = gg.gaussian(img.astype(np.float64), 1.0, 1.0 / case.compactness)
    labels, n_centres = gg.slic_rounds(scaled, case.n_segments, 10)
    got = labels.cpu().numpy()
    assert np.array_equal(got, f["slic_labels"])
    assert len(np.unique(got)) <= n_centres - f["emptied_per_update"][-1]


def test_float64_intensities_reach_slic_unrounded(gg, golden_dir):
    """build_graph smooths voxel_intensities.astype(float64), not a float32 copy of it."""
    from scipy import ndimage

    case = CASES["c4"]
    img, labels = R.make_volume(case)
    img64 = img.astype(np.float64) + 1e-9 * np.random.default_rng(3).standard_normal(img.shape)
    res = gg.build_graph(img64, labels, case.n_segments, case.compactness, 10)
    scaled = ndimage.gaussian_filter(img64, [1, 1, 1, 0]) * (1.0 / case.compactness)
    lo, hi = R.connectivity_sizes(case.shape, case.n_segments)
    want = R.connectivity_ref(R.slic_rounds_ref(scaled, case.n_segments, 10), lo, hi)
    assert np.array_equal(res["slic"], want)


def test_mid_size_volume_against_the_restatement_run_live(gg):
    case = R.Case("mid", (96, 112, 80), 4, 1500, 0.5, 31, None)
    img, _ = R.make_volume(case)
    scaled = gg.gaussian(img.astype(np.float64), 1.0, 2.0)
    got, _ = gg.slic_rounds(scaled, case.n_segments, 10)
    want = R.slic_rounds_ref(scaled, case.n_segments, 10)
    assert np.array_equal(got.cpu().numpy(), want)
    lo, hi = R.connectivity_sizes(case.shape, case.n_segments)
    conn, n = gg.enforce_connectivity(got.cpu().numpy(), lo, hi)
    assert np.array_equal(conn, R.connectivity_ref(want, lo, hi)) and n == conn.max() + 1


@pytest.mark.parametrize("name", list(CASES))
def test_statistics_discard_and_edges_match_the_reference(gg, golden_dir, name):
    f, img, labels = _fixture(golden_dir, name)
    n_sv = int(f["n_sv"])
    feats, cents, svl = gg.supervoxel_statistics(f["conn_labels"], img, labels, n_sv)
    assert np.array_equal(feats, f["sv_feats"])
    assert np.array_equal(cents, f["sv_centroids"])
    assert np.array_equal(svl, f["sv_labels"])
    part, nf, nc, nl = gg.discard_empty_svs(f["conn_labels"], feats, cents, svl)
    assert part.dtype == np.int16 and np.array_equal(part, f["partition"])
    assert np.array_equal(nf, f["node_feats"]) and np.array_equal(nc, f["node_centroids"])
    assert np.array_equal(nl, f["node_labels"])
    assert _pairs(*gg.knn_edges(nc, 10)) == _pairs(*f["knn10"].T)
    assert _pairs(*gg.knn_edges(nc, int(f["k_big"]))) == _pairs(*f["knn_big"].T)
    assert _pairs(*gg.touching_edges(part, len(nl))) == _pairs(*f["touching"].T)


@pytest.mark.parametrize("name", list(CASES))
def test_img2graph_matches_the_reference(gg, golden_dir, name):
    from mri2graph.graphgen import img2graph

    f, img, labels = _fixture(golden_dir, name)
    case = CASES[name]
    for prefix, lab, k in (("g10_", labels, 10), ("g0_", labels, 0), ("gnl_", None, 10)):
        graph, feats, part = img2graph(img, lab, case.n_segments, case.compactness, k)
        assert graph.number_of_nodes() == int(f[prefix + "n_nodes"]) and list(graph.nodes) == list(range(len(feats)))
        edges = sorted((min(u, v), max(u, v)) for u, v in graph.edges)
        assert edges == sorted(map(tuple, f[prefix + "edges"].tolist()))
        assert feats.dtype == np.float64 and np.array_equal(feats, f[prefix + "sv_feats"])
        assert part.dtype == np.int16 and np.array_equal(part, f[prefix + "partition"])
        assert np.array_equal(np.array([graph.nodes[n]["features"] for n in graph.nodes]), f[prefix + "feats"])
        if lab is not None:
            assert [graph.nodes[n]["label"] for n in graph.nodes] == f[prefix + "labels"].tolist()
        else:
            assert all("label" not in graph.nodes[n] for n in graph.nodes)
        if k == 0:
            assert all(graph.has_edge(n, n) for n in graph.nodes)


def test_a_segment_above_the_lds_sort_cap(gg):
    """Segment 0 holds ~35 k voxels (the LDS path sorts at most 4096): the global-memory sort
    gives numpy's quantiles and the mode all the same."""
    rng = np.random.default_rng(5)
    shape = (40, 48, 36)
    part = rng.integers(1, 60, size=shape).astype(np.int32)
    part[:, :, :20] = 0
    part[5, 5, 5] = 60
    img = rng.standard_normal(shape + (3,)).astype(np.float32)
    lab = rng.integers(0, 4, size=shape).astype(np.int16)
    feats, cents, svl = gg.supervoxel_statistics(part, img, lab, 61)
    zz, yy, xx = np.indices(shape)
    for k in (0, 1, 60):
        m = part == k
        want = np.concatenate([np.quantile(img[..., c][m], [0.1, 0.25, 0.5, 0.75, 0.9]) for c in range(3)])
        assert np.array_equal(feats[k], want)
        vals, counts = np.unique(lab[m], return_counts=True)
        assert svl[k] == vals[counts.argmax()]
        assert np.array_equal(cents[k], [zz[m].sum() / m.sum(), yy[m].sum() / m.sum(), xx[m].sum() / m.sum()])


def _brats_graph(gg, seed, n=15000, k=10):
    from data_processing.image_processing import determine_brain_crop, normalize_img, standardize_img
    from gts import synth_mri
    from scripts.preprocess_dataset import STANDARDIZATION_STATS, swap_labels_from_brats

    img, lab = synth_mri.make_sample(seed)
    crop = determine_brain_crop(img)
    data = standardize_img(normalize_img(img[crop]), np.float32(STANDARDIZATION_STATS[0]),
                           np.float32(STANDARDIZATION_STATS[1]))
    return data, gg.build_graph(data, swap_labels_from_brats(lab[crop]), n, 0.5, k)


def test_brats_size_sample_invariants_and_determinism(gg):
    from gts import from_networkx
    from mri2graph.graphgen import _graph

    data, a = _brats_graph(gg, 7)
    slic = a["slic"]
    assert slic.min() == 0 and np.array_equal(np.unique(slic), np.arange(a["n_sv"]))    # every voxel, contiguous
    part = a["partition"]
    n = a["feats"].shape[0]
    assert a["feats"].shape == (n, 20) and 0 < n < a["n_sv"]
    _, first = np.unique(slic, return_index=True)
    remap = part.ravel()[first].astype(np.int64)                                        # each supervoxel's new id
    assert np.array_equal(part, remap[slic])                                            # -1 exactly on dropped ones
    assert np.array_equal(remap[remap >= 0], np.arange(n))                              # kept ones numbered in order
    rows, cols = a["edges"]
    assert (rows < cols).all()
    deg = np.bincount(np.concatenate([rows, cols]), minlength=n)
    assert (deg[: n - 20] >= 10).all()
    g = from_networkx(_graph(n, rows, cols, 1.0))
    assert g.number_of_nodes() == n and g.number_of_edges() == 2 * len(rows)
    _, b = _brats_graph(gg, 7)
    for key in ("slic", "partition", "feats", "centroids", "labels"):
        assert np.array_equal(a[key], b[key]), key
    assert all(np.array_equal(x, y) for x, y in zip(a["edges"], b["edges"]))
