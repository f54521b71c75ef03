"""The stage references of tests/graphgen_ref.py, without a GPU (the kNN check needs the built
library for its host C greedy pass, as tests/test_graphgen_host.py does): each reproduces what
the reference-made fixtures already pin, and each edge input of tests/test_gpu_graphgen_edges.py
is shown, on the reference alone, to tell the contract from its nearest wrong neighbour, so that
the GPU equality tests cannot pass vacuously."""
import os

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial.distance import cdist

from tests import graphgen_ref as R

CASES = {c.name: c for c in R.CASES}


@pytest.fixture(scope="module", params=list(CASES))
def fixture(request, golden_dir):
    f = dict(np.load(os.path.join(golden_dir, f"ref_graphgen_{request.param}.npz")))
    img, labels = R.make_volume(CASES[request.param])
    assert R.digest(img) == str(f["image_digest"]) and R.digest(labels) == str(f["labels_digest"])
    return CASES[request.param], f, img, labels


def test_slic_rounds_from_assign_and_update_reproduce_the_fixture(fixture):
    case, f, img, _ = fixture
    smoothed = ndimage.gaussian_filter(img.astype(np.float64), [1, 1, 1, 0] if img.ndim == 4 else 1)
    emptied = []
    got = R.slic_rounds_ref(smoothed * (1.0 / case.compactness), case.n_segments, 10, emptied)
    assert np.array_equal(got, f["slic_labels"])
    assert np.array_equal(emptied, f["emptied_per_update"])


def test_stats_ref_reproduces_the_fixture(fixture):
    _, f, img, labels = fixture
    n_sv = int(f["n_sv"])
    for ref in (R.stats_ref, R.stats_ref_grouped):
        feats, cents, svl = ref(f["conn_labels"], img, labels, n_sv)
        assert np.array_equal(feats, f["sv_feats"]) and feats.dtype == np.float64
        assert np.array_equal(cents, f["sv_centroids"])
        assert np.array_equal(svl, f["sv_labels"]) and svl.dtype == np.int32


def test_discard_ref_reproduces_the_fixture(fixture):
    _, f, _, _ = fixture
    part, nf, nc, nl = R.discard_ref(f["conn_labels"], f["sv_feats"], f["sv_centroids"], f["sv_labels"])
    assert part.dtype == np.int16 and np.array_equal(part, f["partition"])
    assert np.array_equal(nf, f["node_feats"]) and np.array_equal(nc, f["node_centroids"])
    assert np.array_equal(nl, f["node_labels"])


def test_knn_candidates_ref_through_the_greedy_pass_reproduces_the_fixture(fixture, hip_lib):
    from gts import graphgen as gg

    _, f, _, _ = fixture
    pos = f["node_centroids"]
    for k, key in ((10, "knn10"), (int(f["k_big"]), "knn_big")):
        picks = gg.knn_greedy(R.knn_candidates_ref(pos, k), k)
        rows = np.repeat(np.arange(len(pos)), k).reshape(picks.shape)
        got = sorted(zip(rows[picks >= 0].tolist(), picks[picks >= 0].tolist()))
        assert got == sorted(map(tuple, f[key].tolist()))


def test_touching_ref_reproduces_the_fixture(fixture):
    _, f, _, _ = fixture
    assert R.touching_ref(f["partition"], len(f["node_labels"])) == sorted(map(tuple, f["touching"].tolist()))


# ---- the edge inputs, on the references alone ------------------------------------------------------

def test_stats_edge_case_has_the_stated_sizes_and_both_references_agree():
    part, img, lab, n_sv = R.stats_edge_case()
    sizes = np.bincount(part[(part >= 0) & (part < n_sv)], minlength=n_sv)
    assert sorted(sizes[sizes > 0]) == list(R.STATS_SIZES)
    assert sizes[R.STATS_ABSENT] == 0 and sizes[n_sv - 1] == 0 and (part == -1).any() and (part == n_sv).any()
    a = R.stats_ref(part, img, lab, n_sv)
    b = R.stats_ref_grouped(part, img, lab, n_sv)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    feats, cents, svl = a
    for k in (R.STATS_ABSENT, n_sv - 1):
        assert (feats[k] == -1.0).all() and np.isnan(cents[k]).all() and svl[k] == -1
    assert (svl < -1).any()                                      # a negative voxel label wins somewhere
    by_size = {int(sizes[k]): k for k in range(n_sv) if sizes[k]}
    assert svl[by_size[2]] == -3 and svl[by_size[256]] == -1     # exact ties: the smaller label
    none = R.stats_ref(part, img, None, n_sv)[2]
    assert np.array_equal(none, np.where(sizes > 0, 0, -1))


def test_float64_subtraction_would_differ_from_numpy_on_the_edge_case():
    """numpy's _lerp subtracts in the data's float32; a float64 hi - lo gives another quantile."""
    part, img, _, n_sv = R.stats_edge_case()
    differs = 0
    for k in range(n_sv):
        v = img[..., 1][part == k]
        if len(v) == 0:
            continue
        want = np.quantile(v, R.QUANTILES)
        differs += int(not np.array_equal(want, R.quantile_float64_diff(v, R.QUANTILES)))
        # the variant is the same rule otherwise: on data whose differences are exact it agrees
        dup = img[..., 0][part == k]
        assert np.array_equal(np.quantile(dup, R.QUANTILES), R.quantile_float64_diff(dup, R.QUANTILES))
    assert differs >= 1


@pytest.mark.parametrize("n", [9, 33, 65, 700])
def test_an_unstable_order_would_differ_on_the_tie_lattice(n):
    pos = R.lattice_positions(n)
    assert len(np.unique(pos, axis=0)) == n
    dist = cdist(pos, pos)
    stable = R.knn_candidates_ref(pos, 8)
    # highest j first among equal distances: the stable order of the reversed columns, mapped back
    rev = n - 1 - np.argsort(dist[:, ::-1], axis=1, kind="stable")
    assert np.array_equal(np.take_along_axis(dist, rev, 1), np.sort(dist, axis=1))
    assert not np.array_equal(stable, R.knn_candidates_ref(pos, 8, order=rev))


@pytest.mark.parametrize("name", list(R.WIDE_SLIC))
def test_wide_slic_cases_walk_several_runs_of_64(name):
    shape, n, c, compactness = R.WIDE_SLIC[name]
    vol = R.striped_volume(name)
    assert vol.shape == shape + (c,)
    scaled = ndimage.gaussian_filter(vol, [1, 1, 1, 0]) * (1.0 / compactness)
    emptied, at_update = [], []
    R.slic_rounds_ref(scaled, n, 10, emptied, at_update)
    assert emptied[-1] == 0
    last = at_update[-1]
    n_c = int(last.max()) + 1
    runs = []
    for k in range(n_c):
        xs = np.flatnonzero((last == k).any(axis=(0, 1)))
        assert xs[-1] - xs[0] + 1 > 64, (k, xs[0], xs[-1])
        runs.append(R.x_runs(last == k))
    assert max(runs) > 1
