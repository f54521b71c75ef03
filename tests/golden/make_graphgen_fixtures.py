"""Generate the graph-generation fixtures ref_graphgen_<case>.npz by IMPORTING the reference.

Needs a checkout of the reference (rsinghlab/GNN-Tumor-Seg); not part of the test suite:
    python tests/golden/make_graphgen_fixtures.py /path/to/GNN-Tumor-Seg
The reference's mri2graph.graphgen is imported with two environment shims, its files untouched:
  - a stub `skimage.segmentation` whose `slic` returns a given partition (the numpy restatement's
    SLIC + connectivity labels, tests/graphgen_ref.py), since skimage is not installed;
  - `nx.from_numpy_matrix = nx.from_numpy_array` (removed in networkx 3).
Volumes come from tests/graphgen_ref.make_volume (seeded), so only their digests are stored.
The contract orders equal distances by the lower index (a stable argsort).  numpy's default
argsort leaves that order unspecified, so every kNN adjacency here is computed with argsort forced
to kind='stable'; whether the default one gives the same matrix is recorded per fixture
(`default_argsort_agrees_*`): on volumes whose supervoxel centroids have exactly equal distances it
does not.
"""
import os
import sys
import types

import networkx as nx
import numpy as np
from scipy import ndimage

if len(sys.argv) != 2:
    raise SystemExit(f"usage: python {sys.argv[0]} /path/to/GNN-Tumor-Seg")
REF = os.path.abspath(sys.argv[1])
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
sys.path.insert(0, REF)

from tests import graphgen_ref as R  # noqa: E402

_PARTITION = {}
_stub = types.ModuleType("skimage.segmentation")
_stub.slic = lambda image, **kw: _PARTITION["labels"].copy()
sys.modules.setdefault("skimage", types.ModuleType("skimage"))
sys.modules["skimage.segmentation"] = _stub
nx.from_numpy_matrix = nx.from_numpy_array

from mri2graph import graphgen as ref_gg  # noqa: E402


class _StableNumpy(types.ModuleType):
    """numpy with argsort forced to kind='stable' (to show tie order does not matter)."""

    def __getattr__(self, name):
        if name == "argsort":
            return lambda a, axis=-1: np.argsort(a, axis=axis, kind="stable")
        return getattr(np, name)


def adjacency_pairs(adj):
    r, c = np.nonzero(np.triu(adj, 1))
    return np.stack([r, c], axis=1).astype(np.int32)


def stable(fn, *args):
    saved = ref_gg.np
    ref_gg.np = _StableNumpy("numpy_stable")
    try:
        return fn(*args)
    finally:
        ref_gg.np = saved


def adjacency_both_ways(centroids, feats, k):
    """(adjacency with the stable argsort, whether the default argsort gives the same)."""
    a = ref_gg.build_adjacency_matrix(centroids, feats, k, weighted=False, enforce_regularity=True)
    b = stable(ref_gg.build_adjacency_matrix, centroids, feats, k, False, True)
    return b, bool(np.array_equal(a, b))


def graph_arrays(prefix, graph, feats, part, with_labels):
    out = {}
    edges = np.array(sorted((min(u, v), max(u, v)) for u, v in graph.edges), dtype=np.int32).reshape(-1, 2)
    out[prefix + "edges"] = edges
    out[prefix + "n_nodes"] = np.int32(graph.number_of_nodes())
    out[prefix + "feats"] = np.array([graph.nodes[n]["features"] for n in graph.nodes], dtype=np.float64)
    if with_labels:
        out[prefix + "labels"] = np.array([graph.nodes[n]["label"] for n in graph.nodes], dtype=np.int32)
    out[prefix + "sv_feats"] = np.asarray(feats)
    out[prefix + "partition"] = np.asarray(part)
    return out


def main():
    for case in R.CASES:
        img, labels = R.make_volume(case)
        smoothed = ndimage.gaussian_filter(img.astype(np.float64), [1, 1, 1, 0] if img.ndim == 4 else 1)
        sm4 = smoothed if smoothed.ndim == 4 else smoothed[..., None]
        scaled = sm4 * (1.0 / case.compactness)
        emptied = []
        slic_lab = R.slic_rounds_ref(scaled, case.n_segments, 10, emptied)
        lo, hi = R.connectivity_sizes(case.shape, case.n_segments)
        conn = R.connectivity_ref(slic_lab, lo, hi)
        n_sv = int(conn.max()) + 1
        _PARTITION["labels"] = conn
        part16 = conn.astype(np.int16)

        feats, cents, svl = ref_gg.extract_supervoxel_statistics(part16.copy(), img, labels, n_sv)
        new_part, nfeats, ncents, nlabels = ref_gg.discard_empty_svs(part16.copy(), feats, cents, svl, n_sv)
        k_big = 25
        adj10, agree10 = adjacency_both_ways(ncents, nfeats, 10)
        adj25, agree25 = adjacency_both_ways(ncents, nfeats, k_big)
        touch = ref_gg.find_adjacent_nodes(new_part.copy(), len(nlabels), as_mat=True)
        data = {
            "image_digest": np.array(R.digest(img)), "labels_digest": np.array(R.digest(labels)),
            "smoothed_digest": np.array(R.digest(smoothed)), "smoothed_probe": sm4[case.shape[0] // 2, ::4, ::4],
            "slic_labels": slic_lab.astype(np.int16), "conn_labels": conn.astype(np.int16),
            "n_sv": np.int32(n_sv), "min_size": np.int64(lo), "max_size": np.int64(hi),
            "sv_feats": np.asarray(feats, dtype=np.float64), "sv_centroids": cents, "sv_labels": svl.astype(np.int32),
            "partition": new_part, "node_feats": nfeats, "node_centroids": ncents,
            "node_labels": nlabels.astype(np.int32), "knn10": adjacency_pairs(adj10),
            "k_big": np.int32(k_big), "knn_big": adjacency_pairs(adj25), "touching": np.stack(np.nonzero(touch), 1).astype(np.int32),
            "emptied_per_update": np.array(emptied, dtype=np.int32),
            "default_argsort_agrees_knn10": np.bool_(agree10), "default_argsort_agrees_knn_big": np.bool_(agree25),
        }
        g, f, p = stable(ref_gg.img2graph, img, labels, case.n_segments, case.compactness, 10)
        data.update(graph_arrays("g10_", g, f, p, True))
        g, f, p = ref_gg.img2graph(img, labels, case.n_segments, case.compactness, 0)
        data.update(graph_arrays("g0_", g, f, p, True))
        g, f, p = stable(ref_gg.img2graph, img, None, case.n_segments, case.compactness, 10)
        data.update(graph_arrays("gnl_", g, f, p, False))
        path = os.path.join(OUT, f"ref_graphgen_{case.name}.npz")
        np.savez_compressed(path, **data)
        print(f"{path}: n_sv {n_sv}, nodes {len(nlabels)}, default argsort agrees {agree10}/{agree25}, emptied {emptied[-1]}, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
