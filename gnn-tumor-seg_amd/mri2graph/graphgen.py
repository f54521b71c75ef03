"""The reference's mri2graph/graphgen.py module surface over the HIP kernels of gts.graphgen.

Same names, argument orders and result types as the reference (mri2graph/graphgen.py): SLIC
(skimage <= 0.18 semantics, restated in DESIGN.md), supervoxel statistics, empty-supervoxel
discard and the two edge builders.  networkx graphs are built from edge lists, without
`from_numpy_matrix` (removed in networkx 3) and without any N x N matrix.
"""
import networkx as nx
import numpy as np

from gts import graphgen as gg


def determine_nodes_and_features(supervoxel_partitioning, voxel_intensities, voxel_labels, num_supervoxels):
    """(new_region_img int16, node_feats, node_centroids, node_labels) — reference graphgen.py:34-38."""
    sv_feats, sv_centroids, sv_labels = extract_supervoxel_statistics(supervoxel_partitioning, voxel_intensities,
                                                                      voxel_labels, num_supervoxels)
    return discard_empty_svs(supervoxel_partitioning, sv_feats, sv_centroids, sv_labels, num_supervoxels)


def extract_supervoxel_statistics(sv_partitioning, voxel_intensities, voxel_labels, num_supervoxels):
    """(sv_feats [n, 5C] float64, sv_centroids [n, 3] float64, sv_labels [n] int32) — graphgen.py:47-61."""
    labels = np.zeros(np.shape(sv_partitioning), dtype=np.int16) if voxel_labels is None else voxel_labels
    return gg.supervoxel_statistics(np.asarray(sv_partitioning), np.asarray(voxel_intensities, dtype=np.float32),
                                    np.asarray(labels), int(num_supervoxels))


def discard_empty_svs(sv_partitioning, sv_features, sv_centroids, sv_labels, n_svs):
    """graphgen.py:71-96: drop supervoxels whose 0.9-quantile of channel 0 is within 0.01 of the minimum."""
    if len(sv_features) != n_svs:
        raise ValueError("n_svs does not match the feature rows")
    return gg.discard_empty_svs(np.asarray(sv_partitioning), np.asarray(sv_features), np.asarray(sv_centroids),
                                np.asarray(sv_labels))


def build_adjacency_matrix(positions, intensities, k, weighted=True, enforce_regularity=True):
    """graphgen.py:120-153 for weighted=False, enforce_regularity=True (what img2graph asks for),
    as a dense float64 0/1 matrix for callers that want the matrix."""
    if weighted or not enforce_regularity:
        raise NotImplementedError("only weighted=False, enforce_regularity=True is supported")
    n = len(positions)
    rows, cols = gg.knn_edges(np.asarray(positions, dtype=np.float64), int(k))
    adj = np.zeros((n, n))
    adj[rows, cols] = 1
    adj[cols, rows] = 1
    return adj


def find_adjacent_nodes(regionImg, n_nodes, as_mat=False):
    """graphgen.py:161-196 (3-D): face-adjacent node pairs in both orientations plus self-loops."""
    rows, cols = gg.touching_edges(np.asarray(regionImg), int(n_nodes))
    if as_mat:
        adj = np.zeros((n_nodes, n_nodes), dtype=bool)
        adj[rows, cols] = True
        return adj
    return rows, cols


def _graph(n, rows, cols, weight):
    """networkx.from_numpy_array of the symmetric matrix with ones at (rows, cols): nodes 0..n-1,
    edges inserted in the row-major order of the matrix's nonzeros."""
    pairs = gg.symmetric_pairs(rows, cols)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from((int(u), int(v), {"weight": weight}) for u, v in pairs)
    return g


def img2graph(voxel_intensities, voxel_labels, approx_num_nodes=5000, boxiness=0.5, k=10):
    """(nx_graph, sv_feats [N, 5C] float64, updated_partitioning int16) — graphgen.py:236-271."""
    labels_provided = voxel_labels is not None
    res = gg.build_graph(voxel_intensities, voxel_labels, approx_num_nodes, boxiness, k or 0)
    feats, node_labels = res["feats"], res["labels"]
    n = feats.shape[0]
    rows, cols = res["edges"]
    graph = _graph(n, rows, cols, 1.0 if k else True)
    for node in graph.nodes:
        if labels_provided:
            graph.nodes[node]["label"] = int(node_labels[node])
        graph.nodes[node]["features"] = list(feats[node])
    return graph, feats, res["partition"]
