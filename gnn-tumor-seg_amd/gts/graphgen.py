"""Supervoxel graph construction on the MI355X: the device-level API behind mri2graph.graphgen.

Stages (csrc/gts_graphgen.hip, include/gts_hip.h G1-G8): Gaussian smoothing (G1), SLIC
assignment (G2) and centre update (G3), connectivity enforcement on the host (G4), supervoxel
statistics (G5), discard + renumber (G6), k-nearest-neighbour edges (G7) and face-adjacency edges
(G8).  The SLIC restated here is skimage <= 0.18's (DESIGN.md "Graph generation").

Every function accepts numpy arrays or GPU tensors and returns numpy arrays for numpy input,
tensors on the input's device otherwise.  There is no CPU path: without a GPU the calls raise.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream
from ._operands import scratch

MAX_SV = _lib.const("GTS_GG_MAX_SV")   # the partition is int16, as in the reference
MAX_K = _lib.const("GTS_GG_MAX_K")
MAX_RADIUS = _lib.const("GTS_GG_MAX_RADIUS")
QUANTILES = (0.1, 0.25, 0.5, 0.75, 0.9)


def _device():
    if not torch.cuda.is_available():
        raise _lib.GtsError("graph generation runs on the MI355X HIP path only: no GPU visible")
    return torch.device("cuda", torch.cuda.current_device())


def _tensor(x, dtype, dev=None):
    if isinstance(x, torch.Tensor):
        t = x if x.is_cuda else x.to(dev or _device())
    else:
        t = torch.from_numpy(np.ascontiguousarray(x)).to(dev or _device())
    return t.to(dtype).contiguous()


def _out(t, as_numpy):
    return t.cpu().numpy() if as_numpy else t


def _volume(image):
    """[D,H,W] or [D,H,W,C] -> shape (D, H, W, C)."""
    shape = tuple(image.shape)
    if len(shape) == 3:
        return shape + (1,)
    if len(shape) == 4:
        return shape
    raise ValueError(f"expected a 3-D volume with an optional channel axis, got shape {shape}")


# ---- grid (host) -------------------------------------------------------------------------------

# regular_grid follows skimage.util.regular_grid (scikit-image, BSD-3-Clause licence,
# Copyright (C) 2019, the scikit-image team; redistribution with this notice is permitted).
def regular_grid(shape, n):
    """skimage.util.regular_grid: slices that place about n points evenly over `shape`."""
    ar_shape = np.asanyarray(shape)
    ndim = len(ar_shape)
    unsort_dim_idxs = np.argsort(np.argsort(ar_shape))
    sorted_dims = np.sort(ar_shape)
    space_size = float(np.prod(ar_shape))
    if space_size <= n:
        return (slice(None),) * ndim
    stepsizes = (space_size / n) ** (1.0 / ndim) * np.ones(ndim)
    if (sorted_dims < stepsizes).any():
        for dim in range(ndim):
            stepsizes[dim] = sorted_dims[dim]
            space_size = float(np.prod(sorted_dims[dim + 1:]))
            stepsizes[dim + 1:] = ((space_size / n) ** (1.0 / (ndim - dim - 1)))
            if (sorted_dims >= stepsizes).all():
                break
    starts = (stepsizes // 2).astype(int)
    stepsizes = np.round(stepsizes).astype(int)
    slices = [slice(start, None, step) for start, step in zip(starts, stepsizes)]
    return tuple(slices[i] for i in unsort_dim_idxs)


def _steps(slices):
    return [int(s.step if s.step is not None else 1) for s in slices]


def slic_grid(shape3, n_segments):
    """Initial SLIC centres (z, y, x) in raster order, the scale step and the window steps."""
    slices = regular_grid(shape3, n_segments)
    steps = _steps(slices)
    zz, yy, xx = np.mgrid[:shape3[0], :shape3[1], :shape3[2]]
    coords = np.stack([zz[slices].ravel(), yy[slices].ravel(), xx[slices].ravel()], axis=1).astype(np.float64)
    step = float(max(steps))
    window = _steps(regular_grid(shape3, coords.shape[0]))
    return coords, step, window


def gaussian_weights(sigma):
    """Taps w[0..radius] of scipy.ndimage's Gaussian (truncate 4.0), centre first."""
    radius = int(4.0 * float(sigma) + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    return phi_x[radius:].copy()


# ---- G1 -----------------------------------------------------------------------------------------

def gaussian(image, sigma=1.0, scale=1.0):
    """G1: scipy.ndimage.gaussian_filter(image, [sigma] * 3 + [0]) * scale in fp64 ('reflect');
    sigma = 0 only scales."""
    as_numpy = not isinstance(image, torch.Tensor)
    d, h, w, c = _volume(image)
    img = _tensor(image, torch.float64)
    weights = gaussian_weights(sigma) if sigma > 0 else np.ones(1)
    if len(weights) - 1 > MAX_RADIUS:
        raise ValueError(f"sigma {sigma} needs a radius above {MAX_RADIUS}")
    wt = torch.from_numpy(weights).to(img.device)
    out = torch.empty_like(img)
    tmp = torch.empty_like(img)
    check(_lib.load().gts_gg_gaussian_f64(img.data_ptr(), out.data_ptr(), tmp.data_ptr(), wt.data_ptr(),
                                          len(weights) - 1, float(scale), d, h, w, c, current_stream()),
          "gts_gg_gaussian_f64")
    return _out(out.reshape(image.shape), as_numpy)


# ---- G2 / G3 --------------------------------------------------------------------------------------

def slic_rounds(scaled, n_segments, max_iter=10, on_round=None):
    """SLIC rounds over an already smoothed and scaled [D,H,W(,C)] fp64 volume: the initial grid
    (colour 0), then max_iter assignments with a centre update between consecutive ones.
    Returns the int32 label volume (before connectivity enforcement) on the device, and the
    number of centres.  on_round(i, stage) is called after each stage (timing hooks)."""
    d, h, w, c = _volume(scaled)
    if c > 8:
        raise ValueError("SLIC supports at most 8 channels")
    img = _tensor(scaled, torch.float64)
    dev = img.device
    coords, step, window = slic_grid((d, h, w), n_segments)
    k = coords.shape[0]
    centres = torch.zeros((k, 3 + c), dtype=torch.float64, device=dev)
    centres[:, :3] = torch.from_numpy(coords).to(dev)
    labels = torch.full((d, h, w), -1, dtype=torch.int32, device=dev)
    best = torch.empty(d * h * w, dtype=torch.int64, device=dev)
    winner = torch.empty(d * h * w, dtype=torch.int32, device=dev)
    bbox = torch.empty(k * 6, dtype=torch.int32, device=dev)
    lib = _lib.load()
    sw = 1.0 / (step ** 2)
    for i in range(max_iter):
        if i > 0:
            check(lib.gts_gg_slic_update_f64(img.data_ptr(), labels.data_ptr(), centres.data_ptr(), k, d, h, w, c,
                                             bbox.data_ptr(), current_stream()), "gts_gg_slic_update_f64")
            if on_round:
                on_round(i, "update")
        check(lib.gts_gg_slic_assign_f64(img.data_ptr(), centres.data_ptr(), k, d, h, w, c, *window, sw,
                                         labels.data_ptr(), best.data_ptr(), winner.data_ptr(), current_stream()),
              "gts_gg_slic_assign_f64")
        if on_round:
            on_round(i, "assign")
        if i == 0 and int(labels.min()) < 0:
            raise _lib.GtsError("SLIC: a voxel lies in no centre's window after the first round")
    return labels, k


# ---- G4 -----------------------------------------------------------------------------------------

def connectivity_sizes(shape3, n_segments):
    """(min_size, max_size) of skimage's connectivity pass for the requested n_segments."""
    segment_size = float(np.prod(shape3)) / n_segments
    return int(0.5 * segment_size), int(3 * segment_size)


def _enforce_connectivity(labels, min_size, max_size):
    """G4 (host C): skimage's _enforce_label_connectivity_cython.  Returns (int32 labels, count)."""
    lab = np.ascontiguousarray(np.asarray(labels), dtype=np.int32)
    if lab.ndim != 3:
        raise ValueError("connectivity enforcement needs a 3-D label volume")
    out = np.empty_like(lab)
    queue = np.empty(max(int(max_size), 1), dtype=np.int64)
    n = ctypes.c_int32()
    check(_lib.load().gts_gg_enforce_connectivity(lab.ctypes.data, out.ctypes.data, *lab.shape, int(min_size),
                                                  int(max_size), queue.ctypes.data, ctypes.byref(n)),
          "gts_gg_enforce_connectivity")
    return out, n.value


enforce_connectivity = _enforce_connectivity


def slic(image, n_segments=100, compactness=10.0, sigma=1.0, max_iter=10, enforce_connectivity=True):
    """skimage <= 0.18 slic(image, n_segments, compactness, max_iter, sigma, multichannel=image.ndim == 4,
    convert2lab=False, enforce_connectivity, start_label=0) on the GPU: int32 labels from 0."""
    as_numpy = not isinstance(image, torch.Tensor)
    d, h, w, c = _volume(image)
    if not 0 < n_segments <= MAX_SV:
        raise ValueError(f"n_segments must be in [1, {MAX_SV}]")
    img = _tensor(image, torch.float64).reshape(d, h, w, c)
    scaled = gaussian(img, sigma, 1.0 / compactness)
    labels, _ = slic_rounds(scaled, n_segments, max_iter)
    if enforce_connectivity:
        lo, hi = connectivity_sizes((d, h, w), n_segments)
        host, _ = _enforce_connectivity(labels.cpu().numpy(), lo, hi)
        return host if as_numpy else torch.from_numpy(host).to(img.device)
    return _out(labels, as_numpy)


# ---- G5 / G6 --------------------------------------------------------------------------------------

def supervoxel_statistics(partition, intensities, voxel_labels, n_sv):
    """G5: (feats [n_sv, 5C] fp64, centroids [n_sv, 3] fp64, labels [n_sv] int32) —
    extract_supervoxel_statistics of the reference.  Intensities are taken as float32."""
    as_numpy = not isinstance(partition, torch.Tensor)
    if not 0 < n_sv <= MAX_SV:
        raise ValueError(f"{n_sv} supervoxels: the partition holds at most {MAX_SV}")
    d, h, w, c = _volume(intensities)
    part = _tensor(partition, torch.int32)
    dev = part.device
    img = _tensor(intensities, torch.float32, dev)
    lab = None if voxel_labels is None else _tensor(voxel_labels, torch.int16, dev)
    lib = _lib.load()
    feats = torch.empty((n_sv, 5 * c), dtype=torch.float64, device=dev)
    cents = torch.empty((n_sv, 3), dtype=torch.float64, device=dev)
    svl = torch.empty(n_sv, dtype=torch.int32, device=dev)
    ws = scratch(lib.gts_gg_sv_stats_workspace(d * h * w, n_sv), dev, torch.uint8)
    check(lib.gts_gg_sv_stats(part.data_ptr(), img.data_ptr(), None if lab is None else lab.data_ptr(), d, h, w, c,
                              n_sv, feats.data_ptr(), cents.data_ptr(), svl.data_ptr(), ws.data_ptr(),
                              current_stream()), "gts_gg_sv_stats")
    return _out(feats, as_numpy), _out(cents, as_numpy), _out(svl, as_numpy)


def discard_empty_svs(partition, feats, centroids, sv_labels):
    """G6: (int16 partition with -1 for dropped, node feats, node centroids, node labels)."""
    as_numpy = not isinstance(partition, torch.Tensor)
    part = _tensor(partition, torch.int32)
    dev = part.device
    f = _tensor(feats, torch.float64, dev)
    cen = _tensor(centroids, torch.float64, dev)
    svl = _tensor(sv_labels, torch.int32, dev)
    n_sv, n_feat = f.shape
    if not 0 < n_sv <= MAX_SV:
        raise ValueError(f"{n_sv} supervoxels: the partition holds at most {MAX_SV}")
    remap = torch.empty(n_sv, dtype=torch.int32, device=dev)
    keep = torch.empty(n_sv, dtype=torch.int32, device=dev)
    nf = torch.empty_like(f)
    nc = torch.empty_like(cen)
    nl = torch.empty_like(svl)
    new_part = torch.empty(part.shape, dtype=torch.int16, device=dev)
    n_nodes = torch.zeros(1, dtype=torch.int32, device=dev)
    check(_lib.load().gts_gg_discard_f64(f.data_ptr(), cen.data_ptr(), svl.data_ptr(), n_sv, n_feat, part.data_ptr(),
                                         part.numel(), remap.data_ptr(), keep.data_ptr(), nf.data_ptr(), nc.data_ptr(),
                                         nl.data_ptr(), new_part.data_ptr(), n_nodes.data_ptr(), current_stream()),
          "gts_gg_discard_f64")
    n = int(n_nodes.item())
    return _out(new_part, as_numpy), _out(nf[:n], as_numpy), _out(nc[:n], as_numpy), _out(nl[:n], as_numpy)


# ---- G7 / G8 --------------------------------------------------------------------------------------

def knn_candidates(positions, k):
    """G7 device part: cand[i, t] = the t-th nearest j > i (distance, then j), -1 when exhausted."""
    as_numpy = not isinstance(positions, torch.Tensor)
    n = positions.shape[0]
    if not 0 < n <= MAX_SV or not 0 < k <= MAX_K:
        raise ValueError(f"kNN needs 0 < n <= {MAX_SV} and 0 < k <= {MAX_K}")
    pos = _tensor(positions, torch.float64)
    cand = torch.empty((n, k), dtype=torch.int32, device=pos.device)
    check(_lib.load().gts_gg_knn_candidates_f64(pos.data_ptr(), n, k, cand.data_ptr(), current_stream()),
          "gts_gg_knn_candidates_f64")
    return _out(cand, as_numpy)


def knn_greedy(cand, k):
    """G7 host part: the reference's regularity loop over candidate lists.  Returns picks [n, k]
    (j or -1) as numpy int32."""
    c = np.ascontiguousarray(np.asarray(cand), dtype=np.int32)
    n = c.shape[0]
    picks = np.empty_like(c)
    got = np.empty(n, dtype=np.int32)
    n_edges = ctypes.c_int64()
    check(_lib.load().gts_gg_knn_greedy(c.ctypes.data, n, int(k), picks.ctypes.data, got.ctypes.data,
                                        ctypes.byref(n_edges)),
          "gts_gg_knn_greedy")
    return picks


def knn_edges(positions, k):
    """build_adjacency_matrix(positions, _, k, weighted=False, enforce_regularity=True) as an edge
    list: numpy int64 (rows, cols) with rows < cols, in the order the rows pick them."""
    cand = knn_candidates(positions, k)
    picks = knn_greedy(cand.cpu().numpy() if isinstance(cand, torch.Tensor) else cand, k)
    rows = np.repeat(np.arange(picks.shape[0], dtype=np.int64), k).reshape(picks.shape)
    m = picks >= 0
    return rows[m], picks[m].astype(np.int64)


def touching_edges(partition, n_nodes):
    """G8: find_adjacent_nodes(partition, n_nodes) = np.where(adjacency) with self-loops: numpy
    int64 (rows, cols) in row-major order.  -1 is never a node."""
    if not 0 < n_nodes <= MAX_SV:
        raise ValueError(f"{n_nodes} nodes: at most {MAX_SV}")
    part = _tensor(partition, torch.int16)
    if part.dim() != 3:
        raise ValueError("face adjacency needs a 3-D partition")
    dev = part.device
    lib = _lib.load()
    ws = scratch(lib.gts_gg_touching_workspace(n_nodes), dev, torch.uint8)
    indptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    check(lib.gts_gg_touching_count_i16(part.data_ptr(), *part.shape, n_nodes, ws.data_ptr(), indptr.data_ptr(),
                                        current_stream()), "gts_gg_touching_count_i16")
    n_e = int(indptr[n_nodes].item())
    cols = torch.empty(max(n_e, 1), dtype=torch.int32, device=dev)
    check(lib.gts_gg_touching_emit(ws.data_ptr(), n_nodes, indptr.data_ptr(), cols.data_ptr(), current_stream()),
          "gts_gg_touching_emit")
    ip = indptr.cpu().numpy().astype(np.int64)
    rows = np.repeat(np.arange(n_nodes, dtype=np.int64), np.diff(ip))
    return rows, cols[:n_e].cpu().numpy().astype(np.int64)


# ---- whole pipeline -------------------------------------------------------------------------------

def build_graph(voxel_intensities, voxel_labels, approx_num_nodes=5000, boxiness=0.5, k=10, timer=None,
                keep_on_device=False):
    """img2graph's arithmetic without networkx.  Returns a dict with `slic` (int32 labels after
    connectivity), `n_sv`, `partition` (int16, -1 = dropped), `feats`, `centroids`, `labels`
    (numpy) and `edges` = (rows, cols): for k > 0 the undirected kNN pairs (rows < cols), for
    k == 0 the face adjacency in both orientations with self-loops.  timer(name) is called at
    the end of each stage (host clock hooks for the measurement tool).  keep_on_device: `partition`,
    `feats`, `centroids` and `labels` stay tensors on the device."""
    tick = timer or (lambda name: None)
    d, h, w, c = _volume(voxel_intensities)
    if not 0 < approx_num_nodes <= MAX_SV:
        raise ValueError(f"approx_num_nodes must be in [1, {MAX_SV}]")
    if k and not 0 < k <= MAX_K:
        raise ValueError(f"k must be in [0, {MAX_K}]")
    dev = _device()
    # SLIC sees I = voxel_intensities.astype(float64) (the reference passes float64 to slic); the
    # statistics take the intensities as float32, the dtype the preprocessing pipeline produces
    img64 = _tensor(voxel_intensities, torch.float64, dev).reshape(d, h, w, c)
    scaled = gaussian(img64, 1.0, 1.0 / boxiness)
    del img64
    img32 = _tensor(voxel_intensities, torch.float32, dev).reshape(d, h, w, c)
    tick("gaussian")
    labels, _ = slic_rounds(scaled, approx_num_nodes, 10)
    tick("slic")
    lo, hi = connectivity_sizes((d, h, w), approx_num_nodes)
    slic_host, _ = _enforce_connectivity(labels.cpu().numpy(), lo, hi)
    tick("connectivity")
    n_sv = int(slic_host.max()) + 1
    if n_sv > MAX_SV:
        raise ValueError(f"SLIC produced {n_sv} supervoxels: the int16 partition holds at most {MAX_SV}")
    part = torch.from_numpy(slic_host).to(dev)
    lab = None if voxel_labels is None else _tensor(voxel_labels, torch.int16, dev)
    feats, cents, svl = supervoxel_statistics(part, img32, lab, n_sv)
    tick("statistics")
    new_part, nf, nc, nl = discard_empty_svs(part, feats, cents, svl)
    tick("discard")
    n_nodes = nf.shape[0]
    if k:
        edges = knn_edges(nc, k)
    else:
        edges = touching_edges(new_part, n_nodes)
    tick("edges")
    out = {"partition": new_part, "feats": nf, "centroids": nc, "labels": nl}
    if not keep_on_device:
        out = {name: t.cpu().numpy() for name, t in out.items()}
    return dict(out, slic=slic_host, n_sv=n_sv, edges=edges)


def symmetric_pairs(rows, cols):
    """The distinct (u, v) of the edge list in both orientations, sorted by u, then v: the row-major
    nonzeros of the symmetric 0/1 matrix with ones at (rows, cols) (a self-loop once)."""
    r = np.concatenate([rows, cols])
    c = np.concatenate([cols, rows])
    order = np.lexsort((c, r))
    return np.unique(np.stack([r[order], c[order]], axis=1), axis=0)


def graph_from_edges(edges, n_nodes):
    """gts.Graph of build_graph's edge list without networkx: the graph that
    gts.from_networkx(graph_io.load_networkx_graph(json)) gives for img2graph's networkx graph.
    Nodes 0..n-1 are inserted in order and the pairs in symmetric_pairs order, so every adjacency
    list of that graph is ascending and its directed edges are exactly symmetric_pairs."""
    from .graph import Graph

    pairs = symmetric_pairs(*edges)
    return Graph(pairs[:, 0], pairs[:, 1], n_nodes)
