"""HD95 on the device (gts.metrics.hd95s, H1-H5) against the scipy route (model.evaluation.calculate_hd95s).

    python tools/measure_hd95.py --out profiles/hd95/measure.json [--reps 10]

Host clock around a device synchronise, after warm-up runs:
  * hd95s against calculate_hd95s on one 240 x 240 x 155 pair with nested tumour-shaped regions and on one
    [1, 96, 96, 96] refinement crop (the mask mode), checking that both give the same doubles;
  * GNN.evaluate on one BraTS-size sample (240 x 240 x 152 voxels, 8^3 supervoxels, a spherical tumour),
    with the scipy route substituted for hd95s ("before") and as shipped ("after").
"""
import argparse
import json
import os
import sys
import tempfile
import time

import networkx as nx
import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import build, metrics  # noqa: E402
from model import evaluation  # noqa: E402


def blobs(shape, rng, n_blobs=5):
    """Nested regions: spheres of label 1 holding smaller ones of 2 and 3."""
    grid = np.indices(shape).reshape(len(shape), -1).T.astype(np.float64)
    vol = np.zeros(int(np.prod(shape)), dtype=np.int16)
    for _ in range(n_blobs):
        centre = rng.uniform(0, shape)
        radius = rng.uniform(0.15, 0.35) * min(s for s in shape if s > 1) + 1
        dist = np.sqrt(((grid - centre) ** 2).sum(axis=1))
        for k, lab in enumerate((1, 2, 3)):
            vol[dist < radius * (1 - 0.3 * k)] = lab
    return vol.reshape(shape)


def brats_pair(rng):
    pred, truth = np.zeros((240, 240, 155), np.int16), np.zeros((240, 240, 155), np.int16)
    sub = (slice(70, 170), slice(60, 180), slice(30, 125))
    shape = tuple(s.stop - s.start for s in sub)
    pred[sub], truth[sub] = blobs(shape, rng), blobs(shape, rng)
    return pred, truth


def timed_host(fn, reps, warmup=2):
    """Median seconds of fn() on the host clock, the device synchronised before and after each run."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), fn()


def compare(name, pred, truth, reps, scipy_reps):
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda()
    dev_s, got = timed_host(lambda: metrics.hd95s(p, t), reps)
    host_s, want = timed_host(lambda: evaluation.calculate_hd95s(pred, truth), scipy_reps, warmup=0)
    return {"case": name, "shape": list(pred.shape), "device_ms": round(dev_s * 1e3, 3),
            "scipy_ms": round(host_s * 1e3, 1), "speedup": round(host_s / dev_s, 1),
            "hd95": got, "equal": got == [float(w) for w in want]}


def write_gnn_sample(root, mri_id, rng, shape=(240, 240, 152), cube=8, in_feats=20):
    """One sample of the preprocessed on-disk layout GNN.evaluate reads (graph, supervoxels, labels)."""
    from data_processing import graph_io, nifti_io

    g = [s // cube for s in shape]
    n = g[0] * g[1] * g[2]
    ids = np.arange(n, dtype=np.int16).reshape(g)
    svs = np.repeat(np.repeat(np.repeat(ids, cube, 0), cube, 1), cube, 2)
    centres = (np.indices(g).reshape(3, -1).T + 0.5) * cube
    r = np.sqrt(((centres - np.array(shape) / 2) ** 2).sum(axis=1))
    node_labels = np.where(r < 20, 3, np.where(r < 30, 2, np.where(r < 45, 1, 0)))
    flip = rng.random(n) < 0.1
    node_labels[flip] = rng.integers(0, 4, size=int(flip.sum()))
    G = nx.Graph()
    for i in range(n):
        G.add_node(i, features=[float(v) for v in rng.standard_normal(in_feats)], label=int(node_labels[i]))
    idx = np.arange(n).reshape(g)
    for axis in range(3):
        a = np.take(idx, np.arange(idx.shape[axis] - 1), axis=axis).ravel()
        b = np.take(idx, np.arange(1, idx.shape[axis]), axis=axis).ravel()
        G.add_edges_from(zip(a.tolist(), b.tolist()), weight=1.0)
    folder = os.path.join(root, mri_id)
    os.makedirs(folder, exist_ok=True)
    graph_io.save_networkx_graph(G, os.path.join(folder, f"{mri_id}_nxgraph.json"))
    nifti_io.save_as_nifti(svs, os.path.join(folder, f"{mri_id}_supervoxels.nii.gz"))
    nifti_io.save_as_nifti(node_labels[svs].astype(np.int16), os.path.join(folder, f"{mri_id}_label.nii.gz"))


def gnn_evaluate(reps):
    import io
    from contextlib import redirect_stdout

    from data_processing.data_loader import ImageGraphDataset
    from model import gnn_model
    from utils.hyperparam_helpers import FullParamSet

    with tempfile.TemporaryDirectory() as tmp:
        root = tmp + os.sep
        write_gnn_sample(root, "BraTS_000", np.random.default_rng(5))
        with redirect_stdout(io.StringIO()):
            ds = ImageGraphDataset(root, "BraTS_", read_image=False, read_graph=True, read_label=True)
            hp = FullParamSet(1, 20, 4, 5e-3, 0.98, 1e-4, [0.1, 1, 2, 2], [64, 64], 0, None, None)
            torch.manual_seed(0)
            model = gnn_model.GNN("GSpool", hp, ds, batch_size=1)
        subset = torch.utils.data.Subset(ds, [0])
        after_s, after = timed_host(lambda: model.evaluate(subset), reps)
        shipped = gnn_model.gmetrics.hd95s
        gnn_model.gmetrics.hd95s = lambda p, t: evaluation.calculate_hd95s(p.cpu().numpy(), t.cpu().numpy())
        try:
            before_s, before = timed_host(lambda: model.evaluate(subset), max(1, reps // 3), warmup=1)
        finally:
            gnn_model.gmetrics.hd95s = shipped
        return {"case": "GNN.evaluate, one 240x240x152 sample", "before_ms": round(before_s * 1e3, 1),
                "after_ms": round(after_s * 1e3, 1), "speedup": round(before_s / after_s, 2),
                "equal": bool(np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scipy-reps", type=int, default=3)
    ap.add_argument("--skip-evaluate", action="store_true")
    args = ap.parse_args()
    build.build()
    rng = np.random.default_rng(0)
    rows = [compare("240x240x155", *brats_pair(rng), args.reps, args.scipy_reps)]
    crop = (1, 96, 96, 96)
    rows.append(compare("[1,96,96,96] crop (mask mode)", blobs(crop, rng), blobs(crop, rng), args.reps,
                        args.scipy_reps))
    if not args.skip_evaluate:
        rows.append(gnn_evaluate(args.reps))
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows}, f, indent=1)
    if not all(r["equal"] for r in rows):
        raise SystemExit("device and scipy routes disagree")


if __name__ == "__main__":
    main()
