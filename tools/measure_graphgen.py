"""Per-stage times of graph generation (G1-G8) on a BraTS-size synthetic sample.

    python tools/measure_graphgen.py --volumes 3 --out profiles/graphgen/measure.json

Device stages are timed with HIP events (G1, each G2 assignment and G3 update, G5, G6, G7/G8),
host stages with a host clock (NIfTI read, normalize, G4 connectivity, JSON / NIfTI write, the
whole CLI sample).  The fp64 operations and bytes of one G2 round are counted from the shapes.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import build, graphgen as gg, synth_mri  # noqa: E402


def g2_counts(shape, n_centres, window, channels):
    """fp64 FLOPs and minimum bytes of one assignment round (two window passes)."""
    d, h, w = shape
    per_centre = np.prod([min(4 * s + 1, dim) for s, dim in zip(window, shape)])
    evals = float(per_centre) * n_centres
    flops_per_eval = 3 * 2 + 2 + 1 + 3 * channels + 1          # 3 diffs + 3 squares, 2 adds, 1 scale, colour, 1 add
    flops = 2 * evals * flops_per_eval                           # pass A and pass B evaluate the same distances
    vox = d * h * w
    bytes_min = vox * (8 * channels) + vox * (8 + 4) * 2 + vox * 4   # image once, best/winner set + read, labels
    return evals, flops, bytes_min


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=3)
    ap.add_argument("--n", type=int, default=15000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    build.build()
    from data_processing import graph_io, nifti_io
    from data_processing.image_processing import determine_brain_crop, normalize_img, standardize_img
    from mri2graph.graphgen import _graph
    from scripts import preprocess_dataset as cli

    stream = torch.cuda.current_stream()
    results = []
    tmp = tempfile.mkdtemp()
    for v in range(args.volumes + 1):                            # volume 0 is the warm-up
        folder = synth_mri.write_sample(tmp, f"BraTS_{v:03d}", 500 + v)
        rec = {}
        t0 = time.perf_counter()
        img = nifti_io.read_in_patient_sample(folder, list(synth_mri.MODALITY_EXTS))
        lab = nifti_io.read_in_labels(folder, "_seg.nii.gz")
        rec["host_nifti_read_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        crop = determine_brain_crop(img)
        data = standardize_img(normalize_img(img[crop]), np.float32(cli.STANDARDIZATION_STATS[0]),
                               np.float32(cli.STANDARDIZATION_STATS[1]))
        labels = cli.swap_labels_from_brats(lab[crop])
        rec["host_normalize_s"] = time.perf_counter() - t0
        rec["shape"] = list(data.shape)
        dev = torch.device("cuda", 0)
        x32 = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(stream)
        scaled = gg.gaussian(x32.to(torch.float64), 1.0, 2.0)
        ev[1].record(stream)
        torch.cuda.synchronize()
        rec["g1_ms"] = ev[0].elapsed_time(ev[1])
        marks = [torch.cuda.Event(enable_timing=True)]
        marks[0].record(stream)
        names = []

        def on_round(i, stage):
            e = torch.cuda.Event(enable_timing=True)
            e.record(stream)
            marks.append(e)
            names.append(stage)

        labels_d, n_c = gg.slic_rounds(scaled, args.n, 10, on_round)
        torch.cuda.synchronize()
        per = [marks[i].elapsed_time(marks[i + 1]) for i in range(len(names))]
        rec["g2_assign_ms"] = [t for t, s in zip(per, names) if s == "assign"]
        rec["g3_update_ms"] = [t for t, s in zip(per, names) if s == "update"]
        rec["n_centres"] = n_c
        t0 = time.perf_counter()
        lo, hi = gg.connectivity_sizes(data.shape[:3], args.n)
        host_lab = labels_d.cpu().numpy()
        conn, n_sv = gg.enforce_connectivity(host_lab, lo, hi)
        rec["host_g4_connectivity_s"] = time.perf_counter() - t0
        rec["n_sv"] = n_sv

        def timed(fn, *a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            r = fn(*a)
            e1.record(stream)
            torch.cuda.synchronize()
            return r, e0.elapsed_time(e1)

        part = torch.from_numpy(conn).to(dev)
        lab_d = torch.from_numpy(labels).to(dev)
        (feats, cents, svl), rec["g5_ms"] = timed(gg.supervoxel_statistics, part, x32, lab_d, n_sv)
        (npart, nf, nc, nl), rec["g6_ms"] = timed(gg.discard_empty_svs, part, feats, cents, svl)
        rec["n_nodes"] = int(nf.shape[0])
        cand, rec["g7_candidates_ms"] = timed(gg.knn_candidates, nc, 10)
        t0 = time.perf_counter()
        picks = gg.knn_greedy(cand.cpu().numpy(), 10)
        rec["host_g7_greedy_s"] = time.perf_counter() - t0
        _, rec["g8_touching_ms_incl_host_copy"] = timed(gg.touching_edges, npart, int(nf.shape[0]))
        rows = np.repeat(np.arange(picks.shape[0]), 10).reshape(picks.shape)
        g = _graph(int(nf.shape[0]), rows[picks >= 0], picks[picks >= 0], 1.0)
        for nidx in g.nodes:
            g.nodes[nidx]["label"] = int(nl[nidx])
            g.nodes[nidx]["features"] = list(nf[nidx].cpu().numpy())
        t0 = time.perf_counter()
        graph_io.save_networkx_graph(g, os.path.join(tmp, "g.json"))
        rec["host_json_write_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        nifti_io.save_as_nifti(data, os.path.join(tmp, "in.nii.gz"))
        nifti_io.save_as_nifti(npart.cpu().numpy(), os.path.join(tmp, "sv.nii.gz"))
        nifti_io.save_as_nifti(labels, os.path.join(tmp, "lab.nii.gz"))
        rec["host_nifti_write_s"] = time.perf_counter() - t0
        # whole CLI sample: read -> img2graph -> write, one process, one sample
        gen = cli.DataPreprocessor(cli.build_parser().parse_args(["-d", folder + "/..", "-l", "_seg.nii.gz",
                                                                  "-o", os.path.join(tmp, "out"), "-n", str(args.n)]))
        gen.all_ids = [f"BraTS_{v:03d}"]
        t0 = time.perf_counter()
        assert not gen.run()
        rec["cli_sample_s"] = time.perf_counter() - t0
        evals, flops, nbytes = g2_counts(data.shape[:3], n_c, gg.slic_grid(data.shape[:3], args.n)[2], data.shape[3])
        rec["g2_round_distance_evals"] = evals
        rec["g2_round_fp64_flops"] = flops
        rec["g2_round_min_bytes"] = nbytes
        if v > 0:
            results.append(rec)
        print(json.dumps(rec), flush=True)
    summary = {"volumes": results, "device": torch.cuda.get_device_name(0)}
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
