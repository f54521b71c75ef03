"""Per-stage times of the raw-scan segmenter (scripts/segment_scans.py) on BraTS-size synthetic scans,
and wall time per scan of the segmenter CLI against preprocess_dataset + generate_joint_predictions.

    python tools/measure_segment.py --volumes 3 --out profiles/segment/measure.json

Stages are timed with a host clock after a device synchronisation (decode, upload, I1, I2, I3, graph,
GNN, CNN, write).  I1-I3 are also timed alone with HIP events (each call includes its small copies to
the host).  The nets are random-initialised GSpool [256]*4 and the refinement CNN.  --skip-cli leaves
out the CLI comparison (kernel-trace runs).
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from contextlib import redirect_stdout

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import build, synth_mri  # noqa: E402


def _event_ms(fn, reps=10):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=3)
    ap.add_argument("--n", type=int, default=15000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cli", action="store_true")
    args = ap.parse_args()
    build.build()
    from data_processing import nifti_io
    from data_processing.image_processing import uncrop_to_brats_size
    from gts import graphgen, intake
    from model.networks import CnnRefinementNet, init_graph_net
    from scripts import generate_joint_predictions, preprocess_dataset, segment_scans
    from utils.hyperparam_helpers import EvalParamSet

    tmp = tempfile.mkdtemp(prefix="measure_segment_")
    raw = os.path.join(tmp, "raw")
    ids = [f"BraTS_{i:03d}" for i in range(args.volumes + 1)]           # the first one warms up
    for i, sid in enumerate(ids):
        synth_mri.write_sample(raw, sid, 500 + i)
    torch.manual_seed(0)
    hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
    gnn, cnn = os.path.join(tmp, "gnn.pt"), os.path.join(tmp, "cnn.pt")
    torch.save(init_graph_net("GSpool", hp).state_dict(), gnn)
    torch.save(CnnRefinementNet(8, 4, [16]).state_dict(), cnn)
    seg_args = segment_scans.build_parser().parse_args(["-d", raw, "-o", os.path.join(tmp, "seg"), "-g", gnn, "-c", cnn,
                                                        "-n", str(args.n)])
    seg = segment_scans.Segmenter(seg_args)
    seg.output_dir = os.path.join(tmp, "stages")
    os.makedirs(seg.output_dir)
    scans = segment_scans.find_inputs(raw, seg_args.modality_extensions)

    results = []
    for sid in ids:
        t = {}
        clock = [time.perf_counter()]

        def tick(name):
            torch.cuda.synchronize()
            now = time.perf_counter()
            t[name] = round((now - clock[0]) * 1e3, 3)
            clock[0] = now

        vols = nifti_io.read_in_patient_sample_raw(scans[sid], seg_args.modality_extensions)
        staged = intake.stage_scan(vols)
        tick("decode")
        image, crop, _ = intake.prepare_scan(staged, seg.mean, seg.std, timer=tick)
        res = graphgen.build_graph(image, None, args.n, 0.5, 10, keep_on_device=True)
        graph = graphgen.graph_from_edges(res["edges"], res["feats"].shape[0])
        feats = res["feats"].to(torch.float32)
        tick("graph")
        with torch.no_grad():
            seg.graph_net(graph.to(seg.device), feats)
        tick("gnn")
        pred = generate_joint_predictions.predict_one_sample(seg.graph_net, seg.conv_net, graph, feats, image,
                                                             res["partition"], seg.relabel)
        tick("gnn_cnn")
        t["cnn"] = round(t["gnn_cnn"] - t["gnn"], 3)
        seg.store(sid, uncrop_to_brats_size(crop, pred))
        tick("write")

        # I1-I3 alone (HIP events), on the upload of this scan
        src = staged.to(seg.device)
        shape = tuple(int(d) for d in staged.shape[1:][::-1])
        masks, _ = intake.occupancy(src, shape)
        xs, ys, zs, sizes = intake._index_lists(masks, seg.device)
        ranks = intake.quantile_ranks(int(np.prod(sizes)))
        top = np.ones(4, np.float32)
        t["event_upload_ms"] = _event_ms(lambda: staged.to(seg.device, non_blocking=True))
        t["event_I1_ms"] = _event_ms(lambda: intake.occupancy(src, shape))
        t["event_I2_ms"] = _event_ms(lambda: intake.order_stats(src, shape, (xs, ys, zs), sizes, ranks))
        t["event_I3_ms"] = _event_ms(lambda: intake.standardize(src, shape, (xs, ys, zs), sizes, top, seg.mean,
                                                                seg.std))
        t.update(scan=sid, dtype=str(staged.dtype), volume=list(shape), crop=list(sizes), nodes=int(res["feats"].shape[0]),
                 upload_bytes=int(staged.numel() * staged.element_size()))
        results.append(t)
        print(json.dumps(t), flush=True)
    report = {"stages_ms": results[1:], "warmup": results[0], "n": args.n}

    if not args.skip_cli:
        cli = {}
        sink = io.StringIO()
        start = time.perf_counter()
        with redirect_stdout(sink):
            rc = segment_scans.main(["-d", raw, "-o", os.path.join(tmp, "cli_seg"), "-g", gnn, "-c", cnn,
                                     "-n", str(args.n)])
        cli["segment_scans_s_per_scan"] = (time.perf_counter() - start) / len(ids)
        ds = os.path.join(tmp, "ds")
        start = time.perf_counter()
        with redirect_stdout(sink):
            rc |= preprocess_dataset.main(["-d", raw, "-o", ds, "-n", str(args.n)])
        mid = time.perf_counter()
        with redirect_stdout(sink):
            generate_joint_predictions.main(["-d", ds + "/", "-o", os.path.join(tmp, "cli_joint"), "-g", gnn, "-c", cnn])
        end = time.perf_counter()
        cli["preprocess_dataset_s_per_scan"] = (mid - start) / len(ids)
        cli["generate_joint_predictions_s_per_scan"] = (end - mid) / len(ids)
        cli["two_step_s_per_scan"] = (end - start) / len(ids)
        same = all(np.array_equal(nifti_io.read_nifti(os.path.join(tmp, "cli_seg", f"{s}.nii.gz"), np.int16),
                                  nifti_io.read_nifti(os.path.join(tmp, "cli_joint", f"{s}.nii.gz"), np.int16))
                   for s in ids)
        cli.update(scans=len(ids), exit_status=rc, outputs_equal=bool(same))
        report["cli"] = cli
        print(json.dumps(cli), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
