"""Times of the dataset-statistics path (gts.dataset_stats, scripts/compute_dataset_stats.py) on BraTS-size
synthetic scans, next to the numpy restatement's time for the same scans on the same machine.

    python tools/measure_dataset_stats.py --scans 3 --out profiles/dataset_stats/measure.json

Per scan, with a host clock after a device synchronisation: decode (gzip NIfTI read of four modalities and
the labels, staging), upload, D1, D2, D3; then the numpy restatement (tests/dataset_stats_ref.reference_form,
the reference's float32 arithmetic) on the decoded arrays.  Then scans per second of the command line tool's
loop (decode on the thread pool around the GPU) over the same folder.  --kernels-only runs the device stages
alone (kernel-trace runs).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    build.build()
    from data_processing import nifti_io
    from gts import dataset_stats, intake
    from scripts import compute_dataset_stats, preprocess_dataset
    from tests import dataset_stats_ref

    tmp = tempfile.mkdtemp(prefix="measure_dataset_stats_")
    raw = os.path.join(tmp, "raw")
    ids = [f"BraTS_{i:03d}" for i in range(args.scans + 1)]              # the first one warms up
    for i, sid in enumerate(ids):
        synth_mri.write_sample(raw, sid, 800 + i)
    scans = preprocess_dataset.find_scans(raw, "")
    mods, label_ext = list(synth_mri.MODALITY_EXTS), "_seg.nii.gz"

    results = []
    for sid in ids:
        t = {}
        clock = [time.perf_counter()]

        def tick(name):
            torch.cuda.synchronize()
            now = time.perf_counter()
            t[name + "_ms"] = round((now - clock[0]) * 1e3, 3)
            clock[0] = now

        vols = nifti_io.read_in_patient_sample_raw(scans[sid], mods)
        lab = nifti_io.read_in_labels(scans[sid], label_ext)
        staged, staged_lab = intake.stage_scan(vols), dataset_stats.stage_labels(lab)
        tick("decode")
        got = dataset_stats.scan_stats(staged, staged_lab, timer=tick)
        t["gpu_ms"] = round(t["upload_ms"] + t["D1_ms"] + t["D2_ms"] + t["D3_ms"], 3)
        if not args.kernels_only:
            img = dataset_stats_ref.stack(vols)
            start = time.perf_counter()
            mu, sigma = dataset_stats_ref.reference_form(img, lab)
            t["numpy_ms"] = round((time.perf_counter() - start) * 1e3, 3)
            t["numpy_minus_gpu_mean"] = [float(x) for x in (mu - got.mean)]
        t.update(scan=sid, n=got.n, dtype=str(staged.dtype), mean=[float(x) for x in got.mean],
                 std=[float(x) for x in got.std])
        results.append(t)
        print(json.dumps(t), flush=True)
    report = {"warmup": results[0], "scans": results[1:]}
    timed = results[1:]
    summary = {"gpu_ms_per_scan": float(np.median([r["gpu_ms"] for r in timed])),
               "decode_ms_per_scan": float(np.median([r["decode_ms"] for r in timed]))}
    if not args.kernels_only:
        summary["numpy_ms_per_scan"] = float(np.median([r["numpy_ms"] for r in timed]))
        start = time.perf_counter()
        with redirect_stdout(io.StringIO()):
            per_scan, failed = compute_dataset_stats.compute(scans, mods, label_ext)
        wall = time.perf_counter() - start
        summary.update(folder_scans=len(ids), folder_failed=len(failed), folder_scans_per_s=len(ids) / wall,
                       folder_s_per_scan=wall / len(ids))
        summary["decode_share_of_serial_scan"] = summary["decode_ms_per_scan"] / (
            summary["decode_ms_per_scan"] + summary["gpu_ms_per_scan"])
    report["summary"] = summary
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
