"""Connected-component clean-up on the device (gts.components, C1-C5) against the host route a user has
without it: scipy.ndimage.label + np.bincount on a copy of the volume.

    python tools/measure_components.py --out profiles/components/measure.json [--reps 20]

On one BraTS-size synthetic prediction (gts.synth_mri.make_prediction: nested tumour blobs plus 0.1 % salt noise)
and on an all-foreground volume of the same size (the longest runs and the largest single component), per
connectivity: remove_small_components end to end and component_roots alone, host clock around a device
synchronise, median after warm-up; the host route including the device-to-host copy of the volume; and a check
that both routes give the same volume and counts.

Per-pass kernel times come from a run of their own under the profiler, of the device calls only:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/measure_components.py --profile-workload
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import build, components, synth_mri  # noqa: E402

MIN_VOXELS, ET = 50, dict(et_label=4, et_min_voxels=500, et_replacement=1)


def timed(fn, reps, warmup=3):
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


def host_route(dev_labels, connectivity):
    """What a user does today: copy the volume to the host, scipy.ndimage.label, np.bincount, mask."""
    from scipy import ndimage

    labels = dev_labels.cpu().numpy()
    lab, k = ndimage.label(labels != 0, ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    sizes = np.bincount(lab.ravel(), minlength=k + 1)
    small = sizes < MIN_VOXELS
    small[0] = False
    out = np.where(small[lab], 0, labels)
    et = out == ET["et_label"]
    n_et = int(et.sum())
    relabelled = n_et if 0 < n_et < ET["et_min_voxels"] else 0
    if relabelled:
        out[et] = ET["et_replacement"]
    return out, [k, int(small.sum()), int(sizes[small].sum()), relabelled]


def cases():
    yield "blobs + 0.1 % salt", synth_mri.make_prediction(0, synth_mri.BRATS_SHAPE, salt=0.001)
    yield "all foreground", np.full(synth_mri.BRATS_SHAPE, 2, dtype=np.int16)


def measure(name, labels, connectivity, reps, scipy_reps):
    dev = torch.from_numpy(labels).cuda()
    filter_s, (got, stats) = timed(lambda: components.remove_small_components(dev, MIN_VOXELS, connectivity, **ET), reps)
    roots_s, _ = timed(lambda: components.component_roots(dev, connectivity), reps)
    host_s, (want, want_stats) = timed(lambda: host_route(dev, connectivity), scipy_reps, warmup=1)
    stats = stats.cpu().tolist()
    return {"case": name, "shape": list(labels.shape), "connectivity": connectivity,
            "foreground_voxels": int((labels != 0).sum()), "stats": stats,
            "remove_small_components_ms": round(filter_s * 1e3, 3), "component_roots_ms": round(roots_s * 1e3, 3),
            "scipy_host_route_ms": round(host_s * 1e3, 1), "speedup": round(host_s / filter_s, 1),
            "equal": bool(np.array_equal(got.cpu().numpy(), want) and stats == want_stats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scipy-reps", type=int, default=3)
    ap.add_argument("--profile-workload", action="store_true",
                    help="five filter calls per case and connectivity and nothing else (for rocprofv3 --kernel-trace)")
    args = ap.parse_args()
    build.build()
    if args.profile_workload:
        for _, labels in cases():
            dev = torch.from_numpy(labels).cuda()
            for connectivity in (6, 26):
                for _ in range(5):
                    components.remove_small_components(dev, MIN_VOXELS, connectivity, **ET)
        torch.cuda.synchronize()
        return
    rows = [measure(name, labels, c, args.reps, args.scipy_reps) for name, labels in cases() for c in (6, 26)]
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
