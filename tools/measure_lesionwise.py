"""Lesion-wise scoring on the device (gts.lesionwise, L1-L3 with C1-C3 and H1-H5) against the host route a user
has without it: the scipy reference of the definition (tests/lesionwise_ref.py: binary_dilation, two
ndimage.label calls, np.isin and a medpy-style hd95 per lesion), on 16 threads.

    python tools/measure_lesionwise.py --out profiles/lesionwise/measure.json [--reps 10]

On one BraTS-size pair (240 x 240 x 155): nested ground-truth blobs, a prediction that is a shifted copy with a few
satellite islands and 0.1 % salt noise.  lesionwise_scores end to end (all three regions, legacy numbers
included), dilate_region and lesion_tables alone, host clock around a device synchronise, median after warm-up;
the host route on the same arrays; and a check that both give the same record.

Per-kernel times come from a run of their own under the profiler, of the device calls only:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/measure_lesionwise.py --profile-workload
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import build, lesionwise, synth_mri  # noqa: E402
from tests import lesionwise_ref as ref  # noqa: E402


def make_pair(seed=0, shape=synth_mri.BRATS_SHAPE, salt=0.001, satellites=4):
    """(pred, truth) int16 internal labels: blobs_and_salt's pair with a few more satellite islands."""
    pred, truth = ref.blobs_and_salt(shape, seed, salt=salt)
    rng = np.random.default_rng(seed + 1)
    for _ in range(satellites):
        at = [int(rng.integers(8, n - 8)) for n in shape]
        pred[at[0]:at[0] + 3, at[1]:at[1] + 4, at[2]:at[2] + 3] = rng.integers(1, 4)
    return pred, truth


def timed(fn, reps, warmup=2):
    """Median seconds of fn() on the host clock, the device synchronised before and after each run."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), result


def same(got, want):
    keys = ("lw_dice", "lw_hd95", "dice", "hd95", "n_lesions", "n_scored", "n_fp", "n_fn")
    return all(got[r][k] == want[r][k] for r in ref.REGIONS for k in keys) and \
        all(got[r]["lesions"] == want[r]["lesions"] for r in ref.REGIONS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scipy-reps", type=int, default=3)
    ap.add_argument("--profile-workload", action="store_true",
                    help="five lesionwise_scores calls and nothing else (for rocprofv3 --kernel-trace)")
    args = ap.parse_args()
    build.build()
    pred, truth = make_pair()
    dev_pred, dev_truth = torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda()
    if args.profile_workload:
        for _ in range(5):
            lesionwise.lesionwise_scores(dev_pred, dev_truth)
        torch.cuda.synchronize()
        return
    scores_s, got = timed(lambda: lesionwise.lesionwise_scores(dev_pred, dev_truth), args.reps)
    dilate_s, _ = timed(lambda: lesionwise.dilate_region(dev_truth, "WT", 3), args.reps)
    tables_s, tables = timed(lambda: lesionwise.lesion_tables(dev_pred, dev_truth, "WT"), args.reps)
    host_s, want = timed(lambda: ref.lesionwise_scores(pred, truth), args.scipy_reps, warmup=1)
    row = {"shape": list(pred.shape), "predicted_voxels": int((pred != 0).sum()), "truth_voxels": int((truth != 0).sum()),
           "threads": int(os.environ["OMP_NUM_THREADS"]),
           "counts": {r: {k: got[r][k] for k in ("n_lesions", "n_scored", "n_fp", "n_fn")} for r in ref.REGIONS},
           "wt_components": len(tables["comp_sizes"]),
           "lesionwise_scores_ms": round(scores_s * 1e3, 3), "dilate_region_ms": round(dilate_s * 1e3, 3),
           "lesion_tables_ms": round(tables_s * 1e3, 3), "scipy_host_route_ms": round(host_s * 1e3, 1),
           "speedup": round(host_s / scores_s, 1), "equal": bool(same(got, want))}
    print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": [row]}, f, indent=1)
    if not row["equal"]:
        raise SystemExit("device and scipy routes disagree")


if __name__ == "__main__":
    main()
