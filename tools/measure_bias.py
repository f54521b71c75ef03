"""The bias-field kernels (gts.bias, Z1-Z5) at BraTS size against the bytes they have to move, and one
whole correction at the defaults against the same loop in numpy on the host (tests/bias_ref.py).

    python tools/measure_bias.py --out profiles/bias/measure.json [--reps 20]
    python tools/measure_bias.py --host-only --out profiles/bias/host.json [--host-rounds 2]     # no GPU

A 240 x 240 x 155 phantom (tests/bias_ref.phantom: three tissue classes, a smooth multiplicative field) as int16.
Kernel times are medians of HIP-event brackets around one call, the lattices of all four default levels filled with
random values.  Compulsory bytes: Z1 reads the volume and writes u; Z2, Z3 and the mean read u; Z4 reads u and writes
and reads its row and plane sums once; apply reads the volume and writes the output (and the field).  The B-spline
tables (tens of KB) are not counted.  Fractions are of the 8 TB/s HBM peak.  The whole correction is a host clock
around bias.correct_volume, which ends in a copy to the host.  The host loop is timed over --host-rounds rounds per
level and reported per round: a full run of 200 rounds at this size takes several minutes.  Before this
feature the project had no bias correction at all; the host loop stands in for "no such feature".  No time is a pass
criterion.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from tests import bias_ref as R  # noqa: E402

SHAPE = (240, 240, 155)
PEAK_BYTES_PER_S = 8e12


def event_ms(launch, reps):
    import torch

    for _ in range(3):
        launch()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        launch()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def host_rounds(v, rounds):
    """Seconds per round of the numpy loop at the default lattices, over `rounds` rounds per level."""
    t0 = time.perf_counter()
    _, _, report = R.correct_volume(v, levels=4, spans0=1, iterations=rounds, tol=0.0)
    seconds = time.perf_counter() - t0
    done = sum(r["iterations"] for r in report)
    return {"host_numpy_rounds": done, "host_numpy_s": seconds, "host_numpy_s_per_round": seconds / max(done, 1),
            "host_numpy_s_for_200_rounds_extrapolated": 200 * seconds / max(done, 1)}


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "bias", "measure.json"))
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--host-only", action="store_true", help="only the numpy loop on the host (no GPU)")
    parser.add_argument("--host-rounds", type=int, default=0, help="rounds per level of the numpy loop (0: skip it)")
    parser.add_argument("--seed", type=int, default=0, help="of the phantom")
    args = parser.parse_args()
    v, clean, truth, classes = R.phantom(SHAPE[::-1], args.seed)
    v = np.rint(v).astype(np.int16)
    result = {"volume": list(SHAPE), "seed": args.seed}
    if args.host_only:
        result["host"] = host_rounds(v, max(args.host_rounds, 1))
        print(json.dumps(result["host"]), flush=True)
    else:
        import torch

        from gts import _lib, bias, ops

        _lib.load()
        dev = torch.device("cuda", 0)
        result["device"] = torch.cuda.get_device_name(0)
        result["reps"] = args.reps
        vol = torch.from_numpy(v).to(dev)
        voxels = vol.numel()
        tab = bias.tables(SHAPE, 1, 4, dev)
        rng = np.random.default_rng(1)
        lattice = torch.from_numpy(rng.uniform(-0.05, 0.05, tab.lattice_size())).to(dev)
        u, count = ops.bias_log(vol)
        lo, hi = ops.bias_range(u, tab, lattice).tolist()
        table = bias.sharpen(ops.bias_histogram(u, tab, lattice, lo, hi).cpu().numpy(), lo, hi)
        mean = float(ops.bias_mean(u, tab, lattice)[2])
        out = torch.empty(vol.shape, dtype=torch.float32, device=dev)
        rows_bytes = lambda level: SHAPE[1] * SHAPE[2] * tab.points(level) * 16 * 2 + SHAPE[2] * tab.points(level) ** 2 * 16 * 2  # noqa: E731
        cases = [("Z1 log, int16", lambda: ops.bias_log(vol), voxels * (2 + 4)),
                 ("Z2 range, 4 levels", lambda: ops.bias_range(u, tab, lattice), voxels * 4),
                 ("Z3 histogram, 4 levels", lambda: ops.bias_histogram(u, tab, lattice, lo, hi), voxels * 4)]
        for level in range(4):
            cases.append((f"Z4 fit, level {level} ({1 << level} spans)",
                          lambda level=level: ops.bias_fit(u, tab, lattice, level, lo, hi, table),
                          voxels * 4 + rows_bytes(level)))
        cases += [("Z5 mean, 4 levels", lambda: ops.bias_mean(u, tab, lattice), voxels * 4),
                  ("Z5 apply, int16", lambda: ops.bias_apply(vol, tab, lattice, mean, out=out), voxels * (2 + 4)),
                  ("Z5 apply with the field volume", lambda: ops.bias_apply(vol, tab, lattice, mean, want_field=True,
                                                                            out=out), voxels * (2 + 8))]
        rows = []
        for name, launch, nbytes in cases:
            med, low, high = event_ms(launch, args.reps)
            rows.append({"kernel": name, "ms": med, "min_ms": low, "max_ms": high, "compulsory_bytes": nbytes,
                         "ms_at_8TBps": 1e3 * nbytes / PEAK_BYTES_PER_S,
                         "achieved_bytes_per_s": nbytes / (med * 1e-3),
                         "fraction_of_hbm_peak": nbytes / (med * 1e-3) / PEAK_BYTES_PER_S})
            print(json.dumps(rows[-1]), flush=True)
        result["kernels"] = rows
        # ---- the whole correction of one modality at the defaults
        bias.correct_volume(vol, iterations=2)                               # warm
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            corrected, field, report = bias.correct_volume(vol, want_field=True)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        inside = classes > 0
        corr, rms = R.score(field.cpu().numpy(), truth, inside)
        rounds = sum(level["iterations"] for level in report["levels"])
        result["correct_volume"] = {"gpu_s_median_of_3": float(np.median(times)), "gpu_s_all": times, "rounds": rounds,
                                    "gpu_ms_per_round": 1e3 * float(np.median(times)) / max(rounds, 1),
                                    "levels": report["levels"], "reached_tol": [lv["last_change"] is not None and
                                                                                lv["last_change"] < bias.DEFAULT_TOL
                                                                                for lv in report["levels"]],
                                    "correlation_with_true_field": corr, "rms_residual": rms,
                                    "class_cv_in": R.class_cv(v, classes),
                                    "class_cv_out": R.class_cv(corrected.cpu().numpy(), classes),
                                    "class_cv_clean": R.class_cv(clean, classes)}
        print(json.dumps(result["correct_volume"]), flush=True)
        if args.host_rounds:
            result["host"] = host_rounds(v, args.host_rounds)
            print(json.dumps(result["host"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
