"""Surface distances under a voxel spacing on the device (gts.metrics.surface_stats, H1-H2 and H3w-H5w) against the
unit-spacing path (gts.metrics.hd95_order_stats, H1-H5) and against the scipy route on the host.

    python tools/measure_surface.py --out profiles/surface/measure.json [--reps 10]

Host clock around a device synchronise, after warm-up runs, on one 240 x 240 x 155 pair with nested
tumour-shaped regions:
  * surface_stats with four tolerances for the units (1, 1, 1), (1, 1, 5) and (15, 15, 80), and hd95_order_stats
    on the same pair (the ratio is the cost of int64 values, the lists and the radix select);
  * the scipy route (binary_erosion, distance_transform_edt(sampling=units), np.percentile) once per spacing,
    checking that hd95s_mm gives the same doubles.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import _lib, metrics  # noqa: E402
from model import evaluation  # noqa: E402

SPACINGS = {"1x1x1": (1.0, 1.0, 1.0), "1x1x5": (1.0, 1.0, 5.0), "0.9375x0.9375x5": (0.9375, 0.9375, 5.0)}
TOLERANCES = (0.5, 1.0, 2.0, 5.0)


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


def scipy_hd95s_mm(pred, truth, units, scale_mm):
    """[WT, CT, ET] by the host route: model.evaluation's borders, scipy's EDT with sampling = units."""
    out = []
    footprint = generate_binary_structure(3, 1)
    for p, g in zip(evaluation._regions(pred), evaluation._regions(truth)):
        p, g = p.astype(bool), g.astype(bool)
        if not p.any() or not g.any():
            out.append(0.0 if not p.any() and not g.any() else 300.0)
            continue
        bp, bg = p ^ binary_erosion(p, structure=footprint), g ^ binary_erosion(g, structure=footprint)
        sampling = [float(u) for u in units]
        both = np.hstack((distance_transform_edt(~bg, sampling=sampling)[bp],
                          distance_transform_edt(~bp, sampling=sampling)[bg]))
        out.append(float(np.percentile(both * scale_mm, 95)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scipy-reps", type=int, default=1)
    args = ap.parse_args()
    _lib.load()
    pred, truth = brats_pair(np.random.default_rng(0))
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda()
    unit_s, _ = timed_host(lambda: metrics.hd95_order_stats(p, t), args.reps)
    rows = [{"case": "hd95_order_stats (unit spacing, H1-H5)", "device_ms": round(unit_s * 1e3, 3),
             "workspace_mib": round(_lib.load().gts_hd95_workspace(*pred.shape) / 2 ** 20, 1)}]
    for name, spacing in SPACINGS.items():
        units, scale = metrics.spacing_units(spacing)
        dev_s, table = timed_host(lambda: metrics.surface_stats(p, t, spacing, TOLERANCES), args.reps)
        got = metrics.hd95s_mm(p, t, spacing)
        host_s, want = timed_host(lambda: scipy_hd95s_mm(pred, truth, units, scale), args.scipy_reps, warmup=0)
        rows.append({"case": f"surface_stats, spacing {name} mm", "units": list(units), "scale_mm": scale,
                     "device_ms": round(dev_s * 1e3, 3), "ratio_to_unit_spacing": round(dev_s / unit_s, 2),
                     "scipy_ms": round(host_s * 1e3, 1), "speedup": round(host_s / dev_s, 1),
                     "workspace_mib": round(_lib.load().gts_surface_workspace(
                         *pred.shape, (ctypes.c_int64 * 3)(*units)) / 2 ** 20, 1),
                     "border_voxels": [int(v) for v in table[:, 0].cpu()], "hd95_mm": got,
                     "nsd": metrics.surface_dices(p, t, spacing, TOLERANCES), "equal": got == want})
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "shape": list(pred.shape),
                       "tolerances_mm": list(TOLERANCES), "rows": rows}, f, indent=1)
    if not all(r.get("equal", True) for r in rows):
        raise SystemExit("device and scipy routes disagree")


if __name__ == "__main__":
    main()
