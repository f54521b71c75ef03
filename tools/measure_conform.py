"""The conform kernel (gts.conform, F1) on a BraTS-size scan against the bytes it has to move and against the host
route a user has without it.

    python tools/measure_conform.py --out profiles/conform/measure.json [--reps 20] [--skip-host]

A 240 x 240 x 155 x 4 int16 scan (gts.synth_mri.make_sample).  Cases: the six axis permutations, each with one
axis flipped (exact mode), and one resampled case, 0.9375 x 0.9375 x 5 mm -> 1 mm (trilinear, x and y flipped).
Per case: the median HIP-event time of the kernel alone (tables already on the device), the compulsory bytes
(the input read once, the output written once), what those bytes take at the 8 TB/s peak, and the host
alternative on 16 threads: np.ascontiguousarray(np.transpose(np.flip(...))) per channel slab, or
scipy.ndimage.map_coordinates(order=1) per output slab.  No time is a pass criterion.
"""
import argparse
import itertools
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import build, conform, synth_mri  # noqa: E402

SHAPE = (240, 240, 155)
PEAK_BYTES_PER_S = 8e12
HOST_THREADS = 16
TARGET = (-1, -1, 1)


def affine_of(perm, signs, spacing):
    a = np.eye(4)
    a[:3, :3] = 0.0
    for j in range(3):
        a[perm[j], j] = signs[j] * spacing[j]
    return a


def kernel_ms(launch, reps):
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
    return float(np.median(times))


def host_reorient_ms(vols, plan, reps=3):
    """vols: [C, X, Y, Z] host array.  16 threads, each a slab of one channel along the slowest output axis."""
    flipped = [1 + j for j, f in enumerate(plan.flips) if f]
    view = np.transpose(np.flip(vols, axis=flipped) if flipped else vols, [0] + [1 + j for j in plan.source])
    out = np.empty(view.shape, dtype=vols.dtype)
    slabs = [(c, sl) for c in range(view.shape[0]) for sl in np.array_split(np.arange(view.shape[1]), HOST_THREADS // 4)]

    def work(job):
        c, sl = job
        out[c, sl[0]:sl[-1] + 1] = np.ascontiguousarray(view[c, sl[0]:sl[-1] + 1])
    times = []
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        for _ in range(reps):
            t0 = time.perf_counter()
            list(pool.map(work, slabs))
            times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times))


def host_resample_ms(vols, plan):
    """scipy.ndimage.map_coordinates(order=1) on the reoriented view, one output slab per job, 16 threads."""
    from scipy import ndimage

    flipped = [1 + j for j, f in enumerate(plan.flips) if f]
    view = np.transpose(np.flip(vols, axis=flipped) if flipped else vols, [0] + [1 + j for j in plan.source])
    steps = [1.0 / plan.spacing[j] for j in plan.source]
    ox, oy, oz = plan.out_shape
    out = np.empty((vols.shape[0], ox, oy, oz), dtype=np.float32)
    gy, gz = np.arange(oy) * steps[1], np.arange(oz) * steps[2]
    jobs = [(c, sl) for c in range(vols.shape[0]) for sl in np.array_split(np.arange(ox), HOST_THREADS)]

    def work(job):
        c, sl = job
        grid = np.meshgrid(sl * steps[0], gy, gz, indexing="ij")
        out[c, sl[0]:sl[-1] + 1] = ndimage.map_coordinates(view[c], grid, order=1, output=np.float32, mode="nearest")
    t0 = time.perf_counter()
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        list(pool.map(work, jobs))
    return 1e3 * (time.perf_counter() - t0)


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "conform", "measure.json"))
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--skip-host", action="store_true")
    args = parser.parse_args()
    build.build()
    img, _ = synth_mri.make_sample(7, SHAPE)
    vols = np.ascontiguousarray(np.moveaxis(img.astype(np.int16), 3, 0))          # [C, X, Y, Z]
    cases = []
    for k, perm in enumerate(itertools.permutations(range(3))):
        signs = [TARGET[perm[j]] for j in range(3)]
        signs[k % 3] *= -1                                                        # one flipped axis per case
        cases.append((f"perm {perm} flip axis {k % 3}", perm, tuple(signs), (1.0, 1.0, 1.0)))
    cases.append(("resample 0.9375 x 0.9375 x 5 mm, x and y flipped", (0, 1, 2), (1, 1, 1), (0.9375, 0.9375, 5.0)))
    rows = []
    for name, perm, signs, spacing in cases:
        # the stored scan: the pipeline-frame volume carried onto a grid of this orientation
        stored = np.transpose(vols, [0] + [1 + w for w in perm])
        flipped = [1 + j for j in range(3) if signs[j] != TARGET[perm[j]]]
        stored = np.ascontiguousarray(np.flip(stored, axis=flipped) if flipped else stored)
        plan = conform.plan(affine_of(perm, signs, spacing), stored.shape[1:])
        dev = torch.from_numpy(np.ascontiguousarray(np.transpose(stored, (0, 3, 2, 1)))).cuda()
        mode = conform.MODE_TRILINEAR if plan.resamples else conform.MODE_EXACT
        launch, out = conform._bind(dev, plan.source, plan.forward, mode, "measure_conform")
        ms = kernel_ms(launch, args.reps)
        nbytes = dev.numel() * dev.element_size() + out.numel() * out.element_size()
        row = {"case": name, "mode": "trilinear" if plan.resamples else "exact", "in_shape": list(stored.shape[1:]),
               "out_shape": list(plan.out_shape), "kernel_ms": ms, "compulsory_bytes": nbytes,
               "ms_at_8TBps": 1e3 * nbytes / PEAK_BYTES_PER_S, "achieved_TBps": nbytes / (ms * 1e-3) / 1e12,
               "fastest_axis_moves": plan.source[0] != 0}
        if not args.skip_host:
            row["host_16_threads_ms"] = host_resample_ms(stored, plan) if plan.resamples else host_reorient_ms(stored, plan)
            row["host_route"] = "scipy.ndimage.map_coordinates(order=1)" if plan.resamples else \
                "np.ascontiguousarray(np.transpose(np.flip(...)))"
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev, out, launch
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "scan": list(SHAPE) + [4], "dtype": "int16",
                   "reps": args.reps, "host_threads": HOST_THREADS, "cases": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
