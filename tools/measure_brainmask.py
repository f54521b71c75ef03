"""The brain-extraction kernels (gts.brainmask, S1-S6) at BraTS size against the bytes they have to move,
and one whole mask at the defaults against the same steps in scipy on the host (tests/brainmask_ref.py).

    python tools/measure_brainmask.py --out profiles/brainmask/measure.json [--reps 20]
    python tools/measure_brainmask.py --host-only --out profiles/brainmask/host.json          # no GPU

A 240 x 240 x 155 head phantom (gts.synth_mri.make_head_sample, its t1 channel as int16).  Stage times are medians of
HIP-event brackets around one call of the wrapper (a stage is one to seven launches and, for S1, a copy of two
integers to the host).  Compulsory bytes: S1 and S2 read the volume; the threshold reads it and writes the mask; S3
reads a mask and writes a mask (its one- and two-byte intermediates are not compulsory and are listed apart); S6 reads
four modalities and the mask and writes four.  S4 and S5 are bounded by the union-find of C1-C3 and get no byte figure.
Shares are of the 8 TB/s HBM peak.  The whole mask is a host clock around brainmask.brain_mask, which synchronises
after S1, S2, S4 and S5 to bring integers to the host.  The parent commit has no brain extraction; the scipy route
stands in for "no such feature".  No time is a pass criterion.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from tests import brainmask_ref as R  # noqa: E402

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


def host_route(t1):
    """Seconds of every step of the scipy route at the defaults, and its mask."""
    clock, t0 = {}, time.perf_counter()

    def tick(name):
        nonlocal t0
        now = time.perf_counter()
        clock[name] = now - t0
        t0 = now

    n, hi = R.brain_range(t1)
    t, _, _ = R.threshold_from_counts(R.histogram(t1, hi), hi, 0.1)
    m0 = R.positive(t1) & (t1.astype(np.float64) >= t)
    tick("range, histogram, threshold")
    e = R.erode(m0, 9, 0)
    tick("erode R2 = 9")
    keep = R.largest_component(e, 6)[0]
    tick("largest component")
    d = R.dilate(keep, 9)
    tick("dilate R2 = 9")
    c = R.erode(R.dilate(d, 4), 4, 1)
    tick("close R2 = 4")
    b = R.fill_holes(c)
    tick("fill holes")
    clock["whole"] = sum(clock.values())
    return clock, b


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "brainmask", "measure.json"))
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--host-only", action="store_true", help="only the scipy route on the host (no GPU)")
    parser.add_argument("--seed", type=int, default=0, help="of the phantom")
    args = parser.parse_args()
    from gts import synth_mri

    img, _, truth = synth_mri.make_head_sample(args.seed, SHAPE)
    t1 = np.ascontiguousarray(img[..., 1].astype(np.int16))
    result = {"volume": list(SHAPE), "seed": args.seed}
    if args.host_only:
        clock, mask = host_route(t1)
        result["host_scipy_s"] = clock
        result["host_dice_against_truth"] = R.dice(mask, truth)
        print(json.dumps(result), flush=True)
    else:
        import torch

        from gts import _lib, brainmask, ops

        _lib.load()
        dev = torch.device("cuda", 0)
        result["device"] = torch.cuda.get_device_name(0)
        result["reps"] = args.reps
        vol = torch.from_numpy(t1).to(dev)
        scan = torch.from_numpy(np.ascontiguousarray(img.astype(np.int16).transpose(3, 0, 1, 2))).to(dev)
        voxels = vol.numel()
        n, hi = ops.brain_range(vol)
        t = brainmask.threshold_from_counts(ops.brain_histogram(vol, hi).cpu().numpy(), hi)[0]
        m0, _ = ops.brain_threshold(vol, t)
        eroded = ops.ball_erode(m0, 9)
        keep, _ = ops.largest_component(eroded)
        dilated = ops.ball_dilate(keep, 9)
        closed = ops.ball_erode(ops.ball_dilate(dilated, 4), 4, 1)
        mask, _ = ops.fill_holes(closed)
        morph = voxels * (2 + 2)
        extra = voxels * (1 + 1 + 2 + 2)            # S3's intermediates, each written and read once
        cases = [("S1 range (ends in a copy to the host)", lambda: ops.brain_range(vol), voxels * 2, None),
                 ("S2 histogram", lambda: ops.brain_histogram(vol, hi), voxels * 2, None),
                 ("S2 threshold mask", lambda: ops.brain_threshold(vol, t), voxels * 4, None),
                 ("S3 erode R2 = 9, threshold mask", lambda: ops.ball_erode(m0, 9), morph, extra),
                 ("S3 dilate R2 = 9, kept component", lambda: ops.ball_dilate(keep, 9), morph, extra),
                 ("S3 dilate R2 = 4", lambda: ops.ball_dilate(dilated, 4), morph, extra),
                 ("S3 erode R2 = 4, outside set", lambda: ops.ball_erode(dilated, 4, 1), morph, extra),
                 ("S3 dilate R2 = 255 (the widest window)", lambda: ops.ball_dilate(keep, 255), morph, extra),
                 ("S4 largest component, eroded mask", lambda: ops.largest_component(eroded), None, None),
                 ("S5 fill holes", lambda: ops.fill_holes(closed), None, None),
                 ("S6 apply, 4 x int16", lambda: ops.apply_mask(scan, mask), voxels * (2 + 16), None)]
        rows = []
        for name, launch, nbytes, more in cases:
            med, low, high = event_ms(launch, args.reps)
            row = {"stage": name, "ms": med, "min_ms": low, "max_ms": high}
            if nbytes is not None:
                row.update(compulsory_bytes=nbytes, ms_at_8TBps=1e3 * nbytes / PEAK_BYTES_PER_S,
                           achieved_bytes_per_s=nbytes / (med * 1e-3),
                           fraction_of_hbm_peak=nbytes / (med * 1e-3) / PEAK_BYTES_PER_S)
            if more is not None:
                row["intermediate_bytes"] = more
            rows.append(row)
            print(json.dumps(row), flush=True)
        result["stages"] = rows
        brainmask.brain_mask(vol)                                            # warm
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got, report = brainmask.brain_mask(vol)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        result["brain_mask"] = {"gpu_s_median_of_5": float(np.median(times)), "gpu_s_all": times, "report": report,
                                "dice_against_truth": R.dice(got.cpu().numpy(), truth)}
        print(json.dumps(result["brain_mask"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
