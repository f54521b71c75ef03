"""The uncertainty kernels (U1, U2 of csrc/gts_uncertainty.hip) beside the routes a user would write
with torch on the same GPU, and with numpy on the host.

    python tools/measure_uncertainty.py --out profiles/uncertainty/measure.json [--reps 20]

U1: the three region maps of a 128 x 160 x 128 crop (2.6 M rows of 4 class sums, 40 terms) scattered into a zeroed
140 x 172 x 140 x 3 uint8 volume.  Bytes moved by the launch: 16 B read and 3 B written per crop voxel; the zero fill
of the volume (3 B per volume voxel) is the caller's and is timed separately, as `ops.region_uncertainty_rows` does
both.  torch route: per region the float64 chain of the definition (adds, divide, clamp, minimum, multiply, round, NaN
-> 100) and an advanced-indexing store.
U2: the 3 x 4 x 102 counts of a BraTS-size volume (240 x 240 x 155 = 8.9 M voxels), 7 B read per voxel, on a scan-like
input (2 % tumour, maps non-zero on 5 % of the voxels) and on a random one (every voxel through the LDS atomics).
torch route: one torch.bincount of outcome * 102 + value per region; host route: the numpy masks of the definition at
the default thresholds (tests/uncertainty_ref.qu_scores), arrays already on the host.
HIP events around the calls on preallocated buffers, median of --reps after warm-up, rotating over buffer sets that
together exceed the 256 MiB Infinity Cache so that every pass reads from HBM.  Shares are of the 8 TB/s HBM peak.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd"), os.path.join(REPO, "tools")]

from gts import _lib, ops  # noqa: E402
from measure_ensemble import HBM_PEAK, entry, median_us  # noqa: E402

CROP, VOLUME, TERMS = (128, 160, 128), (140, 172, 140), 40
SCAN = (240, 240, 155)
U1_BUFFERS = 7              # 7 x 42 MB of sums = 294 MB
U2_BUFFERS = 5              # 5 x 62 MB = 312 MB
REGION_CLASSES = ((1, 2, 3), (2, 3), (3,))


def measure_u1(lib, dev, reps):
    rows, n_vol = CROP[0] * CROP[1] * CROP[2], VOLUME[0] * VOLUME[1] * VOLUME[2]
    g = torch.Generator(device=dev).manual_seed(0)
    buffers = []
    for _ in range(U1_BUFFERS):
        sums = torch.zeros(rows, 4, device=dev)
        for _ in range(4):      # ten terms each: sums of 40 softmaxes without 40 tensors alive
            logits = [3.0 * torch.randn(rows, 4, device=dev, generator=g) for _ in range(2)]
            for _ in range(5):
                ops.softmax_accumulate(logits, sums)
        buffers.append(dict(sums=sums, out=torch.zeros((3,) + VOLUME, dtype=torch.uint8, device=dev)))
    offsets = [(v - c) // 2 for v, c in zip(VOLUME, CROP)]
    box = ops.CropBox(*[np.arange(o, o + c) for o, c in zip(offsets, CROP)], VOLUME, dev)
    st, p = _lib.current_stream(), _lib.ptr
    out = {"crop": list(CROP), "rows": rows, "terms": TERMS, "volume": list(VOLUME)}

    def u1(b):
        _lib.check(lib.gts_region_uncertainty_rows_u8(p(b["sums"]), p(box.dev[0]), p(box.dev[1]), p(box.dev[2]),
                                                      p(b["out"]), *CROP, *VOLUME, 4, TERMS, st), "U1")

    def fill(b):
        b["out"].zero_()

    def fill_and_u1(b):
        b["out"].zero_()
        u1(b)

    xs, ys, zs = (d.long() for d in box.dev)
    index = (xs[:, None, None], ys[None, :, None], zs[None, None, :])

    def torch_maps(b, zero=False):
        if zero:
            b["out"].zero_()
        s = b["sums"].double()
        for r, classes in enumerate(REGION_CLASSES):
            total = s[:, classes[0]]
            for c in classes[1:]:
                total = total + s[:, c]
            prob = total / float(TERMS)
            nan = torch.isnan(prob)
            prob = prob.clamp(0.0, 1.0)
            u = torch.round(200.0 * torch.minimum(prob, 1.0 - prob))
            b["out"][r][index] = torch.where(nan, 100.0, u).to(torch.uint8).view(CROP)

    out["u1"] = entry(median_us(u1, buffers, reps), 19 * rows)
    out["zero_fill"] = entry(median_us(fill, buffers, reps), 3 * n_vol)
    out["u1_with_zero_fill"] = entry(median_us(fill_and_u1, buffers, reps), 19 * rows + 3 * n_vol)
    out["u1_torch"] = {"median_us": round(median_us(torch_maps, buffers, reps), 2)}
    out["u1_torch_with_zero_fill"] = {"median_us": round(median_us(lambda b: torch_maps(b, True), buffers, reps), 2)}
    for name in ("u1", "zero_fill", "u1_with_zero_fill"):
        print(f"{name:20s} {out[name]['median_us']:9.2f} us  {out[name]['share_of_hbm_peak']:.3f} of the HBM peak",
              flush=True)
    print(f"torch: three maps {out['u1_torch']['median_us']:.2f} us, with the zero fill "
          f"{out['u1_torch_with_zero_fill']['median_us']:.2f} us", flush=True)
    b = buffers[0]
    mine = ops.region_uncertainty_rows(b["sums"], TERMS, box)
    torch_maps(b, True)
    out["u1_equals_torch"] = bool(torch.equal(mine, b["out"]))
    out["u1_nonzero_share"] = round(float((mine != 0).float().mean()), 4)
    return out


def scan_like(dev, seed):
    """(pred, truth int16, unc uint8 [3, n]) over SCAN: two nested tumour balls, the prediction a shifted copy, maps
    non-zero in a shell around the tumour."""
    g = torch.Generator(device=dev).manual_seed(seed)
    axes = [torch.arange(n, device=dev, dtype=torch.float32) for n in SCAN]

    def ball(centre, radius):
        d2 = sum(((a - c) ** 2).view([-1 if i == k else 1 for i in range(3)])
                 for k, (a, c) in enumerate(zip(axes, centre)))
        return d2 < radius ** 2

    def labels(centre):
        vol = torch.zeros(SCAN, dtype=torch.int16, device=dev)
        for radius, lab in ((34.0, 1), (22.0, 3), (10.0, 2)):
            vol[ball(centre, radius)] = lab
        return vol

    centre = [float(n) * 0.5 + float(torch.randn((), generator=g, device=dev)) * 10.0 for n in SCAN]
    truth, pred = labels(centre), labels([c + 2.0 for c in centre])
    near = ball(centre, 48.0)
    unc = torch.randint(0, 101, (3,) + SCAN, device=dev, generator=g).to(torch.uint8) * near
    return pred.reshape(-1), truth.reshape(-1), unc.reshape(3, -1).contiguous()


def random_like(dev, seed):
    n = SCAN[0] * SCAN[1] * SCAN[2]
    g = torch.Generator(device=dev).manual_seed(seed)
    pred = torch.randint(0, 4, (n,), device=dev, generator=g).to(torch.int16)
    truth = torch.randint(0, 4, (n,), device=dev, generator=g).to(torch.int16)
    return pred, truth, torch.randint(0, 101, (3, n), device=dev, generator=g).to(torch.uint8)


def torch_histogram(pred, truth, unc):
    masks = lambda t: (t != 0, (t == 2) | (t == 3), t == 3)           # noqa: E731
    hist = []
    for r, (P, G) in enumerate(zip(masks(pred), masks(truth))):
        outcome = torch.where(P, 0, 2) + torch.where(G, 0, 1)
        hist.append(torch.bincount(outcome * 102 + unc[r].long(), minlength=408).view(4, 102))
    return torch.stack(hist)


def measure_u2(lib, dev, reps):
    from tests import uncertainty_ref

    n = SCAN[0] * SCAN[1] * SCAN[2]
    st, p = _lib.current_stream(), _lib.ptr
    out = {"volume": list(SCAN), "voxels": n}
    hist = torch.zeros(4, 4, 102, dtype=torch.int64, device=dev)

    def u2(b):
        _lib.check(lib.gts_uncertainty_histogram(p(b[0]), p(b[1]), p(b[2]), p(hist), n, st), "U2")

    for name, make in (("scan_like", scan_like), ("random", random_like)):
        buffers = [make(dev, seed) for seed in range(U2_BUFFERS)]
        row = {"u2": entry(median_us(u2, buffers, reps), 7 * n),
               "torch_bincount": {"median_us": round(median_us(lambda b: torch_histogram(*b), buffers, reps), 2)}}
        pred, truth, unc = buffers[0]
        row["calm_share"] = round(float(((pred == 0) & (truth == 0) & (unc == 0).all(dim=0)).float().mean()), 4)
        row["u2_equals_torch"] = bool(torch.equal(ops.uncertainty_histogram(pred, truth, unc),
                                                  torch_histogram(pred, truth, unc)))
        host = [t.cpu().numpy() for t in buffers[0]]
        times = []
        for _ in range(3):
            start = time.perf_counter()
            uncertainty_ref.qu_scores(*host)
            times.append((time.perf_counter() - start) * 1e6)
        row["numpy_masks"] = {"median_us": round(statistics.median(times), 1), "reps": 3}
        out[name] = row
        print(f"U2 {name:10s} {row['u2']['median_us']:9.2f} us  {row['u2']['share_of_hbm_peak']:.3f} of the HBM peak; "
              f"torch.bincount {row['torch_bincount']['median_us']:.2f} us, numpy masks "
              f"{row['numpy_masks']['median_us']:.0f} us", flush=True)
        del buffers
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_uncertainty needs an MI355X: there is nothing to time without one")
    lib = _lib.load()           # the library as built by `python __graft_entry__.py`
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    result["u1"] = measure_u1(lib, dev, args.reps)
    save()
    torch.cuda.empty_cache()
    result["u2"] = measure_u2(lib, dev, args.reps)
    save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
