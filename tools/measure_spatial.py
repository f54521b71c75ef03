"""The rotated / zoomed crop kernels (A3, A4 of csrc/gts_augment.hip) at the crop training runs them
at, beside A1 (the floor: one read, one write) and the torch route a user would write for the same result.

    python tools/measure_spatial.py --out profiles/spatial/measure.json [--reps 10] [--blocks 5] [--label linear]

A3: the 128 x 160 x 128 crop of 8 channels of tools/measure_augment.py (2.6 M voxels; 4 image + 4 logit channels)
with its int64 labels, rotated by 15 degrees about each axis and zoomed by 1.1, without noise and with noise on all
four image channels.  Bytes: what A1 moves, each channel and each label read once and written once, 2 (4 C + 8) per
voxel; the share is of the 8 TB/s HBM peak.
A4: a gradient of 4 channels over the same crop under the same plan.
Baselines, timed in the same process:
  a1     gts_augment_crop_f32 with the same affine and noise and no mirror.
  torch  permute to NCDHW, affine_grid + grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True), a
         nearest pass for the labels, the jitter and the noise, the permute back.  Its grid_sample backward (with
         respect to the input, on 4 channels) stands against A4.
HIP events around the calls, rotating over buffer sets larger than the 256 MiB Infinity Cache.  Every figure is the
median over --blocks blocks of the median of --reps calls, after warm-up, with the smallest and largest block median
beside it (the spread a comparison has to clear).  GTS_LIB_PATH times another build of the library; --label names it
in the output.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd"), os.path.join(REPO, "tools")]

from gts import _lib  # noqa: E402
from gts.augment import AugmentPlan, rotation_zoom_matrix  # noqa: E402

SHAPE, CHANNELS, IMAGE_CHANNELS, GRAD_CHANNELS = (128, 160, 128), 8, 4, 4
N_SETS = 4                  # 4 x (84 + 84 + 21 + 21 MB) = 840 MB
HBM_PEAK = 8.0e12
ANGLES, ZOOM = (15.0, 15.0, 15.0), 1.1


def block_medians(launch, sets, reps, blocks, warmup=2):
    for i in range(warmup * len(sets)):
        launch(sets[i % len(sets)])
    torch.cuda.synchronize()
    medians = []
    for _ in range(blocks):
        times = []
        for i in range(reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s = sets[i % len(sets)]
            start.record()
            launch(s)
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end) * 1e3)
        medians.append(statistics.median(times))
    return medians


def entry(medians, nbytes=None):
    us = statistics.median(medians)
    out = {"median_us": round(us, 2), "block_min_us": round(min(medians), 2), "block_max_us": round(max(medians), 2)}
    if nbytes is not None:
        out.update(bytes=nbytes, gb_per_s=round(nbytes / us / 1e3, 1),
                   share_of_hbm_peak=round(nbytes / (us * 1e-6) / HBM_PEAK, 3))
    return out


def plan_for(noisy, matrix):
    sigma = [0.05, 0.1, 0.02, 0.08] if noisy else [0.0] * 4
    return AugmentPlan((False, False, False), [1.05, 0.95, 1.1, 0.9], [0.05, -0.05, 0.1, -0.1], sigma, 0.0, (7, 0), 11,
                       matrix)


def torch_theta(matrix, dev):
    """affine_grid's theta [1, 3, 4] for the plan's matrix: normalised coordinates u_a = (index_a - c_a) / c_a with
    align_corners=True, axes in grid_sample's (W, H, D) order."""
    c = (np.asarray(SHAPE, dtype=np.float64) - 1) / 2
    theta = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            theta[i, j] = matrix[2 - i, 2 - j] * c[2 - j] / c[2 - i]
    return torch.from_numpy(theta).float().to(dev)[None]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--label", default="library", help="what build of the library this is (recorded in the output)")
    ap.add_argument("--kernels-only", action="store_true", help="skip the torch route (A/B runs of two builds)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_spatial needs an MI355X: there is nothing to time without one")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st, p = _lib.current_stream(), _lib.ptr
    v = SHAPE[0] * SHAPE[1] * SHAPE[2]
    matrix = rotation_zoom_matrix(ANGLES, ZOOM)
    mat = (ctypes.c_double * 9)(*matrix.reshape(-1))
    g = torch.Generator(device=dev).manual_seed(0)
    sets = [dict(x=torch.randn(*SHAPE, CHANNELS, device=dev, generator=g),
                 y=torch.randint(0, 4, (v,), device=dev, generator=g),
                 x_out=torch.empty(*SHAPE, CHANNELS, device=dev), y_out=torch.empty(v, dtype=torch.int64, device=dev))
            for _ in range(N_SETS)]
    nbytes = 2 * (4 * CHANNELS + 8) * v
    result = {"device": torch.cuda.get_device_name(0), "label": args.label, "library": os.path.basename(_lib.LIB_PATH),
              "reps": args.reps, "blocks": args.blocks, "shape": list(SHAPE), "channels": CHANNELS,
              "image_channels": IMAGE_CHANNELS, "angles_deg": list(ANGLES), "zoom": ZOOM,
              "hbm_peak_bytes_per_s": HBM_PEAK, "a3": {}, "a1": {}, "torch": {}}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    theta = torch_theta(matrix, dev)
    for noisy in (False, True):
        plan = plan_for(noisy, matrix)
        params = torch.from_numpy(np.stack([plan.scale, plan.shift, plan.sigma], axis=1)).to(dev)
        key = "noise" if noisy else "no_noise"

        def a3(s):
            _lib.check(lib.gts_augment_spatial_f32(p(s["x"]), p(s["y"]), p(params), mat, p(s["x_out"]), p(s["y_out"]),
                                                   *SHAPE, CHANNELS, IMAGE_CHANNELS, 0, plan.seed64, plan.step, st), "A3")

        def a1(s):
            _lib.check(lib.gts_augment_crop_f32(p(s["x"]), p(s["y"]), p(params), p(s["x_out"]), p(s["y_out"]), *SHAPE,
                                                CHANNELS, IMAGE_CHANNELS, 0, plan.seed64, plan.step, st), "A1")

        scale, shift, sigma = (torch.from_numpy(a).to(dev) for a in (plan.scale, plan.shift, plan.sigma))

        def torch_route(s):
            xn = s["x"].permute(3, 0, 1, 2)[None]
            grid = F.affine_grid(theta, (1, CHANNELS) + SHAPE, align_corners=True)
            out = F.grid_sample(xn, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]
            lab = F.grid_sample(s["y"].view((1, 1) + SHAPE).float(), grid, mode="nearest", padding_mode="zeros",
                                align_corners=True).long().reshape(-1)
            out = out.permute(1, 2, 3, 0)
            image = out[..., :IMAGE_CHANNELS] * scale + shift
            if noisy:
                image = image + torch.randn_like(image) * sigma
            return torch.cat([image, out[..., IMAGE_CHANNELS:]], dim=-1), lab

        result["a3"][key] = entry(block_medians(a3, sets, args.reps, args.blocks), nbytes)
        result["a1"][key] = entry(block_medians(a1, sets, args.reps, args.blocks), nbytes)
        line = (f"{key:9s} A3 {result['a3'][key]['median_us']:9.2f} us ({result['a3'][key]['share_of_hbm_peak']:.3f} of "
                f"peak)   A1 {result['a1'][key]['median_us']:9.2f} us")
        if not args.kernels_only:
            result["torch"][key] = entry(block_medians(torch_route, sets, args.reps, args.blocks))
            line += f"   torch {result['torch'][key]['median_us']:9.2f} us"
            if not noisy:       # the two routes resample the same volume (float32 grid against float64: no claim)
                a3(sets[0])
                ours = sets[0]["x_out"].clone()
                theirs, _ = torch_route(sets[0])
                result["torch"]["max_abs_difference_to_a3"] = float((ours - theirs).abs().max())
                del ours, theirs
        print(line, flush=True)
        save()

    # A4 against grid_sample's backward with respect to its input, 4 channels
    del sets
    torch.cuda.empty_cache()
    back_sets = [dict(dy=torch.randn(*SHAPE, GRAD_CHANNELS, device=dev, generator=g),
                      dx=torch.empty(*SHAPE, GRAD_CHANNELS, device=dev)) for _ in range(N_SETS)]

    def a4(s):
        _lib.check(lib.gts_augment_spatial_bwd_f32(p(s["dy"]), mat, p(s["dx"]), *SHAPE, GRAD_CHANNELS, 0, st), "A4")

    result["a4"] = entry(block_medians(a4, back_sets, args.reps, args.blocks), 2 * 4 * GRAD_CHANNELS * v)
    line = f"A4 {result['a4']['median_us']:9.2f} us"
    if not args.kernels_only:
        xn = torch.zeros((1, GRAD_CHANNELS) + SHAPE, device=dev, requires_grad=True)
        grid = F.affine_grid(theta, (1, GRAD_CHANNELS) + SHAPE, align_corners=True)
        out = F.grid_sample(xn, grid, mode="bilinear", padding_mode="zeros", align_corners=True)

        def torch_back(s):
            return torch.autograd.grad(out, xn, s["dy"].permute(3, 0, 1, 2)[None], retain_graph=True)[0]

        result["torch"]["grid_sample_backward"] = entry(block_medians(torch_back, back_sets, args.reps, args.blocks))
        line += f"   grid_sample backward {result['torch']['grid_sample_backward']['median_us']:9.2f} us"
    print(line, flush=True)
    save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
