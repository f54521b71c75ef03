"""The fused soft Dice + cross-entropy loss (D1, D2 of csrc/gts_dice_ce.hip) at the size of a crop,
beside the route the training loops took for cross-entropy alone: gts_weighted_ce_f32 (loss and unscaled gradient
in the forward) plus torch's multiply in the backward (the [N, C] multiply alone is timed; the index and division
kernels that form its scalar in `_WeightedCE.backward` are left out of the kernel figures and counted in the op ones).

    python tools/measure_dice_loss.py --out profiles/dice_loss/measure.json [--reps 20]

V = 128 x 160 x 128 rows, C = 4, regions "brats", class weights given.  HIP events around the launches alone (the
entry points are called on preallocated buffers), median of `reps` after warm-up; then the two ops through
autograd, forward + backward, the same way.  One set of tensors (42 MB logits, 21 MB labels, 42 MB gradient) fits
the 256 MiB Infinity Cache, so a repeat on the same buffers reads from it: every figure is taken twice, "warm" on
one set and "rotating" over 8 sets (840 MB), where a set has left the cache when its turn comes again.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import _lib, build, ops  # noqa: E402

SHAPE = (128, 160, 128)
N_SETS = 8
# bytes per row each route needs: logits 16, label 8, gradient 16
BYTES = {"d1": 24, "d2": 24 + 16, "d1_d2": 64, "ce_fwd": 24 + 16, "ce_scale": 16 + 16, "ce_fwd_scale": 72}


def median_us(launch, sets, reps, warmup=3):
    """Median microseconds between two events around launch(set), over the given buffer sets in turn."""
    for i in range(warmup * len(sets)):
        launch(sets[i % len(sets)])
    torch.cuda.synchronize()
    times = []
    for i in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s = sets[i % len(sets)]
        start.record()
        launch(s)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_dice_loss needs an MI355X: there is nothing to time without one")
    build.build()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    v, c = SHAPE[0] * SHAPE[1] * SHAPE[2], 4
    masks = ops.dice_region_masks("brats", c)
    host_masks = (ctypes.c_uint32 * len(masks))(*masks)
    w = torch.tensor([0.1, 1.0, 2.0, 2.0], device=dev)
    one = torch.ones((), device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(N_SETS):
        sets.append(dict(
            x=torch.randn(v, c, device=dev, generator=g) * 3, y=torch.randint(0, c, (v,), device=dev, generator=g),
            grad=torch.empty(v, c, device=dev), out=torch.empty(v, c, device=dev),
            stats=torch.zeros(ops.DICE_STATS_FLOATS, device=dev),
            ws=torch.empty(lib.gts_dice_ce_workspace(v, len(masks)) // 4, device=dev),
            ce_stats=torch.zeros(3, device=dev), ce_ws=torch.empty(lib.gts_weighted_ce_workspace(v) // 4, device=dev)))
    st = _lib.current_stream()
    p = _lib.ptr

    def d1(s):
        _lib.check(lib.gts_dice_ce_fwd_f32(p(s["x"]), p(s["y"]), p(w), host_masks, len(masks), 1.0, 1.0, 1.0,
                                           p(s["stats"]), p(s["ws"]), s["ws"].numel() * 4, v, c, st), "D1")

    def d2(s):
        _lib.check(lib.gts_dice_ce_bwd_f32(p(s["x"]), p(s["y"]), p(w), host_masks, len(masks), 1.0, 1.0, 1.0,
                                           p(s["stats"]), p(one), p(s["grad"]), v, c, st), "D2")

    def ce_fwd(s):
        _lib.check(lib.gts_weighted_ce_f32(p(s["x"]), p(s["y"]), p(w), p(s["grad"]), p(s["ce_ws"]),
                                           s["ce_ws"].numel() * 4, p(s["ce_stats"]), v, c, st), "CE")

    def ce_scale(s):             # the multiply alone: the scalar 1 / den is formed once, outside the events
        torch.mul(s["grad"], s["scale"], out=s["out"])

    def op_route(loss_fn):
        def run(s):
            x = s["x"].requires_grad_(True)
            loss_fn(x, s["y"], w).backward()
            x.grad = None
        return run

    routes = {"d1": d1, "d2": d2, "d1_d2": lambda s: (d1(s), d2(s)), "ce_fwd": ce_fwd, "ce_scale": ce_scale,
              "ce_fwd_scale": lambda s: (ce_fwd(s), ce_scale(s)),
              "op_dice_ce_fwd_bwd": op_route(ops.dice_ce_loss), "op_ce_fwd_bwd": op_route(ops.weighted_cross_entropy)}
    for s in sets:          # D2 and the multiply read what the forwards leave
        d1(s)
        ce_fwd(s)
        s["scale"] = one / s["ce_stats"][1]
    result = {"rows": v, "classes": c, "regions": "brats", "reps": args.reps, "sets_rotating": N_SETS,
              "device": torch.cuda.get_device_name(0), "bytes_per_row": BYTES, "median_us": {}, "gb_per_s": {}}
    for name, launch in routes.items():
        warm = median_us(launch, sets[:1], args.reps)
        rotating = median_us(launch, sets, args.reps)
        result["median_us"][name] = {"warm": round(warm, 2), "rotating": round(rotating, 2)}
        if name in BYTES:
            result["gb_per_s"][name] = {k: round(BYTES[name] * v / t / 1e3, 1)
                                        for k, t in (("warm", warm), ("rotating", rotating))}
        print(f"{name:20s} warm {warm:9.2f} us   rotating {rotating:9.2f} us", flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
