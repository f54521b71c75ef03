"""The augmentation kernels (A1, A2 of csrc/gts_augment.hip) at the sizes training runs them at,
beside the torch route a user would write on the same GPU, and what --augment adds to a training step.

    python tools/measure_augment.py --out profiles/augment/measure.json [--reps 20] [--skip-steps]

A1: a 128 x 160 x 128 crop of 8 channels (2.6 M voxels; 4 image + 4 logit channels) with its int64 labels, for
every combination of mirrored axes, without noise and with noise on all four image channels.  Bytes moved: each
channel read once and written once, each label read once and written once: 2 * (4 C + 8) per voxel.
A2: the node features of the headline batch, 4 graphs of 15 000 nodes, at the dataset's 20 features (and at the
benchmark's 4), without and with feature noise.  Bytes moved: 8 F per row.
torch route: torch.flip + a broadcast multiply / add on the image channels + torch.randn_like * sigma +
torch.cat with the logit channels, and torch.flip of the labels.
HIP events around the calls on preallocated buffers, median of --reps after warm-up, rotating over buffer sets
larger than the 256 MiB Infinity Cache so that every pass reads from HBM.  Shares are of the 8 TB/s HBM peak.
Unless --skip-steps: RefinementModel.train_step on that crop and JointModel.train_step on a 96^3 box of one
synthetic BraTS-size sample (the sample of tools/measure_joint_training.py), each with and without a plan.
"""
import argparse
import io
import itertools
import json
import os
import statistics
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd"), os.path.join(REPO, "tools")]

from gts import _lib, ops  # noqa: E402
from gts.augment import AugmentPlan  # noqa: E402

SHAPE, CHANNELS, IMAGE_CHANNELS = (128, 160, 128), 8, 4
N_SETS = 4                  # 4 x (84 + 84 + 21 + 21 MB) = 840 MB
HBM_PEAK = 8.0e12


def median_us(launch, sets, reps, warmup=2):
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


def entry(us, nbytes):
    return {"median_us": round(us, 2), "bytes": nbytes, "gb_per_s": round(nbytes / us / 1e3, 1),
            "share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)}


def plan_for(flips, noisy):
    sigma = [0.05, 0.1, 0.02, 0.08] if noisy else [0.0] * 4
    return AugmentPlan(flips, [1.05, 0.95, 1.1, 0.9], [0.05, -0.05, 0.1, -0.1], sigma, 0.0, (7, 0), 11)


def measure_crop(lib, dev, reps):
    v = SHAPE[0] * SHAPE[1] * SHAPE[2]
    g = torch.Generator(device=dev).manual_seed(0)
    sets = [dict(x=torch.randn(*SHAPE, CHANNELS, device=dev, generator=g),
                 y=torch.randint(0, 4, (v,), device=dev, generator=g),
                 x_out=torch.empty(*SHAPE, CHANNELS, device=dev), y_out=torch.empty(v, dtype=torch.int64, device=dev))
            for _ in range(N_SETS)]
    st, p = _lib.current_stream(), _lib.ptr
    nbytes = 2 * (4 * CHANNELS + 8) * v
    out = {"shape": list(SHAPE), "channels": CHANNELS, "image_channels": IMAGE_CHANNELS, "a1": {}, "torch": {}}
    for flips in itertools.product((False, True), repeat=3):
        name = "".join(a for a, f in zip("xyz", flips) if f) or "none"
        for noisy in (False, True):
            plan = plan_for(flips, noisy)
            params = torch.from_numpy(np.stack([plan.scale, plan.shift, plan.sigma], axis=1)).to(dev)

            def a1(s):
                _lib.check(lib.gts_augment_crop_f32(p(s["x"]), p(s["y"]), p(params), p(s["x_out"]), p(s["y_out"]),
                                                    *SHAPE, CHANNELS, IMAGE_CHANNELS, plan.flip_mask, plan.seed64,
                                                    plan.step, st), "A1")

            scale = torch.from_numpy(plan.scale).to(dev)
            shift = torch.from_numpy(plan.shift).to(dev)
            sigma = torch.from_numpy(plan.sigma).to(dev)
            dims = [ax for ax in range(3) if flips[ax]]

            def torch_route(s):
                x, y = (torch.flip(s["x"], dims), torch.flip(s["y"].view(SHAPE), dims)) if dims else (s["x"], s["y"])
                image = x[..., :IMAGE_CHANNELS] * scale + shift
                if noisy:
                    image = image + torch.randn_like(image) * sigma
                return torch.cat([image, x[..., IMAGE_CHANNELS:]], dim=-1), y.reshape(-1)

            key = f"flip_{name}_{'noise' if noisy else 'no_noise'}"
            out["a1"][key] = entry(median_us(a1, sets, reps), nbytes)
            out["torch"][key] = {"median_us": round(median_us(torch_route, sets, reps), 2)}
            print(f"A1 {key:24s} {out['a1'][key]['median_us']:9.2f} us  {out['a1'][key]['share_of_hbm_peak']:.3f} of peak"
                  f"   torch {out['torch'][key]['median_us']:9.2f} us", flush=True)
    return out


def measure_features(lib, dev, reps):
    sizes = [15000] * 4
    n = sum(sizes)
    out = {"graphs": len(sizes), "rows": n, "a2": {}, "torch": {}}
    st, p = _lib.current_stream(), _lib.ptr
    row_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    row_ptr_dev = torch.from_numpy(row_ptr).to(dev)
    owner = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev))
    for f, m in ((20, 4), (4, 4)):
        g = torch.Generator(device=dev).manual_seed(1)
        n_sets = 64         # 64 x 2 x 4.8 MB: past the Infinity Cache at F = 20
        sets = [dict(x=torch.randn(n, f, device=dev, generator=g), out=torch.empty(n, f, device=dev))
                for _ in range(n_sets)]
        params = torch.rand(len(sizes), m, 2, device=dev, generator=g) + 0.5
        per_feature = params.repeat_interleave(f // m, dim=1)          # [B, F, 2]
        for sigma in (0.0, 0.05):
            def a2(s):
                _lib.check(lib.gts_augment_features_f32(p(s["x"]), p(row_ptr_dev), row_ptr.ctypes.data, p(params),
                                                        p(s["out"]), n, f, m, len(sizes), sigma, 7, 11, st), "A2")

            def torch_route(s):
                y = s["x"] * per_feature[owner, :, 0] + per_feature[owner, :, 1]
                return y + torch.randn_like(y) * sigma if sigma else y

            key = f"F{f}_{'noise' if sigma else 'no_noise'}"
            out["a2"][key] = entry(median_us(a2, sets, reps * 4), 8 * f * n)
            out["torch"][key] = {"median_us": round(median_us(torch_route, sets, reps * 4), 2)}
            print(f"A2 {key:24s} {out['a2'][key]['median_us']:9.2f} us  {out['a2'][key]['share_of_hbm_peak']:.3f} of peak"
                  f"   torch {out['torch'][key]['median_us']:9.2f} us", flush=True)
    return out


def measure_steps(dev, reps):
    import measure_joint_training as mjt
    from model.cnn_model import RefinementModel
    from model.joint_model import JointModel
    from utils.hyperparam_helpers import populate_hardcoded_hyperparameters

    gnn_hp, cnn_hp = populate_hardcoded_hyperparameters("GSpool"), populate_hardcoded_hyperparameters("CNN")
    plan = plan_for((True, False, True), True)
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        cnn = RefinementModel(cnn_hp, None, None)
        joint = JointModel("GSpool", gnn_hp, cnn_hp, None)
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(*SHAPE, CHANNELS, device=dev, generator=g)
    y = torch.randint(0, 4, (x.numel() // CHANNELS,), device=dev, generator=g)
    out = {"refinement": {"crop": list(SHAPE)}, "joint": {}}
    out["refinement"]["step_ms"] = mjt.timed(lambda: cnn.train_step(x, y), reps)
    out["refinement"]["step_with_augment_ms"] = mjt.timed(lambda: cnn.train_step(*ops.augment_crop(x, y, plan)), reps)
    s = mjt.make_sample(0, 15000, dev)
    box = mjt.centred_box(tuple(s["svs"].shape), 96, dev)
    joint.crop_box = lambda logits, svs: box
    args = (s["graph"], s["feats"], s["node_labels"], s["img"], s["svs"], s["voxel_labels"], s["lists"])
    out["joint"].update(box=list(box.shape), nodes=s["graph"].n)
    out["joint"]["step_ms"] = mjt.timed(lambda: joint.train_step(*args), reps)
    out["joint"]["step_with_augment_ms"] = mjt.timed(lambda: joint.train_step(*args, plan=plan), reps)
    for name in ("refinement", "joint"):
        r = out[name]
        r["overhead_ms"] = round(r["step_with_augment_ms"] - r["step_ms"], 4)
        print(f"{name} step {r['step_ms']:.3f} ms, with a plan {r['step_with_augment_ms']:.3f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true", help="kernels and the torch route only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_augment needs an MI355X: there is nothing to time without one")
    lib = _lib.load()           # the library as built by `python __graft_entry__.py`
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    result["crop"] = measure_crop(lib, dev, args.reps)
    save()
    result["features"] = measure_features(lib, dev, args.reps)
    save()
    if not args.skip_steps:
        result["steps"] = measure_steps(dev, max(5, args.reps // 2))
        save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
