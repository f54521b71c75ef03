"""Refinement-CNN training step: HIP (gts.conv3d C1-C5) against torch's path on the same GPU.

    python tools/measure_cnn_training.py --out profiles/cnn/measure.json [--reps 20]

Per shape and channel set, with the same weights and inputs on both paths:
  * HIP: each launch of the table in DESIGN.md §4h timed by HIP events (median of --reps), and the whole step
    (C1, C2, weighted CE, C4, C3, C5, FlatAdamW);
  * torch: CnnRefinementNet (replicate F.pad + MIOpen conv3d) + torch.nn.CrossEntropyLoss + torch.optim.AdamW,
    its forward, backward and whole step.
Useful FLOP per launch are counted from the shapes (2 * V * Cin * Cout * 125; C3 and C5 at the crop, not the
padded grid) and divided by the 157.3 TF fp32 matrix peak.  The shapes are chosen, not crop statistics: there
is no BraTS data here.  150 x 180 x 140 is the whole-brain box an empty GNN prediction selects.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import build, conv3d, ops  # noqa: E402
from gts.optim import FlatAdamW  # noqa: E402
from model.networks import CnnRefinementNet  # noqa: E402

PEAK_TF = 157.3
SHAPES = [(64, 64, 64), (96, 96, 96), (128, 144, 112), (150, 180, 140)]
CHANNELS = [(8, 16, 4), (9, 16, 5)]


def timed(fn, reps):
    """Median milliseconds of `fn` over `reps` event-bracketed runs after two warm-ups."""
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def measure(dims, cin, cmid, cout, reps, dev):
    torch.manual_seed(0)
    v = dims[0] * dims[1] * dims[2]
    net = CnnRefinementNet(cin, cout, [cmid]).to(dev)
    ref = CnnRefinementNet(cin, cout, [cmid]).to(dev)
    ref.load_state_dict(net.state_dict())
    x = torch.randn(*dims, cin, device=dev)
    y = torch.randint(0, cout, (v,), device=dev)
    cw = torch.tensor([0.1] + [5.0] * (cout - 1), device=dev)
    c1, c2 = net.conv_layers
    h1 = conv3d.conv3d_fwd(x, c1.weight.detach(), c1.bias.detach(), True)
    h1v = h1.view(*dims, cmid)
    dy = torch.randn(v, cout, device=dev)
    dz1 = conv3d.conv3d_bwd_data(dy, c2.weight.detach(), dims, h=h1)
    launches = {
        "C1 conv1 fwd+bias+relu": (lambda: conv3d.conv3d_fwd(x, c1.weight.detach(), c1.bias.detach(), True), cin * cmid),
        "C2 conv2 fwd+bias": (lambda: conv3d.conv3d_fwd(h1v, c2.weight.detach(), c2.bias.detach(), False), cmid * cout),
        "C3 conv2 data grad+mask": (lambda: conv3d.conv3d_bwd_data(dy, c2.weight.detach(), dims, h=h1), cmid * cout),
        "C4 conv2 weight+bias grad": (lambda: conv3d.conv3d_bwd_weight(h1v, dy, cout), cmid * cout),
        "C5 conv1 weight+bias grad": (lambda: conv3d.conv3d_bwd_weight(x, dz1, cmid), cin * cmid),
    }
    out = {"dims": list(dims), "channels": [cin, cmid, cout], "voxels": v, "launches": {}}
    for name, (fn, cc) in launches.items():
        ms = timed(fn, reps)
        flop = 2.0 * v * cc * 125
        out["launches"][name] = {"ms": ms, "gflop": flop / 1e9, "tflops": flop / ms / 1e9,
                                 "peak_fraction": flop / ms / 1e9 / PEAK_TF}
    opt = FlatAdamW(net.parameters(), lr=1e-4, weight_decay=1e-4)

    def hip_step():
        loss = ops.weighted_cross_entropy(conv3d.refinement_logits(x, net), y, cw)
        opt.zero_grad()
        loss.backward()
        opt.step()

    xc = x.movedim(-1, 0)[None].contiguous()
    yc = y.view(1, *dims)
    loss_fn = torch.nn.CrossEntropyLoss(weight=cw)
    topt = torch.optim.AdamW(ref.parameters(), lr=1e-4, weight_decay=1e-4)

    def torch_fwd():
        with torch.no_grad():
            ref(xc)

    def torch_step():
        loss = loss_fn(ref(xc), yc)
        topt.zero_grad()
        loss.backward()
        topt.step()

    out["hip_step_ms"] = timed(hip_step, reps)
    out["torch_fwd_ms"] = timed(torch_fwd, reps)
    out["torch_step_ms"] = timed(torch_step, reps)
    out["hip_fwd_ms"] = out["launches"]["C1 conv1 fwd+bias+relu"]["ms"] + out["launches"]["C2 conv2 fwd+bias"]["ms"]
    out["step_speedup"] = out["torch_step_ms"] / out["hip_step_ms"]
    return out


def sweep(dev, reps):
    """Weight-gradient launches at 96^3 with the channel counts varied one at a time: the output-channel rows
    (C4's 4 of 16 MFMA rows) and the input-channel columns (halo chunk width, column groups)."""
    dims = (96, 96, 96)
    v = dims[0] * dims[1] * dims[2]
    torch.manual_seed(0)
    rows = []
    for cin, cout in ((16, 4), (16, 8), (16, 16), (4, 16), (8, 16), (12, 16)):
        x = torch.randn(*dims, cin, device=dev)
        dy = torch.randn(v, cout, device=dev)
        ms = timed(lambda: conv3d.conv3d_bwd_weight(x, dy, cout), reps)
        flop = 2.0 * v * cin * cout * 125
        rows.append({"cin": cin, "cout": cout, "ms": ms, "peak_fraction": flop / ms / 1e9 / PEAK_TF})
        print(f"wgrad 96^3 cin {cin:2d} cout {cout:2d}: {ms:7.3f} ms {rows[-1]['peak_fraction']:.3f} of peak")
    return rows


def pmc_workload(dev):
    """C4 and C5 of one 96^3 8->16->4 step, three times each (for a counter run)."""
    dims = (96, 96, 96)
    v = dims[0] * dims[1] * dims[2]
    torch.manual_seed(0)
    x, h1 = torch.randn(*dims, 8, device=dev), torch.randn(*dims, 16, device=dev)
    dy, dz1 = torch.randn(v, 4, device=dev), torch.randn(v, 16, device=dev)
    for _ in range(3):
        conv3d.conv3d_bwd_weight(h1, dy, 4)
        conv3d.conv3d_bwd_weight(x, dz1, 16)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="one shape, one channel set (for a profiler run)")
    ap.add_argument("--only", type=int, nargs=6, metavar=("X", "Y", "Z", "CIN", "CMID", "COUT"), default=None,
                    help="measure this one shape and channel set")
    ap.add_argument("--sweep", action="store_true", help="only the weight-gradient channel sweep (sweep())")
    ap.add_argument("--pmc-workload", action="store_true", help="only C4 and C5 at 96^3, for rocprofv3 --pmc")
    ap.add_argument("--miopen-benchmark", action="store_true",
                    help="torch.backends.cudnn.benchmark = True: MIOpen searches its solutions (default: off, "
                         "torch's default selection)")
    args = ap.parse_args()
    build.build()
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.benchmark = args.miopen_benchmark
    if args.pmc_workload:
        pmc_workload(dev)
        return
    if args.sweep:
        rows = sweep(dev, args.reps)
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "peak_tf": PEAK_TF, "wgrad_sweep": rows}, f,
                          indent=1)
        return
    results = []
    shapes, channels = (SHAPES[1:2], CHANNELS[:1]) if args.quick else (SHAPES, CHANNELS)
    if args.only:
        shapes, channels = [tuple(args.only[:3])], [tuple(args.only[3:])]
    for dims in shapes:
        for ch in channels:
            r = measure(dims, *ch, args.reps, dev)
            results.append(r)
            print(json.dumps({k: r[k] for k in ("dims", "channels", "hip_step_ms", "torch_step_ms", "step_speedup")}))
            for name, l in r["launches"].items():
                print(f"    {name:28s} {l['ms']:8.3f} ms {l['tflops']:7.2f} TF {l['peak_fraction']:.3f} of peak")
            torch.cuda.empty_cache()
            if args.out:      # rewritten after every configuration
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                               "miopen_benchmark": args.miopen_benchmark, "peak_tf": PEAK_TF, "results": results},
                              f, indent=1)


if __name__ == "__main__":
    main()
