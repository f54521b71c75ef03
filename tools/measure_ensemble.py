"""The ensemble kernels (E1, E2 of csrc/gts_ensemble.hip) at a BraTS-size crop beside the torch route a
user would write on the same GPU, and what an ensemble costs per scan.

    python tools/measure_ensemble.py --out profiles/ensemble/measure.json [--reps 20] [--skip-scan]

E1: 8 logit sets of a 128 x 160 x 128 crop (2.6 M rows of 4 classes) added onto a running sum.  Bytes moved: every
set read once, the sum read once and written once: (8 + 2) * 16 B per row; when it starts the sum (overwrite),
(8 + 1) * 16.  torch route: acc.add_(torch.softmax(set, 1)) per set.
E2: the arg-max of that crop scattered, relabelled, into a zeroed 140 x 172 x 140 int16 volume.  Bytes moved: 16 B
read and 2 B written per crop voxel (the caller's memset is not part of the launch and is not timed on either side).
torch route: volume[box] = relabel[argmax(scores, 1)] by advanced indexing.
HIP events around the calls on preallocated buffers, median of --reps after warm-up, rotating over buffer sets that
together exceed the 256 MiB Infinity Cache so that every pass reads from HBM.  Shares are of the 8 TB/s HBM peak.
Unless --skip-scan: EnsemblePredictor.predict_joint on one synthetic BraTS-size scan (the sample of
tools/measure_joint_training.py) with the crop box pinned to the centred 128 x 160 x 128 box (or the volume, where
that is smaller), for 1 member x 1 view, 1 x 8 and 5 x 8, beside the single-model predict_one_sample on the same box
(MIOpen convolutions, as torch selects them by default) times the number of terms.
"""
import argparse
import io
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

CROP, VOLUME, CLASSES, SETS = (128, 160, 128), (140, 172, 140), 4, 8
N_BUFFERS = 2               # 2 x (8 + 1) x 42 MB = 755 MB
HBM_PEAK = 8.0e12


def median_us(launch, buffers, reps, warmup=2):
    for i in range(warmup * len(buffers)):
        launch(buffers[i % len(buffers)])
    torch.cuda.synchronize()
    times = []
    for i in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b = buffers[i % len(buffers)]
        start.record()
        launch(b)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e3)
    return statistics.median(times)


def entry(us, nbytes):
    return {"median_us": round(us, 2), "bytes": nbytes, "gb_per_s": round(nbytes / us / 1e3, 1),
            "share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)}


def measure_kernels(lib, dev, reps):
    import ctypes

    rows = CROP[0] * CROP[1] * CROP[2]
    g = torch.Generator(device=dev).manual_seed(0)
    buffers = [dict(sets=[3.0 * torch.randn(rows, CLASSES, device=dev, generator=g) for _ in range(SETS)],
                    acc=torch.zeros(rows, CLASSES, device=dev), out=torch.zeros(VOLUME, dtype=torch.int16, device=dev))
               for _ in range(N_BUFFERS)]
    for b in buffers:
        b["pointers"] = (ctypes.c_void_p * SETS)(*[t.data_ptr() for t in b["sets"]])
    offsets = [(v - c) // 2 for v, c in zip(VOLUME, CROP)]
    box = ops.CropBox(*[np.arange(o, o + c) for o, c in zip(offsets, CROP)], VOLUME, dev)
    relabel = torch.tensor([0, 2, 1, 4], dtype=torch.int16, device=dev)
    st, p = _lib.current_stream(), _lib.ptr
    out = {"crop": list(CROP), "rows": rows, "classes": CLASSES, "sets": SETS, "volume": list(VOLUME)}

    def e1(overwrite):
        def launch(b):
            _lib.check(lib.gts_softmax_accumulate_f32(b["pointers"], SETS, p(b["acc"]), rows, CLASSES, overwrite, st),
                       "E1")
        return launch

    def torch_e1(b):
        for s in b["sets"]:
            b["acc"].add_(torch.softmax(s, dim=1))

    def e2(b):
        _lib.check(lib.gts_argmax_scatter_rows_i16(p(b["acc"]), p(relabel), p(box.dev[0]), p(box.dev[1]), p(box.dev[2]),
                                                   p(b["out"]), *CROP, VOLUME[1], VOLUME[2], CLASSES, st), "E2")

    xs, ys, zs = (d.long() for d in box.dev)
    index = (xs[:, None, None], ys[None, :, None], zs[None, None, :])
    long_relabel = relabel.long()

    def torch_e2(b):
        b["out"][index] = long_relabel[torch.argmax(b["acc"], dim=1)].to(torch.int16).view(CROP)

    row_bytes = 4 * CLASSES
    out["e1_accumulate"] = entry(median_us(e1(0), buffers, reps), (SETS + 2) * row_bytes * rows)
    out["e1_overwrite"] = entry(median_us(e1(1), buffers, reps), (SETS + 1) * row_bytes * rows)
    out["e1_torch"] = {"median_us": round(median_us(torch_e1, buffers, reps), 2)}
    out["e2"] = entry(median_us(e2, buffers, reps), (row_bytes + 2) * rows)
    out["e2_torch"] = {"median_us": round(median_us(torch_e2, buffers, reps), 2)}
    for name in ("e1_accumulate", "e1_overwrite", "e2"):
        print(f"{name:16s} {out[name]['median_us']:9.2f} us  {out[name]['share_of_hbm_peak']:.3f} of the HBM peak",
              flush=True)
    print(f"torch: E1 {out['e1_torch']['median_us']:.2f} us, E2 {out['e2_torch']['median_us']:.2f} us", flush=True)
    # same results on both routes at this size (the sums differ in their last bits: torch's softmax is another sequence)
    b = buffers[0]
    mine = ops.softmax_accumulate(b["sets"])
    theirs = torch.zeros_like(mine)
    for s in b["sets"]:
        theirs.add_(torch.softmax(s, dim=1))
    out["e1_max_abs_diff_to_torch"] = float((mine - theirs).abs().max())
    mine_labels = ops.argmax_scatter_rows(mine, box, relabel)
    theirs_labels = torch.zeros_like(mine_labels)
    theirs_labels[index] = long_relabel[torch.argmax(mine, dim=1)].to(torch.int16).view(CROP)
    out["e2_equals_torch"] = bool(torch.equal(mine_labels, theirs_labels))
    return out


def measure_scan(dev, reps):
    import measure_joint_training as mjt
    from gts.ensemble import EnsemblePredictor, mirror_views
    from model.networks import CnnRefinementNet, init_graph_net
    from scripts import generate_joint_predictions as joint
    from utils.hyperparam_helpers import EvalParamSet

    s = mjt.make_sample(21, 15000, dev)
    shape = tuple(s["svs"].shape)
    extents = [min(c, n) for c, n in zip(CROP, shape)]
    box = ops.CropBox(*[np.arange((n - e) // 2, (n - e) // 2 + e) for n, e in zip(shape, extents)], shape, dev)
    joint.gnn_crop_box = lambda svs, node_logits, cleanup=None: box        # both routes take their box from here
    hp = EvalParamSet(in_feats=s["feats"].shape[1], out_classes=4, layer_sizes=[256] * 4, gat_heads=None,
                      gat_residuals=None)
    nets = []
    for seed in range(5):
        torch.manual_seed(seed)
        nets.append((init_graph_net("GSpool", hp).to(dev).eval(), CnnRefinementNet(8, 4, [16]).to(dev).eval()))
    relabel = torch.tensor([0, 2, 1, 4], dtype=torch.int16, device=dev)
    args = (s["graph"], s["feats"], s["img"], s["svs"], relabel)
    out = {"volume": list(shape), "box": list(box.shape), "voxels": int(np.prod(box.shape)), "nodes": s["graph"].n}
    with redirect_stdout(io.StringIO()):
        out["single_model_ms"] = mjt.timed(lambda: joint.predict_one_sample(*nets[0], *args), reps)
    print(f"predict_one_sample {out['single_model_ms']:.2f} ms per scan", flush=True)
    out["ensembles"] = []
    for members, axes in ((1, ""), (1, "xyz"), (5, "xyz")):
        predictor = EnsemblePredictor([g for g, _ in nets[:members]], [c for _, c in nets[:members]], mirror_views(axes))
        ms = mjt.timed(lambda: predictor.predict_joint(*args), reps)
        row = {"members": members, "views": len(predictor.views), "terms": predictor.terms, "predict_joint_ms": ms,
               "terms_times_single_model_ms": predictor.terms * out["single_model_ms"]}
        out["ensembles"].append(row)
        print(f"{members} member(s) x {row['views']} view(s): predict_joint {ms:.2f} ms per scan, "
              f"{row['terms']} x single model {row['terms_times_single_model_ms']:.2f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-scan", action="store_true", help="the two kernels and the torch route only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_ensemble needs an MI355X: there is nothing to time without one")
    lib = _lib.load()           # the library as built by `python __graft_entry__.py`
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    result["kernels"] = measure_kernels(lib, dev, args.reps)
    save()
    if not args.skip_scan:
        torch.cuda.empty_cache()
        result["scan"] = measure_scan(dev, max(5, args.reps // 2))
        save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
