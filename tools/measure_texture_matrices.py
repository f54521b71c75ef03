"""The run, zone and neighbourhood kernels (gts.texture with matrices=, X4-X6) on a BraTS-size
synthetic prediction and scan, stage by stage, and the same tables on the host.

    python tools/measure_texture_matrices.py --out profiles/texture_matrices/texture_matrices.json [--reps 10]

The prediction and the two images (`noisy`, `homogeneous`) are tools/measure_texture.py's, whose method this follows:
stage times are HIP events recorded where gts.texture.lesion_texture has enqueued each stage of the whole-tumour region
at 32 bins, median of --reps after 3 warm-ups; the added host time is a host clock around lesion_texture with and
without the four families, and around gts.measure.tumour_report with four modalities with and without them.  The device
tables are checked against the host route (tests/texture_matrices_ref.py: shifted-array comparison, scipy's label per
lesion and level) before anything is timed; the parent commit has no such feature and that route stands in for it.  No
time is a pass criterion.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd"), os.path.join(REPO, "tools")]

import measure_lesion_shape as shape_tool  # noqa: E402
import measure_texture as base_tool  # noqa: E402
from tests import texture_matrices_ref as M  # noqa: E402
from tests import texture_ref as R  # noqa: E402

NEW_STAGES = ("X4 run lengths", "X4 run counts", "X5 zones", "X6 neighbourhood", "matrices (copy)")


def clock(call, runs=5):
    import torch

    call()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"s_median": float(np.median(times)), "min": min(times), "max": max(times)}


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "texture_matrices", "texture_matrices.json"))
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--bins", type=int, default=32)
    parser.add_argument("--shape", type=int, nargs=3, default=list(shape_tool.SHAPE), help="for a rehearsal")
    args = parser.parse_args()
    import torch

    from gts import measure, texture

    shape = tuple(args.shape)
    labels = shape_tool.make_prediction(args.seed)
    if shape != shape_tool.SHAPE:
        labels = np.ascontiguousarray(labels[tuple(slice((n - s) // 2, (n - s) // 2 + s)
                                                   for n, s in zip(shape_tool.SHAPE, shape))])
    images = base_tool.make_images(args.seed, shape)
    result = {"volume": list(shape), "seed": args.seed, "bins": args.bins, "reps": args.reps,
              "device": torch.cuda.get_device_name(0), "images": {}}
    dev = torch.from_numpy(labels).cuda()
    every = texture.MATRICES
    for name, image in images.items():
        record = result["images"][name] = {}
        img = torch.from_numpy(image).cuda()
        t0 = time.perf_counter()
        R.lesion_texture(labels, image, "WT", bins=args.bins)
        t1 = time.perf_counter()
        want = M.lesion_matrices(labels, image, "WT", bins=args.bins)
        t2 = time.perf_counter()
        record["host_numpy_definition_s"] = {"tables_of_4aa": t1 - t0, "the_four_families_added": (t2 - t1) - (t1 - t0)}
        got = texture.lesion_texture(dev, img, "WT", bins=args.bins, matrices=every)
        for key in M.TABLE_KEYS:
            assert np.array_equal(got[key], want[key]), (name, key)
        record["device_equals_host_route"] = True
        big = int(want["n"].argmax())
        record["whole_tumour"] = {"lesions": len(want["n"]), "listed_voxels": int(want["n"].sum()),
                                  "largest_voxels": int(want["n"][big]), "longest_run": int(want["glrlm"].shape[3]),
                                  "runs": int(want["glrlm"].sum()), "zones": int(want["zones"][:, 3].sum()),
                                  "largest_zone": int(want["zones"][:, 2].max())}
        stages = base_tool.stage_times(
            lambda mark: texture.lesion_texture(dev, img, "WT", bins=args.bins, mark=mark, matrices=every), args.reps)
        record["stages_whole_tumour"] = base_tool.rows_of(stages)
        record["new_stages_sum_ms"] = sum(float(np.median(stages[s])) for s in NEW_STAGES)
        record["lesion_texture_call"] = {
            "without": clock(lambda: texture.lesion_texture(dev, img, "WT", bins=args.bins)),
            "with_four_families": clock(lambda: texture.lesion_texture(dev, img, "WT", bins=args.bins,
                                                                       matrices=every))}
        table = texture.lesion_texture(dev, img, "WT", bins=args.bins)
        t0 = time.perf_counter()
        [texture.derive(table, k) for k in range(len(table["root"]))]
        t1 = time.perf_counter()
        [texture.derive(got, k) for k in range(len(got["root"]))]
        record["derive_all_wt_lesions_s"] = {"without": t1 - t0, "with_four_families": time.perf_counter() - t1}
        print(name, json.dumps(record), flush=True)
    four = {f"m{k}": torch.from_numpy(images["noisy"] * (1.0 + 0.25 * k)).cuda() for k in range(4)}
    report = {}
    for label, kwargs in (("four_modalities", dict(texture=four, texture_bins=args.bins)),
                          ("four_modalities_all_families", dict(texture=four, texture_bins=args.bins,
                                                                texture_matrices=every))):
        report[label] = clock(lambda: measure.tumour_report(dev, **kwargs), 3)
    result["tumour_report"] = report
    print(json.dumps(report), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
