"""The texture kernels (gts.texture, X1-X3) on a BraTS-size synthetic prediction and scan, stage by
stage, the same tables on the host, and the two forms of X3 against each other.

    python tools/measure_texture.py --build-direct                          # no GPU: builds the diag form of X3
    python tools/measure_texture.py --out profiles/texture/texture.json [--reps 10]

The prediction is tools/measure_lesion_shape.py's (240 x 240 x 155, 1 mm: one tumour of about 100 ml and 36 small
islands).  Two images: `noisy`, the T1ce channel of gts.synth_mri.make_sample(seed) (float32), and `homogeneous`, a
constant one, on which every add of a direction meets one counter.  Stage times are HIP events recorded where
gts.texture.lesion_texture has enqueued each stage of the whole-tumour region at 32 bins; the whole call is a host
clock around lesion_texture per region, and around gts.measure.tumour_report with and without four modalities.  The
device tables are checked against the host route (tests/texture_ref.py: scipy's label, numpy levels, bincount and
shifted-array comparison) before anything is timed; the parent commit has no such feature and that route stands in
for it.  X3 is timed in two forms in the same process, alternating: the library's (an LDS tile per work unit, flushed
with global atomics) and tools/diag/texture_glcm_direct.hip (global atomics straight from the voxel pass).  No time is
a pass criterion.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd"), os.path.join(REPO, "tools")]

import measure_lesion_shape as shape_tool  # noqa: E402
from tests import texture_ref as R  # noqa: E402

DIRECT_SRC = os.path.join(REPO, "tools", "diag", "texture_glcm_direct.hip")
DIRECT_LIB = os.path.join(REPO, "tools", "diag", "texture_glcm_direct.so")
KEYS = ("root", "n", "lo", "hi", "levels", "hist", "glcm")
REGIONS = ("WT", "CT", "ET")


def build_direct():
    from gts import build

    cmd = [build._hipcc(), *build.CXXFLAGS, "-shared", DIRECT_SRC, "-o", DIRECT_LIB]
    subprocess.run(cmd, check=True)
    return DIRECT_LIB


def make_images(seed, shape):
    from gts import synth_mri

    noisy = np.ascontiguousarray(synth_mri.make_sample(seed, shape)[0][..., 2], dtype=np.float32)
    return {"noisy": noisy, "homogeneous": np.full(shape, 100.0, dtype=np.float32)}


def stage_times(call, reps):
    """{stage: [ms]} of `call(mark)` over reps runs after 3 warm-ups, HIP events where a stage has been enqueued."""
    import torch

    stages = {}
    for rep in range(3 + reps):
        events = []

        def mark(stage):
            event = torch.cuda.Event(enable_timing=True)
            event.record()
            events.append((stage, event))

        mark("start")
        call(mark)
        torch.cuda.synchronize()
        if rep >= 3:
            for (_, before), (stage, after) in zip(events, events[1:]):
                stages.setdefault(stage, []).append(before.elapsed_time(after))
    return stages


def rows_of(stages):
    return [{"stage": s, "ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
            for s, t in stages.items()]


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "texture", "texture.json"))
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--bins", type=int, default=32)
    parser.add_argument("--build-direct", action="store_true", help="only build the diag form of X3 (no GPU)")
    parser.add_argument("--shape", type=int, nargs=3, default=list(shape_tool.SHAPE), help="for a rehearsal")
    args = parser.parse_args()
    if args.build_direct:
        print(build_direct())
        return
    import torch

    from gts import _lib, measure, texture

    shape = tuple(args.shape)
    labels = shape_tool.make_prediction(args.seed)
    if shape != shape_tool.SHAPE:
        labels = np.ascontiguousarray(labels[tuple(slice((n - s) // 2, (n - s) // 2 + s)
                                                   for n, s in zip(shape_tool.SHAPE, shape))])
    images = make_images(args.seed, shape)
    lib = _lib.load()
    result = {"volume": list(shape), "seed": args.seed, "bins": args.bins, "reps": args.reps,
              "device": torch.cuda.get_device_name(0), "images": {}}
    dev = torch.from_numpy(labels).cuda()
    direct = ctypes.CDLL(DIRECT_LIB).diag_texture_glcm_direct
    direct.argtypes, direct.restype = lib.gts_texture_glcm.argtypes, lib.gts_texture_glcm.restype
    shipped = lib.gts_texture_glcm
    for name, image in images.items():
        record = result["images"][name] = {}
        img = torch.from_numpy(image).cuda()
        host_s = {}
        for region in REGIONS:
            t0 = time.perf_counter()
            want = R.lesion_texture(labels, image, region, bins=args.bins)
            host_s[region] = time.perf_counter() - t0
            for form, fn in (("lds_tile", shipped), ("direct_global", direct)):
                lib.gts_texture_glcm = fn
                got = texture.lesion_texture(dev, img, region, bins=args.bins)
                for key in KEYS:
                    assert np.array_equal(got[key], want[key]), (name, region, form, key)
            lib.gts_texture_glcm = shipped
            if region == "WT":
                big = int(want["n"].argmax())
                record["whole_tumour"] = {"lesions": len(want["n"]), "listed_voxels": int(want["n"].sum()),
                                          "largest_voxels": int(want["n"][big]),
                                          "largest_levels": int(want["levels"][big]),
                                          "work_units": len(texture.work_units(want["n"])),
                                          "pairs_largest": int(want["glcm"][big].sum()) // 2}
        host_s["whole"] = sum(host_s.values())
        record["host_numpy_definition_s"] = host_s
        record["device_equals_host_route_both_forms"] = True
        record["stages_whole_tumour"] = rows_of(stage_times(
            lambda mark: texture.lesion_texture(dev, img, "WT", bins=args.bins, mark=mark), args.reps))
        record["stages_sum_ms"] = sum(r["ms"] for r in record["stages_whole_tumour"])
        # the two forms of X3, alternating in one process
        x3 = {"lds_tile": [], "direct_global": []}
        for _ in range(2):
            for form, fn in (("lds_tile", shipped), ("direct_global", direct)):
                lib.gts_texture_glcm = fn
                stages = stage_times(lambda mark: texture.lesion_texture(dev, img, "WT", bins=args.bins, mark=mark),
                                     args.reps)
                x3[form] += stages["X3 co-occurrence"]
        lib.gts_texture_glcm = shipped
        record["x3_forms_ms"] = {form: {"median": float(np.median(t)), "min": float(np.min(t)),
                                        "max": float(np.max(t)), "runs": len(t)} for form, t in x3.items()}
        calls = {}
        for region in REGIONS:
            texture.lesion_texture(dev, img, region, bins=args.bins)
            times = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                texture.lesion_texture(dev, img, region, bins=args.bins)
                times.append(time.perf_counter() - t0)
            calls[region] = {"gpu_s_median_of_5": float(np.median(times)), "min": min(times), "max": max(times)}
        record["lesion_texture_call"] = calls
        t0 = time.perf_counter()
        table = texture.lesion_texture(dev, img, "WT", bins=args.bins)
        [texture.derive(table, k) for k in range(len(table["root"]))]
        record["derive_all_wt_lesions_s_incl_call"] = time.perf_counter() - t0
        print(name, json.dumps(record), flush=True)
    four = {f"m{k}": torch.from_numpy(images["noisy"] * (1.0 + 0.25 * k)).cuda() for k in range(4)}
    report = {}
    for label, kwargs in (("plain", {}), ("four_modalities", dict(texture=four, texture_bins=args.bins))):
        measure.tumour_report(dev, **kwargs)
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            measure.tumour_report(dev, **kwargs)
            times.append(time.perf_counter() - t0)
        report[label] = {"s_median_of_5": float(np.median(times)), "min": min(times), "max": max(times)}
    result["tumour_report"] = report
    print(json.dumps(report), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
