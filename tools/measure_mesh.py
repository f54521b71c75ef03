"""The mesh kernels (gts.mesh, T1-T5) on the BraTS-size synthetic prediction of
tools/measure_lesion_shape.py, stage by stage, and the area ratios on analytic balls.

    python tools/measure_mesh.py --out profiles/mesh/mesh.json [--reps 10]
    python tools/measure_mesh.py --host-only --out profiles/mesh/host.json          # no GPU

Stage times are HIP events recorded where gts.mesh.region_mesh has enqueued each stage of the whole-tumour region
(a stage is one to six launches; the table stage a copy of the table's head to the host).  Beside them: triangles and
vertices, the bytes each stage has to move at least (compulsory bytes: every input read once, every output written
once), and for the classify pass the fraction of the 8 TB/s HBM peak those bytes are.  The whole call is a host clock
around region_mesh, ending in a synchronize.  The parent commit has no such feature; the host stand-in is the
vectorised numpy route below (scipy's label, the 16-case rule applied to all cells of one case at once, no smoothing,
no ordering), checked against the device's integer table.  It is a stand-in, not a baseline.  No time is a pass
criterion.

The balls x^2 + y^2 + z^2 <= R^2 (R = 8 and 12, unit spacing) give area / 4 pi R^2 for the voxel-face count, the raw
mesh and the mesh after 20 Taubin iterations, by tests/mesh_ref.py on the host and, with a GPU, by the device.
Agreement with pyradiomics or IBSI values is unknown, and nothing here was run on real anatomy.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd"), os.path.join(REPO, "tools")]

from tests import measure_ref  # noqa: E402
from tests import mesh_ref  # noqa: E402

HBM_PEAK = 8.0e12


def numpy_table(labels, region, connectivity=26):
    """The integer table by vectorised numpy: per tetrahedron type the inside counts of all cells at once; triangles
    = (0, 1, 2, 1, 0)[count], 48 x volume = (0, 1, 4, 7, 8)[count], the lesion from the smallest root among the inside
    corners (scipy's label).  Class counts are left out: they need the triangles themselves."""
    mask = measure_ref.region_mask(labels, region)
    roots = mesh_ref.lesion_roots(mask, connectivity)
    pad = np.pad(mask, 1)
    big = np.iinfo(np.int64).max
    plab = np.pad(np.where(mask, roots, big), 1, constant_values=big)
    shape = tuple(n + 1 for n in mask.shape)
    tris, v48 = {}, {}
    for path in mesh_ref.PATHS:
        views = [tuple(slice(p[a], p[a] + shape[a]) for a in range(3)) for p in path]
        count = sum(pad[v].astype(np.int8) for v in views)
        root = np.minimum.reduce([plab[v] for v in views])
        active = (count > 0) & (count < 4)
        r = root[active]
        c = count[active]
        order = np.unique(r, return_inverse=True)
        t = np.bincount(order[1], weights=np.array([0, 1, 2, 1, 0])[c], minlength=len(order[0]))
        full = (count > 0)
        r_all, c_all = root[full], count[full]
        order_all = np.unique(r_all, return_inverse=True)
        v = np.bincount(order_all[1], weights=np.array([0, 1, 4, 7, 8])[c_all], minlength=len(order_all[0]))
        for key, val in zip(order[0].tolist(), t.tolist()):
            tris[key] = tris.get(key, 0) + int(val)
        for key, val in zip(order_all[0].tolist(), v.tolist()):
            v48[key] = v48.get(key, 0) + int(val)
    keys = sorted(tris)
    return dict(root=np.array(keys, dtype=np.int64), triangles=np.array([tris[k] for k in keys], dtype=np.int64),
                v6=np.array([v48[k] for k in keys], dtype=np.int64))


def ball_ratios(radius, device):
    size = 2 * radius + 5
    mask = mesh_ref.ball(radius * radius, size)
    sphere = 4.0 * math.pi * radius * radius
    vertices, faces, roots = mesh_ref.surface(mask)
    table = mesh_ref.integer_table(vertices, faces, roots)
    rows = mesh_ref.neighbours(faces, len(vertices))
    start = mesh_ref.positions_mm(vertices, (1, 1, 1), 1.0)
    area, volume = mesh_ref.face_terms(mesh_ref.smooth(start, rows, 20), faces)
    pairs = int((mask[1:] & mask[:-1]).sum() + (mask[:, 1:] & mask[:, :-1]).sum() + (mask[:, :, 1:] & mask[:, :, :-1]).sum())
    faces_count = 6 * int(mask.sum()) - 2 * pairs          # gts.measure's face_area_mm2 at unit spacing
    out = {"radius": radius, "voxels": int(mask.sum()), "triangles": len(faces), "vertices": len(vertices),
           "degree_min_max": [min(map(len, rows)), max(map(len, rows))],
           "face_count_over_sphere": float(faces_count) / sphere,
           "raw_mesh_over_sphere": mesh_ref.raw_area_mm2(table["classes"][0], (1, 1, 1), 1.0) / sphere,
           "smoothed_20_over_sphere": math.fsum(area) / sphere,
           "raw_volume_voxels": int(table["v6"][0]) / 48.0, "smoothed_volume_voxels": math.fsum(volume),
           "volume_change": math.fsum(volume) / (int(table["v6"][0]) / 48.0) - 1.0, "by": "tests/mesh_ref.py (host)"}
    if device:
        import torch

        from gts import mesh

        got = mesh.region_mesh(torch.from_numpy(np.where(mask, 3, 0).astype(np.int16)).cuda(), "WT")
        (f,) = mesh.shape_features(got)
        out["device"] = {"raw_mesh_over_sphere": f["mesh_area_mm2"] / sphere,
                         "smoothed_20_over_sphere": f["smooth_area_mm2"] / sphere, "sphericity": f["sphericity"],
                         "positions_equal_host_bits": bool(np.array_equal(got["vertices_mm"].cpu().numpy(),
                                                                          mesh_ref.smooth(start, rows, 20)))}
    return out


def main():
    from measure_lesion_shape import SHAPE, make_prediction

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh", "mesh.json"))
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--host-only", action="store_true", help="only the numpy stand-in and the balls (no GPU)")
    parser.add_argument("--seed", type=int, default=0, help="of the prediction")
    parser.add_argument("--shape", type=int, nargs=3, default=list(SHAPE), help="for a rehearsal at a small size")
    args = parser.parse_args()
    shape = tuple(args.shape)
    labels = make_prediction(args.seed) if shape == SHAPE else np.ascontiguousarray(
        make_prediction(args.seed)[tuple(slice((n - s) // 2, (n - s) // 2 + s) for n, s in zip(SHAPE, shape))])
    result = {"volume": list(shape), "seed": args.seed, "spacing_mm": [1, 1, 1],
              "cells": int(np.prod([n + 1 for n in shape]))}
    t0 = time.perf_counter()
    host = numpy_table(labels, "WT")
    result["host_numpy_stand_in_s"] = time.perf_counter() - t0
    result["host_numpy_stand_in_is"] = "scipy label + the 16-case counts over whole arrays; no vertices, faces or smoothing"
    result["balls"] = [ball_ratios(r, not args.host_only) for r in (8, 12)]
    print(json.dumps({k: result[k] for k in ("host_numpy_stand_in_s", "balls")}), flush=True)
    if not args.host_only:
        import torch

        from gts import _lib, mesh

        _lib.load()
        result["device"] = torch.cuda.get_device_name(0)
        result["reps"] = args.reps
        dev = torch.from_numpy(labels).cuda()
        got = mesh.region_mesh(dev, "WT")
        for key in ("root", "triangles", "v6"):
            assert np.array_equal(got[key], host[key]), key
        result["device_equals_numpy_stand_in"] = True
        n_v, n_f = got["vertices_half"].shape[0], got["faces"].shape[0]
        cells, voxels = result["cells"], int(np.prod(shape))
        result["whole_tumour"] = {"lesions": len(got["root"]), "vertices": n_v, "triangles": n_f,
                                  "largest": mesh.shape_features(got)[int(got["triangles"].argmax())]}
        # compulsory bytes: inputs read once, outputs written once
        bytes_of = {"T1-T2 classify, scans": 4 * voxels + 4 * voxels + cells + 16 * (cells // 256 + 1),
                    "T3 emit": 2 * cells + 4 * cells + 12 * n_v + 16 * n_f,
                    "T4 adjacency": 3 * (12 * n_f) + 8 * n_v + 2 * 12 * n_f,
                    "T5 smooth": 40 * (4 * n_v + 12 * n_f + 2 * 24 * n_v),
                    "T5 terms": 24 * n_v + 12 * n_f + 16 * n_f}
        stages = {}
        for rep in range(3 + args.reps):
            events = []

            def mark(stage):
                event = torch.cuda.Event(enable_timing=True)
                event.record()
                events.append((stage, event))

            mark("start")
            mesh.region_mesh(dev, "WT", mark=mark)
            torch.cuda.synchronize()
            if rep >= 3:
                for (_, before), (stage, after) in zip(events, events[1:]):
                    stages.setdefault(stage, []).append(before.elapsed_time(after))
        rows = []
        for s, t in stages.items():
            row = {"stage": s, "ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
            if s in bytes_of:
                row["compulsory_bytes"] = int(bytes_of[s])
                row["fraction_of_hbm_peak"] = bytes_of[s] / (row["ms"] * 1e-3) / HBM_PEAK
            rows.append(row)
            print(json.dumps(row), flush=True)
        result["stages_whole_tumour"] = rows
        result["stages_sum_ms"] = sum(r["ms"] for r in rows)
        result["smooth_20_iterations_ms"] = next(r["ms"] for r in rows if r["stage"] == "T5 smooth")
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh.region_mesh(dev, "WT")
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        result["region_mesh_s_median_of_5"] = float(np.median(times))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
