"""The measurement kernels (gts.measure, M1-M4) on a BraTS-size synthetic prediction, stage by stage,
and the same report on the host.

    python tools/measure_lesion_shape.py --out profiles/measure/measure.json [--reps 10]
    python tools/measure_lesion_shape.py --host-only --out profiles/measure/host.json          # no GPU

The prediction (240 x 240 x 155, 1 mm): one tumour of about 100 ml, nested ellipsoids with the centres offset
(edema around an enhancing rim around a core), and 36 small islands.  Stage times are HIP events recorded where
gts.measure.lesion_table has enqueued each stage of the whole-tumour region: a stage is one to four launches, the
plan stage a copy of the table to the host, the host's plan and its upload.  The whole report is a host clock around
gts.measure.tumour_report (three regions), ending in its last copy.  Beside them: the sizes of the candidate lists
against the border voxels (voxels with an exposed face), the number of pairs M3 takes, and the same report on the
host: scipy's label, numpy per lesion over its box, and the same hull-vertex pruning before the pairwise step
(unpruned numpy would not finish).  The device tables are checked against that route before anything is timed.  The
parent commit has no such feature; the host route stands in for it.  No time is a pass criterion.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from tests import measure_ref as R  # noqa: E402

SHAPE = (240, 240, 155)
KEYS = ("root", "n", "n_class", "box", "coord_sum", "faces", "d3", "plane_z", "plane_d2", "plane_w")


def make_prediction(seed, shape=SHAPE, islands=36):
    """int16 internal labels: the tumour and `islands` small ellipsoids of one random label each."""
    rng = np.random.default_rng(seed)
    grid = np.ogrid[:shape[0], :shape[1], :shape[2]]
    labels = np.zeros(shape, dtype=np.int16)

    def ellipsoid(centre, radii):
        return sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radii)) <= 1.0

    centre = np.array([118.0, 131.0, 77.0])
    labels[ellipsoid(centre, (33.0, 28.5, 25.5))] = 1
    labels[ellipsoid(centre + (4, -3, 2), (19.0, 17.0, 15.0))] = 3
    labels[ellipsoid(centre + (5, -3, 2), (14.0, 12.5, 11.0))] = 2
    for _ in range(islands):
        c = [rng.uniform(12, n - 12) for n in shape]
        blob = ellipsoid(c, rng.uniform(0.8, 4.5, 3)) & (labels == 0)
        labels[blob] = rng.integers(1, 4)
    return labels


def _shifted(mask, axis, step):
    """mask's neighbour at `step` along `axis`, False outside."""
    out = np.zeros_like(mask)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[axis], dst[axis] = (slice(1, None), slice(None, -1)) if step > 0 else (slice(None, -1), slice(1, None))
    out[tuple(dst)] = mask[tuple(src)]
    return out


def host_table(labels, region, units, connectivity=26):
    """gts.measure.lesion_table's integers by scipy and numpy, lesion by lesion over its box, with the kernels'
    hull-vertex pruning before the pairwise steps; also the candidate and border counts."""
    from scipy import ndimage

    mask = R.region_mask(labels, region)
    lab, _ = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1))
    u = np.array(units, dtype=np.int64)
    out = {k: [] for k in KEYS + ("candidates", "plane_candidates", "border")}
    for k, box in enumerate(ndimage.find_objects(lab), 1):
        m = lab[box] == k
        origin = np.array([s.start for s in box], dtype=np.int64)
        pts = np.argwhere(m).astype(np.int64) + origin
        values = labels[box][m]
        both = [_shifted(m, a, -1) & _shifted(m, a, 1) for a in range(3)]
        faces = []
        for a in range(3):
            lo, hi = _neighbour(mask, box, a, -1), _neighbour(mask, box, a, 1)
            faces.append(int((m & ~lo).sum() + (m & ~hi).sum()))
        border = m & ~np.logical_and.reduce([_neighbour(mask, box, a, s) for a in range(3) for s in (-1, 1)])
        cand3 = np.argwhere(m & ~both[0] & ~both[1] & ~both[2]).astype(np.int64) + origin
        cand2 = m & ~both[0] & ~both[1]
        best = None
        for dz in range(m.shape[2]):
            foot = (np.argwhere(cand2[:, :, dz]).astype(np.int64) + origin[:2]) * u[:2]
            d2, w, _ = R.plane_measure(foot)
            if best is None or w > best[2]:
                best = (int(origin[2]) + dz, d2, w)
        out["root"].append(1 + int(np.ravel_multi_index(tuple(pts[0]), labels.shape)))
        out["n"].append(len(pts))
        out["n_class"].append([int((values == c).sum()) for c in (1, 2, 3)])
        out["box"].append([v for s in box for v in (s.start, s.stop)])
        out["coord_sum"].append(pts.sum(axis=0).tolist())
        out["faces"].append(faces)
        out["d3"].append(R.diameter2(cand3 * u))
        out["plane_z"].append(best[0])
        out["plane_d2"].append(best[1])
        out["plane_w"].append(best[2])
        out["candidates"].append(len(cand3))
        out["plane_candidates"].append(int(cand2.sum()))
        out["border"].append(int(border.sum()))
    return {k: np.array(v, dtype=np.int64) for k, v in out.items()}


def _neighbour(mask, box, axis, step):
    """Over the lesion's box: whether the voxel at `step` along `axis` is in the region mask (False outside the
    volume)."""
    shape = tuple(s.stop - s.start for s in box)
    out = np.zeros(shape, dtype=bool)
    lo, hi = box[axis].start + step, box[axis].stop + step
    cut_lo, cut_hi = max(lo, 0), min(hi, mask.shape[axis])
    src, dst = list(box), [slice(None)] * 3
    src[axis] = slice(cut_lo, cut_hi)
    dst[axis] = slice(cut_lo - lo, shape[axis] - (hi - cut_hi))
    out[tuple(dst)] = mask[tuple(src)]
    return out


def host_report(labels, units):
    clock, tables = {}, {}
    for region in R.REGIONS:
        t0 = time.perf_counter()
        tables[region] = host_table(labels, region, units)
        clock[region] = time.perf_counter() - t0
    clock["whole"] = sum(clock.values())
    return clock, tables


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "measure", "measure.json"))
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--host-only", action="store_true", help="only the scipy / numpy route on the host (no GPU)")
    parser.add_argument("--seed", type=int, default=0, help="of the prediction")
    parser.add_argument("--shape", type=int, nargs=3, default=list(SHAPE), help="for a rehearsal at a small size")
    args = parser.parse_args()
    shape = tuple(args.shape)
    labels = make_prediction(args.seed) if shape == SHAPE else np.ascontiguousarray(
        make_prediction(args.seed)[tuple(slice((n - s) // 2, (n - s) // 2 + s) for n, s in zip(SHAPE, shape))])
    units = (1, 1, 1)
    result = {"volume": list(shape), "seed": args.seed, "spacing_mm": [1, 1, 1],
              "voxels_per_label": [int((labels == c).sum()) for c in (1, 2, 3)]}
    clock, host = host_report(labels, units)
    result["host_scipy_numpy_s"] = clock
    wt = host["WT"]
    big = int(wt["n"].argmax())
    result["whole_tumour"] = {
        "lesions": len(wt["n"]), "largest_voxels": int(wt["n"][big]), "largest_border_voxels": int(wt["border"][big]),
        "largest_candidates_3d": int(wt["candidates"][big]),
        "largest_pairs_3d": int(wt["candidates"][big]) * (int(wt["candidates"][big]) + 1) // 2,
        "largest_plane_candidates": int(wt["plane_candidates"][big]),
        "largest_slices": int(wt["box"][big][5] - wt["box"][big][4]),
        "border_voxels_all": int(wt["border"].sum()), "candidates_3d_all": int(wt["candidates"].sum()),
        "plane_candidates_all": int(wt["plane_candidates"].sum()),
        "largest": {k: wt[k][big].tolist() for k in KEYS}}
    print(json.dumps({k: result[k] for k in ("host_scipy_numpy_s", "whole_tumour")}), flush=True)
    if not args.host_only:
        import torch

        from gts import _lib, measure

        _lib.load()
        result["device"] = torch.cuda.get_device_name(0)
        result["reps"] = args.reps
        dev = torch.from_numpy(labels).cuda()
        for region in R.REGIONS:                     # the device's integers are the host route's, in every field
            got = measure.lesion_table(dev, region)
            for key in KEYS + ("candidates",):
                assert np.array_equal(got[key], host[region][key]), (region, key)
            assert got["plane_candidates"] == int(host[region]["plane_candidates"].sum()), region
        result["device_equals_host_route"] = True
        stages = {}
        for rep in range(3 + args.reps):
            events = []

            def mark(stage):
                event = torch.cuda.Event(enable_timing=True)
                event.record()
                events.append((stage, event))

            mark("start")
            measure.lesion_table(dev, "WT", mark=mark)
            torch.cuda.synchronize()
            if rep >= 3:
                for (_, before), (stage, after) in zip(events, events[1:]):
                    stages.setdefault(stage, []).append(before.elapsed_time(after))
        rows = [{"stage": s, "ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}
                for s, t in stages.items()]
        total = sum(r["ms"] for r in rows)
        m3 = next(r["ms"] for r in rows if r["stage"].startswith("M3"))
        result["stages_whole_tumour"] = rows
        result["stages_sum_ms"] = total
        result["m3_longer_than_the_rest"] = bool(m3 > total - m3)
        for row in rows:
            print(json.dumps(row), flush=True)
        measure.tumour_report(dev)
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            report = measure.tumour_report(dev)
            times.append(time.perf_counter() - t0)
        result["tumour_report"] = {"gpu_s_median_of_5": float(np.median(times)), "gpu_s_all": times,
                                   "largest_wt_lesion": report["WT"]["lesions"][0]}
        print(json.dumps(result["tumour_report"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
