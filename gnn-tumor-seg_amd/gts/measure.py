"""How much tumour, where, and how big each lesion is: per-lesion volumes, boxes, centroids, face counts, the
largest 3-D diameter and an in-plane bidimensional measurement of a label volume, on the device (M1-M4,
csrc/gts_measure.hip; definitions: DESIGN.md 4y).

A lesion is a connected component (connectivity 6 or 26) of a region's mask (WT, CT or ET); lesions are listed by
ascending root, 1 + the smallest C-order index, as gts.components gives it.  Points are voxel centres.  The spacing
is taken as integer units (u_x, u_y, u_z) and a scale in mm by gts.metrics.spacing_units; every device quantity is
an exact int64:

    n, n_class[1..3], box (begin, end per axis), coord_sum S_a, faces F_a (voxel faces towards the outside of the
    region mask or of the volume), d3 = max over voxel pairs of sum_a u_a^2 d_a^2, and on the planes of constant
    last axis z (the axial plane of the BraTS / conformed frame) plane_d2 = the largest in-plane squared distance
    of the slice z* = plane_z and plane_w = the largest caliper width perpendicular to a pair that reaches it,
    times that distance: exactly (major diameter) x (perpendicular width) in units^2.  z* is the smallest z with
    the largest W_z.  The footprint is the lesion's whole cross-section in the slice, connected or not; distances
    are centre to centre, so a one-pixel footprint measures 0.  This is a definition in the spirit of RANO's
    bidimensional product, not an implementation of any reader's protocol.

The float64 quantities are derived on the host, each by one fixed expression (`derive`).  Labels are internal: 0
healthy, 1 edema, 2 NET, 3 ET.  Everything runs on the current stream.
"""
import math

import numpy as np
import torch

from . import _lib, _volume
from ._lesions import REGIONS, RegionLesions, grid_arg, table_head
from ._lib import check, current_stream, ptr

HEAD_I64 = _lib.const("GTS_MEASURE_HEAD_I64")
ROW_I64 = _lib.const("GTS_MEASURE_ROW_I64")
PAIR_TILE = _lib.const("GTS_MEASURE_PAIR_TILE")
LIMITS = "every extent in [1, 4097], fewer than 2^31 voxels, 2 * sum_a u_a^2 (N_a - 1)^2 < 2^62"
TABLE_KEYS = ("root", "n", "n_class", "box", "coord_sum", "faces", "d3", "plane_z", "plane_d2", "plane_w")


def _work_units(rows, z_extent):
    """The host's plan from the table's rows (in arrival order): M3's (row, tile i, tile j >= i) over every list of
    at least two candidates, and M4's (row, slice of the box), both int32."""
    tiles = -(-rows[:, 17] // PAIR_TILE)
    tiles[rows[:, 17] < 2] = 0                      # a lone voxel: D3 stays 0
    single = np.flatnonzero(tiles == 1)
    pairs = [np.stack([single, np.zeros_like(single), np.zeros_like(single)], axis=1)]
    for s in np.flatnonzero(tiles > 1):
        i, j = np.triu_indices(int(tiles[s]))
        pairs.append(np.stack([np.full_like(i, s), i, j], axis=1))
    pairs = np.concatenate(pairs).astype(np.int32)
    slots = np.repeat(np.arange(len(rows)), z_extent)
    first = np.cumsum(z_extent) - z_extent
    planes = np.stack([slots, np.arange(len(slots)) - first[slots]], axis=1).astype(np.int32)
    return pairs, planes


def lesion_table(labels, region, spacing_mm=(1, 1, 1), connectivity=26, *, grid_blocks=0, mark=None):
    """The integer measurements of one region's lesions: a dict of numpy int64 arrays in lesion order (ascending
    root), root [L], n [L], n_class [L, 3] (labels 1, 2, 3), box [L, 6] (begin and end per axis), coord_sum [L, 3],
    faces [L, 3], d3, plane_z, plane_d2, plane_w [L] as the module's docstring defines them, and candidates [L],
    the hull-vertex candidates the 3-D diameter was taken over; `units` (u_x, u_y, u_z) and `scale_mm` as
    gts.metrics.spacing_units gives them, and plane_candidates, the in-plane candidates of all slices together.

    labels: int16 CUDA tensor [X, Y, Z] of internal labels; region "WT", "CT" or "ET" (or 0..2).  One copy of the
    table comes to the host for the plan of the pairwise work and one for the results.  grid_blocks: workgroups of
    every pass (0: the library's choice); no value depends on it.  mark: called with a stage's name once the stage
    is enqueued (tools/measure_lesion_shape.py records an event there)."""
    what = "lesion_table"
    grid_blocks = grid_arg(grid_blocks, what)
    return _table(RegionLesions(labels, region, spacing_mm, connectivity, what, LIMITS, mark), grid_blocks)


def _table(front, grid_blocks=0):
    """lesion_table's own stages, M1-M4, on a front end."""
    lib, labels, roots, c_units, (x, y, z) = front.lib, front.labels, front.roots, front.c_units, front.shape
    workspace, size = _volume.workspace(lib.gts_measure_workspace, x, y, z, labels.device, "lesion_table", LIMITS)
    ints = lib.gts_measure_table_i64s(x, y, z, front.connectivity)
    table = torch.empty(ints, dtype=torch.int64, device=labels.device)
    stream = current_stream()
    check(lib.gts_measure_tables_i16(ptr(labels), ptr(roots), x, y, z, front.region, front.connectivity, ptr(table),
                                     ints, ptr(workspace), size, grid_blocks, stream), "gts_measure_tables_i16")
    front.mark("M1 tables")
    check(lib.gts_measure_candidates(ptr(roots), x, y, z, ptr(table), ints, ptr(workspace), size, grid_blocks, stream),
          "gts_measure_candidates")
    front.mark("M2 candidates")
    head = table_head(table, lambda head: HEAD_I64 + ROW_I64 * int(head[0]))
    n_lesions, n_slices, plane_candidates = int(head[0]), int(head[1]), int(head[3])
    rows = head[HEAD_I64:].reshape(n_lesions, ROW_I64)
    if n_lesions:
        pairs, planes = _work_units(rows, rows[:, 9] + rows[:, 10] - z)
        work = torch.from_numpy(np.concatenate([pairs.ravel(), planes.ravel()])).to(labels.device)
        slices = torch.empty(2 * n_slices, dtype=torch.int64, device=labels.device)
        front.mark("plan (copy, host, upload)")
        check(lib.gts_measure_diameters(x, y, z, c_units, ptr(work), len(pairs), ptr(table), ints, ptr(workspace),
                                        size, grid_blocks, stream), "gts_measure_diameters")
        front.mark("M3 diameters")
        check(lib.gts_measure_planes(x, y, z, c_units, work.data_ptr() + 4 * pairs.size, len(planes), ptr(slices),
                                     n_slices, ptr(table), ints, ptr(workspace), size, grid_blocks, stream),
              "gts_measure_planes")
        front.mark("M4 planes")
        rows = table[HEAD_I64:head.size].cpu().numpy().reshape(n_lesions, ROW_I64)
        front.mark("results (copy)")
    rows = rows[np.argsort(rows[:, 0])]
    extent = np.array([x, x, y, y, z, z], dtype=np.int64)
    box = rows[:, 5:11].copy()
    box[:, 1::2] = extent[1::2] - box[:, 1::2]          # max(N - c) -> begin
    box = box[:, [1, 0, 3, 2, 5, 4]]                    # (begin, end) per axis
    return dict(root=rows[:, 0].copy(), n=rows[:, 1].copy(), n_class=rows[:, 2:5].copy(), box=box,
                coord_sum=rows[:, 11:14].copy(), faces=rows[:, 14:17].copy(), d3=rows[:, 20].copy(),
                plane_z=rows[:, 21].copy(), plane_d2=rows[:, 22].copy(), plane_w=rows[:, 23].copy(),
                candidates=rows[:, 17].copy(), plane_candidates=plane_candidates, units=tuple(front.units),
                scale_mm=front.scale_mm)


def volume_ml(voxels, units, scale_mm):
    """float(voxels * u_x * u_y * u_z) * scale^3 / 1000."""
    return float(int(voxels) * units[0] * units[1] * units[2]) * (scale_mm * scale_mm * scale_mm) / 1000.0


def derive(table, k):
    """The float64 quantities of lesion k of a lesion_table, each one fixed expression over Python integers, with
    s = scale_mm and u = units:

        volume_mm3        float(n u_x u_y u_z) * (s * s * s)          volume_ml       volume_mm3 / 1000.0
        centroid_voxel_a  S_a / n                                      centroid_mm_a   (S_a u_a) / n * s
        extent_mm_a       float((end_a - begin_a) u_a) * s
        face_area_mm2     float(F_x u_y u_z + F_y u_x u_z + F_z u_x u_y) * (s * s); it counts voxel faces, a staircase,
                          and so overestimates a smooth surface (by up to a factor of about 1.5 on a sphere)
        diameter_mm       sqrt(d3) * s
        plane_major_mm    sqrt(plane_d2) * s          plane_minor_mm   plane_w / sqrt(plane_d2) * s (0.0 at plane_d2 0)
        plane_product_mm2 float(plane_w) * (s * s)

    with the integers root, n, n_class, box, plane_z beside them."""
    u, s = table["units"], table["scale_mm"]
    n = int(table["n"][k])
    box = [int(v) for v in table["box"][k]]
    sums = [int(v) for v in table["coord_sum"][k]]
    faces = [int(v) for v in table["faces"][k]]
    d3, d2, w = int(table["d3"][k]), int(table["plane_d2"][k]), int(table["plane_w"][k])
    volume_mm3 = float(n * u[0] * u[1] * u[2]) * (s * s * s)
    return dict(root=int(table["root"][k]), n=n, n_class=[int(v) for v in table["n_class"][k]], box=box,
                volume_mm3=volume_mm3, volume_ml=volume_mm3 / 1000.0,
                class_ml=[float(int(c) * u[0] * u[1] * u[2]) * (s * s * s) / 1000.0 for c in table["n_class"][k]],
                centroid_voxel=[sums[a] / n for a in range(3)],
                centroid_mm=[(sums[a] * u[a]) / n * s for a in range(3)],
                extent_mm=[float((box[2 * a + 1] - box[2 * a]) * u[a]) * s for a in range(3)],
                face_area_mm2=float(faces[0] * u[1] * u[2] + faces[1] * u[0] * u[2] + faces[2] * u[0] * u[1]) * (s * s),
                diameter_mm=math.sqrt(d3) * s, plane_z=int(table["plane_z"][k]),
                plane_major_mm=math.sqrt(d2) * s, plane_minor_mm=w / math.sqrt(d2) * s if d2 else 0.0,
                plane_product_mm2=float(w) * (s * s))


def lesion_measurements(labels, region, spacing_mm=(1, 1, 1), connectivity=26, *, grid_blocks=0):
    """lesion_table's lesions as a list of dicts in lesion order, each with the float64 quantities of `derive`."""
    table = lesion_table(labels, region, spacing_mm, connectivity, grid_blocks=grid_blocks)
    return [derive(table, k) for k in range(len(table["root"]))]


def report_from_table(table, min_lesion_voxels=1, features=None, texture=None):
    """One region's part of tumour_report from its lesion_table.  features: gts.mesh.shape_features of the same
    region in lesion order; each listed lesion then carries its keys too.  texture: {name: {root: the features of
    gts.texture.derive}} over the listed lesions; each then carries `texture`, {name: features}."""
    u, s = table["units"], table["scale_mm"]
    voxels = int(table["n"].sum())
    classes = [int(v) for v in table["n_class"].sum(axis=0)] if len(table["n"]) else [0, 0, 0]
    order = sorted(range(len(table["n"])), key=lambda k: (-int(table["n"][k]), int(table["root"][k])))
    return dict(voxels=voxels, ml=volume_ml(voxels, u, s), class_ml=[volume_ml(c, u, s) for c in classes],
                n_lesions=len(order),
                lesions=[dict(derive(table, k), **(features[k] if features is not None else {}),
                              **({"texture": {name: by_root[int(table["root"][k])] for name, by_root in texture.items()}}
                                 if texture is not None else {}))
                         for k in order if int(table["n"][k]) >= min_lesion_voxels])


def tumour_report(labels, spacing_mm=(1, 1, 1), connectivity=26, min_lesion_voxels=1, *, mesh=False,
                  smooth_iterations=20, meshes=None, texture=None, texture_bins=32, texture_bin_width=None,
                  texture_matrices=(), texture_dependence_alpha=0):
    """{"WT" | "CT" | "ET": record}: voxels and ml of the region, class_ml (the region's voxels of label 1, 2, 3 in
    ml), n_lesions, and `lesions`, the dicts of `derive` sorted by descending n, then root.  A lesion of fewer than
    min_lesion_voxels voxels is counted in the totals and in n_lesions but not listed.

    mesh=True: each listed lesion also carries gts.mesh.shape_features' keys (the triangle surface of DESIGN.md 4z
    after smooth_iterations Taubin iterations); meshes, a dict, then receives every region's gts.mesh.region_mesh.

    texture={name: image}: int16 or float32 tensors of labels' shape, one per modality; each listed lesion also carries
    texture[name], gts.texture.derive's features of that lesion on that image without `root` and `n`,
    at texture_bins levels or, when given, at a bin width of texture_bin_width.  texture_matrices, a subset of
    gts.texture.MATRICES, and texture_dependence_alpha go to the texture call as `matrices` and `dependence_alpha`:
    texture[name] then also carries the features of those families.  They need `texture`."""
    if texture is not None or texture_matrices:
        from . import texture as gts_texture

        if texture is None:
            raise _lib.GtsError("tumour_report: texture_matrices needs texture")
        binning = gts_texture.binning_args(texture_bins, texture_bin_width, "tumour_report")
        families = gts_texture.matrices_arg(texture_matrices, texture_dependence_alpha, "tumour_report")
    report = {}
    for name in REGIONS:
        front = RegionLesions(labels, name, spacing_mm, connectivity, "lesion_table", LIMITS)
        table = _table(front)
        features = None
        if mesh:       # the same roots under both tables: one region mask and one labelling per region
            from . import mesh as gts_mesh

            surface = gts_mesh._mesh(front, gts_mesh.iterations_arg(smooth_iterations))
            if not np.array_equal(surface["root"], table["root"]):
                raise _lib.GtsError(f"tumour_report: the mesh and the table of {name} list different lesions")
            features = gts_mesh.shape_features(surface)
            if meshes is not None:
                meshes[name] = surface
        by_image = None
        if texture is not None:    # the same roots again: the lesions of a region are labelled once
            by_image = {}
            for key, image in texture.items():
                tex = gts_texture._texture(front, image, *binning, max(1, min_lesion_voxels), 0, *families)
                rows = [gts_texture.derive(tex, k) for k in range(len(tex["root"]))]
                by_image[key] = {row.pop("root"): row for row in rows if row.pop("n")}
        report[name] = report_from_table(table, min_lesion_voxels, features, by_image)
    return report
