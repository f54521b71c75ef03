"""Written predictions -> how much tumour there is, where, and how big each lesion is, on the MI355X.

Every {id}.nii.gz in PRED_DIR, as segment_scans and the two generate_* scripts write it, is decoded, mapped to the
internal labels and measured per region (WT, CT, ET) by gts.measure.tumour_report (definitions: DESIGN.md 4y): per
lesion the volume in ml, the centroid and extent in mm, the face-count area, the largest 3-D diameter and, on the
planes of constant last axis, the major diameter, the caliper width perpendicular to it and their product (in the
spirit of RANO's bidimensional product; not a reader's protocol).  Files may hold {0, 1, 2, 4} or the 2023
convention {0, 1, 2, 3}; a file with both 3 and 4, or any other value, is refused.  The voxel spacing is read from
each file's own affine (its column norms).

One CSV row per (scan, region, lesion), the lesions of a region by descending size, and one `total` row per (scan,
region); --json writes the whole report as well.  The GPU takes one scan at a time while a small thread pool decodes
the next ones.  A file that cannot be measured is reported and left out; the exit status is then 1.

--mesh adds the triangle surface of every region (gts.mesh): the columns of MESH_HEADER after the
existing ones (raw mesh area and volume, the same after --mesh_smooth Taubin iterations, sphericity, surface to
volume), and with --mesh_dir DIR a binary PLY per (scan, region), DIR/{id}_{region}.ply, in the world coordinates of
the file's own affine.  Without --mesh the CSV and the JSON are what they were.

--texture SCAN_DIR adds what the tissue inside each lesion looks like on the scans (gts.texture): per
modality of --texture_modalities the columns tex_{modality}_{feature} over TEXTURE_FEATURES (first-order and GLCM
features at --texture_bins grey levels, or at a bin width of --texture_bin_width), after the mesh columns.  The scan
of {id}.nii.gz is the folder {id} under SCAN_DIR, each modality the first file directly in it that ends with the
extension; a scan with a modality that is missing, of another shape than the prediction or on another grid (affines
more than gts.conform.AFFINE_AGREEMENT apart) is reported and left out.  Without --texture the CSV and the JSON are
what they were.

--texture_matrices NAME [NAME ...] (with --texture; glrlm, glszm, gldm, ngtdm or all) adds the features of the
run-length, size-zone, dependence and neighbourhood-difference families (gts.texture.GLRLM_KEYS and
its siblings; --texture_dependence_alpha A is the GLDM's level tolerance, default 0): the columns
tex_{modality}_{key} after all the columns above, by modality and then by family.  Without it the CSV and the JSON of
--texture are what they were.

    python -m scripts.measure_tumours -s PRED_DIR -o report.csv --json report.json --min_lesion_voxels 10
    python -m scripts.measure_tumours -s PRED_DIR -o report.csv --mesh --mesh_dir meshes
    python -m scripts.measure_tumours -s PRED_DIR -o report.csv --texture SCAN_DIR --texture_bins 32
    python -m scripts.measure_tumours -s PRED_DIR -o report.csv --texture SCAN_DIR --texture_matrices all
"""
import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import numpy as np  # noqa: E402

from data_processing import labels as label_maps  # noqa: E402
from data_processing import nifti_io  # noqa: E402
from scripts.score_predictions import IO_WORKERS, READ_AHEAD, spacing_of  # noqa: E402

REGIONS = ("WT", "CT", "ET")
SUFFIX = ".nii.gz"
HEADER = ["id", "region", "lesion", "n_lesions", "root", "voxels", "volume_ml", "ml_label1", "ml_label2", "ml_label3",
          "centroid_x_mm", "centroid_y_mm", "centroid_z_mm", "extent_x_mm", "extent_y_mm", "extent_z_mm",
          "face_area_mm2", "diameter_mm", "plane_z", "plane_major_mm", "plane_minor_mm", "plane_product_mm2"]
MESH_HEADER = ["mesh_triangles", "mesh_area_mm2", "mesh_volume_ml", "smooth_area_mm2", "smooth_volume_ml", "sphericity",
               "surface_to_volume_per_mm"]       # gts.mesh.FEATURE_KEYS, appended by --mesh
TEXTURE_MODALITIES = ["_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"]
TEXTURE_FEATURES = ["min", "max", "range", "levels", "mean_level", "variance", "skewness", "kurtosis", "median_level",
                    "p10_level", "p90_level", "mode_level", "entropy", "uniformity", "mean_intensity_approx",
                    "joint_maximum", "joint_average", "joint_variance", "joint_entropy", "difference_average",
                    "difference_variance", "difference_entropy", "sum_average", "sum_variance", "sum_entropy",
                    "angular_second_moment", "contrast", "dissimilarity", "inverse_difference",
                    "inverse_difference_moment", "correlation", "autocorrelation", "cluster_tendency", "cluster_shade",
                    "cluster_prominence", "information_correlation_1",
                    "information_correlation_2"]    # gts.texture.FEATURE_KEYS, per modality of --texture


def modality_name(extension):
    """The name of a modality in the columns and the JSON: its extension without the leading '_' and the file type."""
    name = extension[:-len(SUFFIX)] if extension.endswith(SUFFIX) else extension.split(".")[0]
    return name.lstrip("_") or extension


TEXTURE_MATRICES = ["glrlm", "glszm", "gldm", "ngtdm"]       # gts.texture.MATRICES, --texture_matrices


def matrix_features(matrices):
    """The feature names of the families of --texture_matrices, in TEXTURE_MATRICES' order."""
    from gts.texture import MATRIX_FEATURE_KEYS

    return [key for family in TEXTURE_MATRICES if family in matrices for key in MATRIX_FEATURE_KEYS[family]]


def texture_header(modalities, matrices=()):
    more = matrix_features(matrices) if matrices else []
    return [f"tex_{modality_name(ext)}_{key}" for ext in modalities for key in TEXTURE_FEATURES] + \
        [f"tex_{modality_name(ext)}_{key}" for ext in modalities for key in more]


def build_parser():
    parser = argparse.ArgumentParser(description="Per-lesion volumes, extents and diameters of written predictions on "
                                                 "MI355X")
    parser.add_argument("-s", "--pred_dir", required=True, help="folder holding the predictions, {id}.nii.gz")
    parser.add_argument("-o", "--output", required=True, help="the CSV file to write")
    parser.add_argument("--json", default=None, metavar="FILE", help="also write the whole report as JSON")
    parser.add_argument("--connectivity", type=int, default=26, choices=(6, 26),
                        help="voxels of one lesion are connected through faces (6) or faces, edges and corners (26)")
    parser.add_argument("--min_lesion_voxels", type=int, default=1,
                        help="a smaller lesion is counted in the totals but gets no row")
    parser.add_argument("--regions", nargs="+", default=list(REGIONS), choices=REGIONS, help="the regions to report")
    parser.add_argument("--mesh", action="store_true",
                        help="also mesh every region (marching tetrahedra) and append the shape columns")
    parser.add_argument("--mesh_smooth", type=int, default=20, metavar="N",
                        help="Taubin iterations before the smooth area, volume and sphericity (0: the raw mesh)")
    parser.add_argument("--mesh_dir", default=None, metavar="DIR",
                        help="with --mesh: write DIR/{id}_{region}.ply in each file's world coordinates")
    parser.add_argument("--texture", default=None, metavar="SCAN_DIR",
                        help="also report intensity and texture features of every lesion on the scans under SCAN_DIR "
                             "(the folder {id} of a prediction {id}.nii.gz)")
    parser.add_argument("--texture_modalities", nargs="+", default=list(TEXTURE_MODALITIES), metavar="EXT",
                        help="with --texture: file suffixes of the modalities to report")
    binning = parser.add_mutually_exclusive_group()
    binning.add_argument("--texture_bins", type=int, default=None, metavar="N",
                         help="with --texture: grey levels per lesion, a fixed bin number (default 32)")
    binning.add_argument("--texture_bin_width", type=float, default=None, metavar="W",
                         help="with --texture: a fixed bin width in the scan's units instead of a bin number")
    parser.add_argument("--texture_matrices", nargs="+", default=None, metavar="NAME",
                        choices=TEXTURE_MATRICES + ["all"],
                        help="with --texture: also report the features of these families (glrlm, glszm, gldm, ngtdm, "
                             "or all)")
    parser.add_argument("--texture_dependence_alpha", type=int, default=None, metavar="A",
                        help="with --texture_matrices: levels at most A apart count as dependent (GLDM; default 0)")
    return parser


def find_predictions(pred_dir):
    """{id: path} of every {id}.nii.gz directly in pred_dir."""
    return {f[:-len(SUFFIX)]: os.path.join(pred_dir, f) for f in sorted(os.listdir(pred_dir)) if f.endswith(SUFFIX)}


def load_prediction(path):
    """Host stage: (internal int16 labels, C-contiguous; spacing in mm)."""
    labels = label_maps.swap_labels_from_brats_any(nifti_io.read_nifti(path, np.int16))
    if labels.ndim != 3:
        raise ValueError(f"the label volume has {labels.ndim} axes, expected 3")
    return np.ascontiguousarray(labels), spacing_of(path)


def load_texture(path, shape, scan_dir, modalities):
    """Host stage of --texture: {modality name: the scan's volume as stored (int16 or float32), C-contiguous} of the
    prediction at `path`, every modality of the prediction's `shape` and on its grid."""
    from gts.conform import AFFINE_AGREEMENT

    scan_id = os.path.basename(path)[:-len(SUFFIX)]
    folder = os.path.join(scan_dir, scan_id)
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"no scan folder {folder}")
    affine, _ = nifti_io.read_affine(path)
    images = {}
    for ext in modalities:
        found = sorted(f for f in os.listdir(folder) if f.endswith(ext))
        if not found:
            raise FileNotFoundError(f"{folder}: no file ending with {ext!r}")
        file = os.path.join(folder, found[0])
        volume = nifti_io.read_nifti_raw(file)
        if volume.shape != shape:
            raise ValueError(f"{found[0]} {volume.shape} and the prediction {shape} differ in shape")
        gap = float(np.max(np.abs(nifti_io.read_affine(file)[0] - affine)))
        if not gap <= AFFINE_AGREEMENT:
            raise ValueError(f"the affines of {found[0]} and the prediction disagree by {gap:g} "
                             f"(limit {AFFINE_AGREEMENT:g})")
        images[modality_name(ext)] = np.ascontiguousarray(volume)
    return images


def _cell(value):
    return "" if value is None else repr(value) if isinstance(value, float) else str(value)


def rows_of(scan_id, report, regions=REGIONS, mesh=False, texture=(), matrices=()):
    """The CSV rows (lists of strings, HEADER's order) of one scan's tumour_report: per region its lesions in the
    report's order, numbered from 1, then the `total` row.  mesh: MESH_HEADER's columns after them (empty in the
    `total` row), from a report made with mesh=True.  texture: the modality names of a report made with texture=;
    TEXTURE_FEATURES' columns per modality after those (empty in the `total` row, and where a feature is None).
    matrices: the families of a report made with texture_matrices=; their columns per modality after all those."""
    rows = []
    more = matrix_features(matrices) if matrices else []
    extra = (len(MESH_HEADER) if mesh else 0) + len(texture) * (len(TEXTURE_FEATURES) + len(more))
    for region in regions:
        record = report[region]
        for rank, m in enumerate(record["lesions"], 1):
            rows.append([scan_id, region, rank, "", m["root"], m["n"], m["volume_ml"]] + m["class_ml"] +
                        m["centroid_mm"] + m["extent_mm"] +
                        [m["face_area_mm2"], m["diameter_mm"], m["plane_z"], m["plane_major_mm"], m["plane_minor_mm"],
                         m["plane_product_mm2"]] + ([m[key] for key in MESH_HEADER] if mesh else []) +
                        [m["texture"][name][key] for name in texture for key in TEXTURE_FEATURES] +
                        [m["texture"][name][key] for name in texture for key in more])
        rows.append([scan_id, region, "total", record["n_lesions"], "", record["voxels"], record["ml"]] +
                    record["class_ml"] + [""] * (12 + extra))
    return [[_cell(v) for v in row] for row in rows]


def write_csv(path, rows, mesh=False, texture=(), matrices=()):
    """texture: the extensions of --texture_modalities; matrices: the families of --texture_matrices."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(",".join(HEADER + (MESH_HEADER if mesh else []) + texture_header(texture, matrices)) + "\n")
        for row in rows:
            f.write(",".join(row) + "\n")


def measure(paths, connectivity=26, min_lesion_voxels=1, mesh=False, mesh_smooth=20, mesh_dir=None, regions=REGIONS,
            texture_dir=None, texture_modalities=(), texture_bins=32, texture_bin_width=None, texture_matrices=(),
            texture_dependence_alpha=0):
    """({id: {"spacing_mm", "regions": tumour_report}}, ids left out) of {id: path}.  mesh: the report carries the
    shape features; mesh_dir: the PLY files of `regions` go there.  texture_dir: the report carries the texture
    features of texture_modalities, the scans being decoded on the read-ahead pool beside the predictions, and those
    of the families of texture_matrices."""
    import torch

    from gts import measure as gts_measure

    if mesh and mesh_dir:
        from gts import mesh as gts_mesh

        os.makedirs(mesh_dir, exist_ok=True)

    def load(path):
        labels, spacing = load_prediction(path)
        return labels, spacing, (load_texture(path, labels.shape, texture_dir, texture_modalities)
                                 if texture_dir is not None else None)

    ids = sorted(paths)
    reports, failed = {}, []
    with ThreadPoolExecutor(max_workers=IO_WORKERS) as pool:
        pending = {i: pool.submit(load, paths[ids[i]]) for i in range(min(READ_AHEAD, len(ids)))}
        for i, scan_id in enumerate(ids):
            if i + READ_AHEAD < len(ids):
                pending[i + READ_AHEAD] = pool.submit(load, paths[ids[i + READ_AHEAD]])
            try:
                labels, spacing, images = pending.pop(i).result()
                options, meshes = {}, {}
                if mesh:
                    options.update(mesh=True, smooth_iterations=mesh_smooth, meshes=meshes)
                if images is not None:
                    options.update(texture={name: torch.from_numpy(v).cuda() for name, v in images.items()},
                                   texture_bins=texture_bins, texture_bin_width=texture_bin_width)
                    if texture_matrices:
                        options.update(texture_matrices=tuple(texture_matrices),
                                       texture_dependence_alpha=texture_dependence_alpha)
                report = gts_measure.tumour_report(torch.from_numpy(labels).cuda(), spacing, connectivity,
                                                   min_lesion_voxels, **options)
                if mesh and mesh_dir:
                    affine, _ = nifti_io.read_affine(paths[scan_id])
                    for region in regions:
                        gts_mesh.write_ply(os.path.join(mesh_dir, f"{scan_id}_{region}.ply"), meshes[region], affine)
                reports[scan_id] = dict(spacing_mm=list(spacing), regions=report)
            except Exception as exc:
                print(f"{scan_id}: left out ({exc!r})")
                failed.append(scan_id)
    return reports, failed


def main(argv=None):
    args = build_parser().parse_args(argv)
    paths = find_predictions(os.path.expanduser(args.pred_dir))
    print(f"{len(paths)} predictions found; the report goes to {args.output}")
    if args.mesh_dir and not args.mesh:
        raise SystemExit("--mesh_dir needs --mesh")
    if not args.texture and (args.texture_bins is not None or args.texture_bin_width is not None):
        raise SystemExit("--texture_bins and --texture_bin_width need --texture")
    if not args.texture and (args.texture_matrices is not None or args.texture_dependence_alpha is not None):
        raise SystemExit("--texture_matrices and --texture_dependence_alpha need --texture")
    if args.texture_dependence_alpha is not None and args.texture_dependence_alpha < 0:
        raise SystemExit("--texture_dependence_alpha: 0 or more")
    chosen = args.texture_matrices or []
    matrices = [m for m in TEXTURE_MATRICES if m in chosen or "all" in chosen]
    modalities = tuple(args.texture_modalities) if args.texture else ()
    names = [modality_name(ext) for ext in modalities]
    if len(set(names)) != len(names):
        raise SystemExit(f"--texture_modalities: {names} are not distinct names")
    reports, failed = measure(paths, args.connectivity, args.min_lesion_voxels, args.mesh, args.mesh_smooth,
                              os.path.expanduser(args.mesh_dir) if args.mesh_dir else None, args.regions,
                              os.path.expanduser(args.texture) if args.texture else None, modalities,
                              32 if args.texture_bins is None else args.texture_bins, args.texture_bin_width,
                              matrices, args.texture_dependence_alpha or 0)
    rows = [row for scan_id in sorted(reports)
            for row in rows_of(scan_id, reports[scan_id]["regions"], args.regions, args.mesh, names, matrices)]
    write_csv(os.path.expanduser(args.output), rows, args.mesh, modalities, matrices)
    if args.json:
        path = os.path.expanduser(args.json)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(reports, f, indent=1, sort_keys=True)
    for scan_id in sorted(reports):
        for region in args.regions:
            record = reports[scan_id]["regions"][region]
            largest = record["lesions"][0] if record["lesions"] else None
            print(f"{scan_id} {region}: {record['ml']:.2f} ml in {record['n_lesions']} lesion(s)" +
                  (f", the largest {largest['volume_ml']:.2f} ml, {largest['diameter_mm']:.1f} mm across, "
                   f"{largest['plane_major_mm']:.1f} x {largest['plane_minor_mm']:.1f} mm in slice {largest['plane_z']}"
                   if largest else ""))
    print(f"{len(reports)} prediction(s) measured, {len(failed)} left out")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
