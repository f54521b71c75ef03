"""Written predictions + ground truth -> legacy and lesion-wise BraTS scores, on the MI355X.

For each scan folder under DATA_DIR the label volume (the file ending with the label extension) and
PRED_DIR/{id}.nii.gz, as segment_scans and the two generate_* scripts write it, are decoded, mapped to the
internal labels and scored per region (WT, CT, ET) by gts.lesionwise.lesionwise_scores: the legacy whole-region
Dice and HD95, and the BraTS 2023 lesion-wise Dice and HD95 (definition, and how it deviates from the
challenge's script: DESIGN.md 4o).  Files may hold {0, 1, 2, 4} or the 2023 convention {0, 1, 2, 3}; a file with
both 3 and 4, or any other value, is refused.  Volumes are scored as stored: prediction and truth must share a
shape.

One CSV row per scan and a final `mean` row over the scans; the same means are printed.  The GPU takes one scan
at a time while a small thread pool decodes the next ones.  A scan whose prediction is missing, whose shape
differs from its truth or that raises is reported and left out; the exit status is 1 when any scan was left out.

    python -m scripts.score_predictions -d DATA_DIR -l _seg.nii.gz -s PRED_DIR -o scores.csv

--mm scores distances in millimetres: the voxel spacing is read from the ground-truth file's affine (its column
norms) and the whole-region and per-lesion HD95 come from gts.metrics' spacing-aware route; a scan
whose prediction has another spacing, in any step of 1e-4 mm, is left out.  --nsd_tolerance MM [MM ...] (at most
4, implies --mm) appends the normalised surface Dice at each tolerance, whole-region and lesion-wise, as
{region}_nsd@{tol} and {region}_lw_nsd@{tol} columns after the existing ones.  Without either flag the CSV is
what it always was.

    python -m scripts.score_predictions -d DATA_DIR -s PRED_DIR -o scores_mm.csv --mm --nsd_tolerance 1 2

--uncertainty_dir DIR scores the uncertainty maps the prediction scripts write there with the same flag
({id}_unc_whole / _unc_core / _unc_enhance.nii.gz, values 0..100) QU-BraTS style (gts.uncertainty):
after all other columns come, per region, {region}_qu, {region}_qu_dice_auc, {region}_qu_ftp_auc and
{region}_qu_ftn_auc.  --qu_thresholds T [T ...] sets the filtering thresholds (default 25 50 75 100; at most 8
strictly ascending integers in 0..100).  A scan with a missing or wrongly shaped map, or one holding a value above
100, is left out.  Without the flag the CSV is what it always was.

    python -m scripts.score_predictions -d DATA_DIR -s PRED_DIR -o scores_qu.csv --uncertainty_dir UNC_DIR
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import numpy as np  # noqa: E402

import Filepaths  # noqa: E402
from data_processing import labels as label_maps  # noqa: E402
from data_processing import nifti_io  # noqa: E402
from scripts import preprocess_dataset as prep  # noqa: E402

IO_WORKERS = 3     # threads for NIfTI decode around the GPU work
READ_AHEAD = 2     # scans decoded ahead of the one on the GPU
REGIONS = ("WT", "CT", "ET")
FIELDS = ("dice", "hd95", "lw_dice", "lw_hd95", "n_scored", "n_fp", "n_fn")
COUNTS = ("n_scored", "n_fp", "n_fn")
HEADER = ["id"] + [f"{region}_{field}" for region in REGIONS for field in FIELDS]
MAX_TOLERANCES = 4
QU_FIELDS = ("qu", "dice_auc", "ftp_auc", "ftn_auc")      # gts.uncertainty.FIELDS; columns {region}_qu, {region}_qu_*
QU_COLUMNS = [f"{region}_qu" + ("" if field == "qu" else f"_{field}") for region in REGIONS for field in QU_FIELDS]


def header_for(tolerances=(), qu=False):
    """HEADER, then per tolerance {region}_nsd@{tol} and {region}_lw_nsd@{tol} for the three regions, then (qu) the
    QU_COLUMNS."""
    return HEADER + [f"{region}_{field}@{tol:g}" for tol in tolerances for region in REGIONS
                     for field in ("nsd", "lw_nsd")] + (QU_COLUMNS if qu else [])


def build_parser():
    parser = argparse.ArgumentParser(description="Legacy and lesion-wise BraTS scores of written predictions on MI355X")
    parser.add_argument("-d", "--data_dir", default=None, type=str,
                        help="folder holding the scan folders (default: Filepaths.INPUT_MRI_DIR)")
    parser.add_argument("-l", "--label_extension", default="_seg.nii.gz", help="file suffix of the label volume")
    parser.add_argument("-s", "--pred_dir", required=True, help="folder holding the predictions, {id}.nii.gz")
    parser.add_argument("-p", "--data_prefix", default="", help="common prefix of the scan folders, e.g. BraTS2021")
    parser.add_argument("-o", "--output", required=True, help="the CSV file to write")
    parser.add_argument("--dilation", type=int, default=3, choices=(0, 1, 2, 3),
                        help="dilation steps that merge ground-truth components into lesions")
    parser.add_argument("--min_lesion_voxels", type=int, default=50,
                        help="a ground-truth lesion is scored when it has more voxels than this")
    parser.add_argument("--mm", action="store_true",
                        help="HD95 in millimetres, with the voxel spacing of the ground-truth file's affine")
    parser.add_argument("--nsd_tolerance", type=float, nargs="+", default=[], metavar="MM",
                        help=f"surface Dice tolerances in mm (at most {MAX_TOLERANCES}; implies --mm): appends "
                             "{region}_nsd@MM and {region}_lw_nsd@MM columns")
    parser.add_argument("--uncertainty_dir", default=None, metavar="DIR",
                        help="folder of the uncertainty maps {id}_unc_whole / _unc_core / _unc_enhance.nii.gz: appends "
                             "the {region}_qu columns")
    parser.add_argument("--qu_thresholds", type=int, nargs="+", default=None, metavar="T",
                        help="uncertainty thresholds of the QU score: at most 8 ascending integers in 0..100 "
                             "(default 25 50 75 100; needs --uncertainty_dir)")
    return parser


def qu_thresholds(args):
    """The QU thresholds of parsed arguments (None without --uncertainty_dir); FlagError for ones that cannot be
    scored, before any scan is read."""
    from gts.uncertainty import DEFAULT_THRESHOLDS, check_thresholds
    from scripts.ensemble_flags import FlagError

    given = getattr(args, "qu_thresholds", None)
    if not getattr(args, "uncertainty_dir", None):
        if given:
            raise FlagError("--qu_thresholds needs --uncertainty_dir")
        return None
    try:
        return check_thresholds(DEFAULT_THRESHOLDS if given is None else given)
    except ValueError as exc:
        raise FlagError(f"--qu_thresholds: {exc}") from None


def load_maps(uncertainty_dir, scan_id, shape):
    """Host stage of --uncertainty_dir: the scan's three maps as one C-contiguous uint8 [3, X, Y, Z]."""
    from gts.uncertainty import map_file_names

    maps = np.empty((3,) + tuple(shape), dtype=np.uint8)
    for k, name in enumerate(map_file_names(scan_id)):
        path = os.path.join(uncertainty_dir, name)
        if not os.path.exists(path):
            raise FileNotFoundError(f"no uncertainty map {path}")
        volume = nifti_io.read_nifti(path, np.int16)
        if volume.shape != tuple(shape):
            raise ValueError(f"uncertainty map {name} has shape {volume.shape}, the labels {tuple(shape)}")
        if volume.min() < 0 or volume.max() > 100:
            raise ValueError(f"uncertainty map {name} holds values outside 0..100")
        maps[k] = volume
    return maps


def spacing_of(path):
    """The voxel spacing (x, y, z) in mm of a NIfTI file: the column norms of its affine."""
    affine, _ = nifti_io.read_affine(path)
    return tuple(float(v) for v in np.sqrt((affine[:3, :3] ** 2).sum(axis=0)))


def load_spacing(folder, scan_id, label_extension, pred_dir):
    """Host stage of --mm: the truth file's voxel spacing, which the prediction's must equal in every step of
    1e-4 mm (the unit gts.metrics.spacing_units works in)."""
    truth_path = sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.endswith(label_extension))[0]
    spacing, pred_spacing = spacing_of(truth_path), spacing_of(os.path.join(pred_dir, scan_id + ".nii.gz"))
    if [round(v * 10000) for v in spacing] != [round(v * 10000) for v in pred_spacing]:
        raise ValueError(f"prediction spacing {pred_spacing} mm and ground-truth spacing {spacing} mm differ")
    return spacing


def load_pair(folder, scan_id, label_extension, pred_dir):
    """Host stage: both volumes as internal int16 labels, C-contiguous."""
    pred_path = os.path.join(pred_dir, scan_id + ".nii.gz")
    if not os.path.exists(pred_path):
        raise FileNotFoundError(f"no prediction {pred_path}")
    truth = label_maps.swap_labels_from_brats_any(nifti_io.read_in_labels(folder, label_extension))
    pred = label_maps.swap_labels_from_brats_any(nifti_io.read_nifti(pred_path, np.int16))
    if pred.shape != truth.shape:
        raise ValueError(f"prediction {pred.shape} and ground truth {truth.shape} differ in shape")
    if pred.ndim != 3:
        raise ValueError(f"label volumes have {pred.ndim} axes, expected 3")
    return np.ascontiguousarray(pred), np.ascontiguousarray(truth)


def row_of(scores, n_tolerances=0):
    """The CSV fields of one scan's lesionwise_scores record, in header_for's order (without the id)."""
    return [scores[region][field] for region in REGIONS for field in FIELDS] + \
        [scores[region][field][k] for k in range(n_tolerances) for region in REGIONS for field in ("nsd", "lw_nsd")]


def mean_row(rows):
    """Column means over the scans' rows (plain float64 means; counts become averages per scan)."""
    return [float(np.mean([row[c] for row in rows])) for c in range(len(rows[0]))]


def format_value(field, value):
    return str(int(value)) if field.split("_", 1)[1] in COUNTS and float(value).is_integer() else repr(float(value))


def format_row(name, values, header=HEADER):
    return ",".join([name] + [format_value(field, value) for field, value in zip(header[1:], values)])


def write_csv(path, rows, tolerances=(), qu=False):
    """rows: {id: values}; the ids in sorted order, then the mean row (when any scan was scored)."""
    header = header_for(tolerances, qu)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(",".join(header) + "\n")
        for scan_id in sorted(rows):
            f.write(format_row(scan_id, rows[scan_id], header) + "\n")
        if rows:
            f.write(format_row("mean", mean_row([rows[s] for s in sorted(rows)]), header) + "\n")


def score(scans, label_extension, pred_dir, dilation=3, min_lesion_voxels=50, mm=False, tolerances=(),
          uncertainty_dir=None, thresholds=None):
    """({id: CSV values}, ids left out) of {id: folder}.  uncertainty_dir / thresholds: the QU_COLUMNS are appended
    to every row."""
    import torch

    from gts import lesionwise, uncertainty

    ids = sorted(scans)
    rows, failed = {}, []
    with ThreadPoolExecutor(max_workers=IO_WORKERS) as pool:
        def load(i):
            pair = load_pair(scans[ids[i]], ids[i], label_extension, pred_dir)
            maps = (load_maps(uncertainty_dir, ids[i], pair[0].shape),) if uncertainty_dir else ()
            return pair + maps + ((load_spacing(scans[ids[i]], ids[i], label_extension, pred_dir),) if mm else ())

        def submit(i):
            return pool.submit(load, i)

        pending = {i: submit(i) for i in range(min(READ_AHEAD, len(ids)))}
        for i, scan_id in enumerate(ids):
            if i + READ_AHEAD < len(ids):
                pending[i + READ_AHEAD] = submit(i + READ_AHEAD)
            try:
                pred, truth, *rest = pending.pop(i).result()
                maps = rest.pop(0) if uncertainty_dir else None
                extra = dict(spacing_mm=rest[0], nsd_tolerances_mm=tuple(tolerances)) if mm else {}
                pred, truth = torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda()
                row = row_of(lesionwise.lesionwise_scores(pred, truth, dilation, min_lesion_voxels, **extra),
                             len(tolerances))
                if maps is not None:
                    qu = uncertainty.qu_scores(pred, truth, torch.from_numpy(maps).cuda(), thresholds)
                    row += [qu[region][field] for region in REGIONS for field in QU_FIELDS]
                rows[scan_id] = row
            except Exception as exc:
                print(f"{scan_id}: left out ({exc!r})")
                failed.append(scan_id)
    return rows, failed


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if len(args.nsd_tolerance) > MAX_TOLERANCES:
        parser.error(f"--nsd_tolerance takes at most {MAX_TOLERANCES} values")
    try:
        thresholds = qu_thresholds(args)
    except ValueError as exc:       # a FlagError
        print(f"score_predictions: {exc}", file=sys.stderr)
        return 2
    unc_dir = os.path.expanduser(args.uncertainty_dir) if args.uncertainty_dir else None
    mm = args.mm or bool(args.nsd_tolerance)
    scans = prep.find_scans(args.data_dir or Filepaths.INPUT_MRI_DIR, args.data_prefix)
    print(f"{len(scans)} scan folders found; scores go to {args.output}")
    rows, failed = score(scans, args.label_extension, os.path.expanduser(args.pred_dir), args.dilation,
                         args.min_lesion_voxels, mm, args.nsd_tolerance, unc_dir, thresholds)
    write_csv(os.path.expanduser(args.output), rows, args.nsd_tolerance, unc_dir is not None)
    if rows:
        means = mean_row([rows[s] for s in sorted(rows)])
        for r, region in enumerate(REGIONS):
            part = dict(zip(FIELDS, means[r * len(FIELDS):(r + 1) * len(FIELDS)]))
            print(f"{region}: Dice {part['dice']:.4f}, HD95 {part['hd95']:.3f}, lesion-wise Dice {part['lw_dice']:.4f}, "
                  f"lesion-wise HD95 {part['lw_hd95']:.3f} (per scan: {part['n_scored']:.2f} scored lesions, "
                  f"{part['n_fp']:.2f} false positives, {part['n_fn']:.2f} missed)")
            for k, tol in enumerate(args.nsd_tolerance):
                at = len(HEADER) - 1 + 2 * (len(REGIONS) * k + r)
                print(f"{region}: surface Dice at {tol:g} mm {means[at]:.4f}, lesion-wise {means[at + 1]:.4f}")
            if unc_dir is not None:
                part = dict(zip(QU_FIELDS, means[len(means) - len(QU_COLUMNS) + r * len(QU_FIELDS):]))
                print(f"{region}: QU score {part['qu']:.4f} at thresholds {' '.join(map(str, thresholds))} (Dice AUC "
                      f"{part['dice_auc']:.4f}, filtered TP AUC {part['ftp_auc']:.4f}, filtered TN AUC "
                      f"{part['ftn_auc']:.4f})")
    print(f"{len(rows)} scan(s) scored, {len(failed)} left out")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
