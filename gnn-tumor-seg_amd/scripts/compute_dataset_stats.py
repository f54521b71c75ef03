"""Raw scan folders -> the dataset's standardization statistics, on the MI355X (counterpart of the
reference's DataPreprocessor.compute_dataset_stats, scripts/preprocess_dataset.py:93-115, which it only
reaches when its STANDARDIZATION_STATS constant is edited to None).

For each scan folder the four modalities and the label volume are decoded and uploaded as stored; the
healthy-tissue mask (first modality > 0.001, label 0), the 0.995 quantile of each modality over it and the
mean and standard deviation of the normalized values are taken on the device (gts.dataset_stats, D1-D3).
The dataset's values are the medians over the scans.  They go into a JSON file that
`preprocess_dataset --stats` and `segment_scans --stats` read, together with the modality list they belong
to and each scan's own values.

Labels are required: the method is defined on the healthy tissue.  The GPU takes one scan at a time while
a small thread pool decodes the next ones.  A scan that raises is reported and left out of the medians;
the exit status is 1 when any scan was left out.

    python -m scripts.compute_dataset_stats -d RAW_DIR -l _seg.nii.gz -o STATS.json

--bias_correct (and the --bias_* settings, as scripts.segment_scans documents them) removes each modality's bias field
on the device (gts.bias) before the statistics are taken, for datasets that are preprocessed and
segmented with the same flag.  --skull_strip [MODALITY] (and the --strip_* settings) sets every modality to 0 outside a
brain mask found on the device (gts.brainmask) before that, for scans that still hold their skull.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import Filepaths  # noqa: E402
from data_processing import nifti_io, standardization  # noqa: E402
from scripts import preprocess_dataset as prep  # noqa: E402

IO_WORKERS = 3     # threads for NIfTI decode around the GPU work
READ_AHEAD = 2     # scans decoded ahead of the one on the GPU
QUANTILE = 0.995   # normalize_img's


def build_parser():
    """preprocess_dataset's data flags (same names, defaults and meanings) and the output file."""
    parser = argparse.ArgumentParser(description="Standardization statistics of a raw MRI dataset on MI355X")
    parser.add_argument("-d", "--data_dir", default=None, type=str,
                        help="folder holding the raw scan folders (default: Filepaths.INPUT_MRI_DIR)")
    parser.add_argument("-m", "--modality_extensions", nargs="+", default=list(prep.BRATS_MODALITIES),
                        help="file suffix of each modality, in channel order")
    parser.add_argument("-l", "--label_extension", default=None,
                        help="file suffix of the label volume (required: the statistics are taken over healthy tissue)")
    parser.add_argument("-p", "--data_prefix", default="", help="common prefix of the scan folders, e.g. BraTS2021")
    parser.add_argument("-o", "--output", default=None, type=str, help="the statistics file to write (JSON)")
    from gts import bias, brainmask

    return brainmask.add_flags(bias.add_flags(parser))


def check_request(modality_extensions, label_extension):
    """StatsError for what the method cannot work with."""
    if not label_extension:
        raise standardization.StatsError("dataset statistics need the label volumes (-l): they are taken over "
                                         "healthy tissue, voxels with label 0")
    if len(modality_extensions) != standardization.CHANNELS:
        raise standardization.StatsError(f"{len(modality_extensions)} modalities given; intake and graph generation "
                                         f"are built for exactly {standardization.CHANNELS}, other counts are not "
                                         "supported")


def load_scan(folder, modality_extensions, label_extension):
    """Host stage: decode the modalities and the labels and stage them for the upload."""
    from gts import dataset_stats, intake

    staged = intake.stage_scan(nifti_io.read_in_patient_sample_raw(folder, modality_extensions))
    return staged, dataset_stats.stage_labels(nifti_io.read_in_labels(folder, label_extension))


def compute(scans, modality_extensions, label_extension, q=QUANTILE, bias_settings=None, bias_report=None,
            strip_settings=None, strip_report=None):
    """Per-scan statistics of {id: folder}: ({id: ScanStats}, ids left out).  bias_settings: gts.bias.correct_volume's
    settings, to correct every modality on the device first (None: the values as stored); bias_report, a dict,
    receives the correction's per-modality reports by scan id.  strip_settings: gts.brainmask.settings_from_args' pair,
    to strip the skull on the device before that; strip_report receives the masks' reports."""
    from gts import bias, brainmask, dataset_stats, intake

    check_request(modality_extensions, label_extension)
    ids = sorted(scans)
    per_scan, failed = {}, []
    with ThreadPoolExecutor(max_workers=IO_WORKERS) as pool:
        def submit(i):
            return pool.submit(load_scan, scans[ids[i]], modality_extensions, label_extension)

        pending = {i: submit(i) for i in range(min(READ_AHEAD, len(ids)))}
        for i, scan_id in enumerate(ids):
            if i + READ_AHEAD < len(ids):
                pending[i + READ_AHEAD] = submit(i + READ_AHEAD)
            try:
                staged, labels = pending.pop(i).result()
                if strip_settings is not None:
                    staged, _, found = brainmask.strip_scan(staged.to(intake._device(), non_blocking=True),
                                                            strip_settings[0], **strip_settings[1])
                    if strip_report is not None:
                        strip_report[scan_id] = found
                if bias_settings is not None:
                    staged, reports = bias.correct_scan(staged.to(intake._device(), non_blocking=True), **bias_settings)
                    if bias_report is not None:
                        bias_report[scan_id] = reports
                per_scan[scan_id] = dataset_stats.scan_stats(staged, labels, q)
            except Exception as exc:
                print(f"{scan_id}: left out ({exc!r})")
                failed.append(scan_id)
    return per_scan, failed


def compute_and_save(scans, modality_extensions, label_extension, path, q=QUANTILE, bias_settings=None,
                     bias_report=None, strip_settings=None, strip_report=None):
    """compute, then the medians into the file at path: (mean, std, ids left out).  StatsError when no
    scan gave statistics (nothing is written then)."""
    from gts import dataset_stats

    per_scan, failed = compute(scans, modality_extensions, label_extension, q, bias_settings, bias_report,
                               strip_settings, strip_report)
    if not per_scan:
        raise standardization.StatsError(f"none of the {len(scans)} scan(s) gave statistics")
    mean, std = dataset_stats.dataset_stats([per_scan[s] for s in sorted(per_scan)])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    standardization.save_stats(path, mean, std, modality_extensions, q, per_scan)
    return mean, std, failed


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.output:
        parser.error("-o STATS.json is required")
    try:
        check_request(args.modality_extensions, args.label_extension)
    except standardization.StatsError as exc:
        parser.error(str(exc))
    from gts import bias, brainmask

    try:
        settings = bias.settings_from_args(args)
        strip = brainmask.settings_from_args(args)
    except ValueError as exc:
        parser.error(str(exc))
    report, strip_report = {}, {}
    scans = prep.find_scans(args.data_dir or Filepaths.INPUT_MRI_DIR, args.data_prefix)
    print(f"{len(scans)} scan folders found; statistics go to {args.output}")
    try:
        mean, std, failed = compute_and_save(scans, args.modality_extensions, args.label_extension,
                                             os.path.expanduser(args.output), bias_settings=settings,
                                             bias_report=report, strip_settings=strip, strip_report=strip_report)
    except standardization.StatsError as exc:
        print(f"no statistics written: {exc}")
        return 1
    if args.bias_report:
        bias.save_report(args.bias_report, args.modality_extensions, settings, report)
    if args.strip_report:
        brainmask.save_report(args.strip_report, args.modality_extensions, strip[0], strip[1], strip_report)
    for scan_id in sorted(strip_report):
        print(f"{scan_id}: {brainmask.describe(strip_report[scan_id])}")
    print(f"mean {mean.tolist()}, standard deviation {std.tolist()} over {len(scans) - len(failed)} scan(s), "
          f"{len(failed)} left out")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
