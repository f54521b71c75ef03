"""Scan folders -> the same scans with each modality's bias field removed, on the MI355X (gts.bias, DESIGN.md 4w:
N4's scheme of histogram sharpening and multilevel B-spline fitting under this project's definition).

For every scan under SCANS (found as scripts.segment_scans finds them) each modality file is decoded, uploaded as
stored (int16 or float32), corrected on the device on its own grid and written as float32 to OUT/{id}/ under its own
file name with the input's own affine.  --save_field also writes the estimated field as a ratio (the factor the
volume was divided by), {name}_biasfield.nii.gz.  The mask the field is estimated from is every voxel above
--bias_threshold (default 0): strip the skull first (scripts.skull_strip).  A scan that raises is reported and skipped; the exit
status is 1 when any scan was skipped.

    python -m scripts.bias_correct -d SCANS -o OUT [--save_field] [--bias_levels L --bias_spans S --bias_iterations N
                                   --bias_tol T --bias_threshold V --bias_report FILE.json]
"""
import argparse
import os
import sys

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from data_processing import nifti_io  # noqa: E402
from gts import bias  # noqa: E402
from scripts import preprocess_dataset as prep  # noqa: E402
from scripts import segment_scans  # noqa: E402

FIELD_SUFFIX = "_biasfield.nii.gz"


def build_parser():
    parser = argparse.ArgumentParser(description="Remove the bias field of MRI scans on MI355X: NIfTI in, NIfTI out")
    parser.add_argument("-d", "--data_dir", required=True,
                        help="folder of one scan's modality files, or a folder of scan folders")
    parser.add_argument("-o", "--output_dir", required=True, help="where {id}/{modality file} goes")
    parser.add_argument("-M", "--modality_extensions", nargs="+", default=list(prep.BRATS_MODALITIES),
                        help="file suffix of each modality")
    parser.add_argument("-p", "--data_prefix", default="", help="common prefix of the scan folders, e.g. BraTS2021")
    parser.add_argument("--save_field", action="store_true", help="also write the field each volume was divided by")
    return bias.add_flags(parser, switch=False)


def correct_file(path, out_path, settings, field_path=None):
    """One modality file -> its corrected float32 file with the same affine; returns the report."""
    volume = np.asarray(nifti_io.read_nifti_raw(path))
    if volume.dtype not in (np.int16, np.float32):
        volume = volume.astype(np.float32)
    affine = nifti_io.read_affine(path)[0]
    device = torch.device("cuda", torch.cuda.current_device())
    staged = torch.from_numpy(np.array(volume.T, order="C")).to(device)          # [Z, Y, X], x fastest
    corrected, field, report = bias.correct_volume(staged, want_field=True, **settings)
    nifti_io.save_as_nifti(np.asfortranarray(corrected.cpu().numpy().T), out_path, affine)
    if field_path:
        nifti_io.save_as_nifti(np.asfortranarray(torch.exp(field).cpu().numpy().T), field_path, affine)
    return report


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        settings = bias.settings_from_args(args, switch=False)
    except ValueError as exc:
        print(f"bias_correct: {exc}", file=sys.stderr)
        return 2
    if not torch.cuda.is_available():
        raise RuntimeError("bias_correct needs an AMD GPU (no CPU fallback)")
    scans = segment_scans.find_inputs(args.data_dir, args.modality_extensions, args.data_prefix)
    out_root = os.path.expanduser(args.output_dir)
    print(f"{len(scans)} scan(s) found; corrected volumes go to {out_root}")
    failed, reports = [], {}
    for scan_id in sorted(scans):
        try:
            paths = nifti_io.find_modality_files(scans[scan_id], args.modality_extensions)
            os.makedirs(os.path.join(out_root, scan_id), exist_ok=True)
            rows = []
            for path, ext in zip(paths, args.modality_extensions):
                name = os.path.basename(path)
                out_path = os.path.join(out_root, scan_id, name)
                field_path = out_path[:-len(ext)] + ext.split(".")[0] + FIELD_SUFFIX if args.save_field else None
                rows.append(correct_file(path, out_path, settings, field_path))
            reports[scan_id] = rows
            print(f"{scan_id}: done ({bias.describe(rows)})")
        except Exception as exc:
            print(f"{scan_id}: skipped ({exc!r})")
            failed.append(scan_id)
    if args.bias_report:
        bias.save_report(args.bias_report, args.modality_extensions, settings, reports)
    print(f"bias correction finished, {len(failed)} scan(s) skipped")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
