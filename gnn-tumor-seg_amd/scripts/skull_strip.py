"""Scan folders -> the same scans with everything outside the brain set to 0, on the MI355X (gts.brainmask, DESIGN.md
4x: threshold, erosion by a ball, largest connected component, dilation, closing, hole fill, under this project's own
definition; it has not been run on real anatomy, and agreement with BET, HD-BET or ROBEX is unknown).

For every scan under SCANS (found as scripts.segment_scans finds them) each modality file is decoded and uploaded as
stored (int16 or float32), the mask is found from one modality (--strip_modality; default _t1.nii.gz when it is among
the extensions, else the first) and every modality is written to OUT/{id}/ under its own file name, in its own dtype and
with its own affine, 0 outside the mask.  --save_mask also writes {id}_brainmask.nii.gz (int16 0/1, the affine of the
modality the mask came from).  The modalities of a scan must share one grid (co-register first if they do not).  A
scan that raises is reported and skipped; the exit status is 1 when any scan was skipped.

    python -m scripts.skull_strip -d SCANS -o OUT [--save_mask] [--strip_modality EXT --strip_radius R --strip_close R
                                  --strip_fraction F --strip_connectivity {6,26} --strip_report FILE.json]
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
from gts import brainmask  # noqa: E402
from scripts import preprocess_dataset as prep  # noqa: E402
from scripts import segment_scans  # noqa: E402


def build_parser():
    parser = argparse.ArgumentParser(description="Strip the skull of MRI scans on MI355X: NIfTI in, NIfTI out")
    parser.add_argument("-d", "--data_dir", required=True,
                        help="folder of one scan's modality files, or a folder of scan folders")
    parser.add_argument("-o", "--output_dir", required=True, help="where {id}/{modality file} goes")
    parser.add_argument("-M", "--modality_extensions", nargs="+", default=list(prep.BRATS_MODALITIES),
                        help="file suffix of each modality")
    parser.add_argument("-p", "--data_prefix", default="", help="common prefix of the scan folders, e.g. BraTS2021")
    parser.add_argument("--save_mask", action="store_true", help="also write the brain mask")
    return brainmask.add_flags(parser, switch=False)


def _stage(path):
    """One modality file as the device tensor [Z, Y, X] in its stored dtype (int16 or float32, else float32)."""
    volume = np.asarray(nifti_io.read_nifti_raw(path))
    if volume.dtype not in (np.int16, np.float32):
        volume = volume.astype(np.float32)
    device = torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(np.array(volume.T, order="C")).to(device)


def strip_files(paths, out_paths, ref_index, settings, mask_path=None):
    """The modality files of one scan -> their stripped files, each with its own dtype and affine; returns the report."""
    volumes = [_stage(p) for p in paths]
    if any(v.shape != volumes[0].shape for v in volumes):
        raise ValueError(f"the modalities lie on different grids {[tuple(v.shape)[::-1] for v in volumes]}: "
                         "co-register them first")
    mask, report = brainmask.brain_mask(volumes[ref_index], **settings)
    for volume, path, out_path in zip(volumes, paths, out_paths):
        stripped, _ = brainmask.apply_mask(volume, mask)
        nifti_io.save_as_nifti(np.asfortranarray(stripped.cpu().numpy().T), out_path, nifti_io.read_affine(path)[0])
    if mask_path:
        nifti_io.save_as_nifti(np.asfortranarray(mask.cpu().numpy().T), mask_path,
                               nifti_io.read_affine(paths[ref_index])[0])
    return report


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        ref_index, settings = brainmask.settings_from_args(args, switch=False)
    except ValueError as exc:
        print(f"skull_strip: {exc}", file=sys.stderr)
        return 2
    if not torch.cuda.is_available():
        raise RuntimeError("skull_strip needs an AMD GPU (no CPU fallback)")
    scans = segment_scans.find_inputs(args.data_dir, args.modality_extensions, args.data_prefix)
    out_root = os.path.expanduser(args.output_dir)
    print(f"{len(scans)} scan(s) found; stripped volumes go to {out_root}")
    failed, reports = [], {}
    for scan_id in sorted(scans):
        try:
            paths = nifti_io.find_modality_files(scans[scan_id], args.modality_extensions)
            os.makedirs(os.path.join(out_root, scan_id), exist_ok=True)
            out_paths = [os.path.join(out_root, scan_id, os.path.basename(p)) for p in paths]
            mask_path = os.path.join(out_root, scan_id, scan_id + brainmask.MASK_SUFFIX) if args.save_mask else None
            reports[scan_id] = strip_files(paths, out_paths, ref_index, settings, mask_path)
            print(f"{scan_id}: done ({brainmask.describe(reports[scan_id])})")
        except Exception as exc:
            print(f"{scan_id}: skipped ({exc!r})")
            failed.append(scan_id)
    if args.strip_report:
        brainmask.save_report(args.strip_report, args.modality_extensions, ref_index, settings, reports)
    print(f"skull stripping finished, {len(failed)} scan(s) skipped")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
