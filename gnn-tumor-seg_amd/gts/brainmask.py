"""Brain extraction (skull stripping) of MRI volumes on the MI355X: the classical morphological scheme under this
project's own definition (S1-S6, csrc/gts_brainmask.hip).

A scan as the scanner writes it still holds skull, scalp and neck.  The mask of the intracranial volume is found from
one modality: a threshold from the robust range of the positive intensities (S1, S2 and `threshold_from_counts`, numpy
on the 4096 counts), an erosion by a ball that cuts the thin bridges between brain and scalp (S3), the largest
connected component of what is left (S4), a dilation by the same ball, a closing by a second ball (S3), and a hole
fill (S5).  Every modality of the scan is then set to 0 outside the mask (S6).

Every step is integer work and equals scipy.ndimage voxel for voxel (tests/brainmask_ref.py).  The definition is
symmetric in the axes: a volume is handed over as the tensor lies in memory.  Nothing here has been run on real
anatomy, and agreement with BET, HD-BET or ROBEX is unknown.  The defaults (radius 3, close 2, fraction 0.1) are
untuned.

threshold_from_counts, squared_radius and the flag helpers are pure numpy and run without a GPU.
"""
import math

import numpy as np

BINS = 4096
LOW_QUANTILE, HIGH_QUANTILE = 0.02, 0.98
MAX_R2 = 255
DEFAULT_RADIUS = 3.0
DEFAULT_CLOSE = 2.0
DEFAULT_FRACTION = 0.1
DEFAULT_CONNECTIVITY = 6
DEFAULT_MODALITY = "_t1.nii.gz"
MASK_SUFFIX = "_brainmask.nii.gz"


def squared_radius(radius):
    """R2 = floor(radius^2) of a ball radius in voxels: the ball holds the integer offsets o with |o|^2 <= R2.  Raises
    ValueError outside 0 <= R2 <= 255."""
    radius = float(radius)
    if not (radius >= 0 and math.isfinite(radius)) or math.floor(radius * radius) > MAX_R2:
        raise ValueError(f"a ball radius of {radius} voxels is outside 0 <= floor(r^2) <= {MAX_R2}")
    return int(math.floor(radius * radius))


def check_settings(radius, close, fraction, connectivity):
    """Raises ValueError for settings brain_mask cannot run with."""
    squared_radius(radius)
    squared_radius(close)
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError(f"the threshold fraction {fraction} is outside [0, 1]")
    if connectivity not in (6, 26):
        raise ValueError(f"connectivity {connectivity!r} (6 or 26)")


def threshold_from_counts(counts, hi, fraction=DEFAULT_FRACTION):
    """(t, b2, b98) from the 4096 counts of the positive voxels over (0, hi]: b2 and b98 are the first bins whose
    cumulative count reaches ceil(0.02 n) and ceil(0.98 n), t = (b2 + fraction (b98 - b2)) hi / 4096 in float64."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if counts.size != BINS or counts.min() < 0 or counts.sum() == 0:
        raise ValueError(f"threshold_from_counts takes {BINS} counts that are not negative and not all zero")
    n = int(counts.sum())
    cum = np.cumsum(counts)
    b2 = int(np.searchsorted(cum, math.ceil(LOW_QUANTILE * n), side="left"))
    b98 = int(np.searchsorted(cum, math.ceil(HIGH_QUANTILE * n), side="left"))
    t = (np.float64(b2) + np.float64(fraction) * np.float64(b98 - b2)) * np.float64(hi) / np.float64(BINS)
    return float(t), b2, b98


# ---- the steps on the device: thin fronts over gts.ops that raise where the definition raises ----------------------

def brain_range(volume, grid_blocks=0):
    """(n, hi) of the finite voxels > 0.  Raises ValueError when there is none."""
    from . import ops

    n, hi = ops.brain_range(volume, grid_blocks)
    if n == 0:
        raise ValueError("no finite voxel above 0: nothing to find a brain in")
    return n, hi


def brain_histogram(volume, hi, grid_blocks=0):
    from . import ops

    return ops.brain_histogram(volume, hi, grid_blocks)


def ball_erode(mask, r2, border_value=0, grid_blocks=0):
    from . import ops

    return ops.ball_erode(mask, r2, border_value, grid_blocks)


def ball_dilate(mask, r2, grid_blocks=0):
    from . import ops

    return ops.ball_dilate(mask, r2, grid_blocks)


def largest_component(mask, connectivity=DEFAULT_CONNECTIVITY, grid_blocks=0):
    """(keep, {"components", "largest", "second", "voxels"}).  Raises ValueError for an empty mask."""
    from . import ops

    keep, stats = ops.largest_component(mask, connectivity, grid_blocks)
    components, largest, second, _, voxels = stats.tolist()
    if components == 0:
        raise ValueError("nothing is left after the erosion: no component to keep")
    return keep, {"components": int(components), "largest": int(largest), "second": int(second), "voxels": int(voxels)}


def fill_holes(mask, grid_blocks=0):
    from . import ops

    return ops.fill_holes(mask, grid_blocks)


def apply_mask(scan, mask, grid_blocks=0):
    from . import ops

    return ops.apply_mask(scan, mask, grid_blocks)


def brain_mask(volume, radius=DEFAULT_RADIUS, close=DEFAULT_CLOSE, fraction=DEFAULT_FRACTION,
               connectivity=DEFAULT_CONNECTIVITY, timer=None, grid_blocks=0):
    """One volume (a device tensor of three axes, int16 or float32) -> (mask int16 0/1 of its shape, report).
    report: {"threshold", "hi", "positive_voxels", "threshold_voxels", "eroded_voxels", "components", "largest",
    "second", "mask_voxels", "mask_ml", "mask_fraction"}; mask_ml takes a voxel as 1 mm^3.  Raises ValueError when no
    voxel is positive or the erosion leaves nothing."""
    from . import ops

    check_settings(radius, close, fraction, connectivity)
    r2e, r2c = squared_radius(radius), squared_radius(close)
    tick = timer or (lambda name: None)
    volume = volume.contiguous()
    n, hi = brain_range(volume, grid_blocks)
    tick("S1")
    counts = ops.brain_histogram(volume, hi, grid_blocks).cpu().numpy()
    t, _, _ = threshold_from_counts(counts, hi, fraction)
    m0, m0_count = ops.brain_threshold(volume, t, grid_blocks)
    tick("S2")
    eroded = ops.ball_erode(m0, r2e, 0, grid_blocks)
    tick("S3 erode")
    keep, found = largest_component(eroded, connectivity, grid_blocks)
    tick("S4")
    mask = ops.ball_dilate(keep, r2e, grid_blocks)
    if r2c > 0:
        mask = ops.ball_erode(ops.ball_dilate(mask, r2c, grid_blocks), r2c, 1, grid_blocks)
    tick("S3 dilate, close")
    mask, stats = ops.fill_holes(mask, grid_blocks)
    voxels = int(stats[0].item())
    tick("S5")
    report = {"threshold": t, "hi": hi, "positive_voxels": n, "threshold_voxels": int(m0_count.item()),
              "eroded_voxels": found["voxels"], "components": found["components"], "largest": found["largest"],
              "second": found["second"], "mask_voxels": voxels, "mask_ml": voxels / 1000.0,
              "mask_fraction": voxels / n}
    return mask, report


def reference_index(modality_extensions, modality=None):
    """The index of the modality the mask is computed from: `modality` when named (ValueError if it is none of the
    extensions), else _t1.nii.gz when it is among them, else the first."""
    extensions = list(modality_extensions)
    if modality:
        if modality not in extensions:
            raise ValueError(f"--skull_strip {modality!r} is none of the modality extensions {extensions}")
        return extensions.index(modality)
    return extensions.index(DEFAULT_MODALITY) if DEFAULT_MODALITY in extensions else 0


def strip_scan(scan, ref_index=0, **settings):
    """A scan [C, Z, Y, X] on the device (int16 or float32) -> (the scan with every modality 0 outside the brain mask
    of modality ref_index, dtype kept; the mask int16 [Z, Y, X]; the report)."""
    if scan.dim() != 4 or not 0 <= int(ref_index) < scan.shape[0]:
        raise ValueError(f"strip_scan takes [C, Z, Y, X] and a modality index below C, got {tuple(scan.shape)}, "
                         f"{ref_index}")
    scan = scan.contiguous()
    mask, report = brain_mask(scan[int(ref_index)], **settings)
    stripped, _ = apply_mask(scan, mask, settings.get("grid_blocks", 0))
    if settings.get("timer"):
        settings["timer"]("S6")
    return stripped, mask, report


def strip_image(image, ref_index=0, **settings):
    """A host image [X, Y, Z, C] (as nifti_io.read_in_patient_sample stacks a scan) -> (the stripped float32 image of
    the same layout, the mask int16 [X, Y, Z], the report): upload, strip_scan, download."""
    import torch

    host = np.ascontiguousarray(np.asarray(image, dtype=np.float32).transpose(3, 2, 1, 0))
    device = torch.device("cuda", torch.cuda.current_device())
    out, mask, report = strip_scan(torch.from_numpy(host).to(device), ref_index, **settings)
    return (np.ascontiguousarray(out.cpu().numpy().transpose(3, 2, 1, 0)),
            np.ascontiguousarray(mask.cpu().numpy().transpose(2, 1, 0)), report)


# ---- command-line flags, shared by segment_scans, preprocess_dataset, compute_dataset_stats and skull_strip ----------

def add_flags(parser, switch=True):
    """--skull_strip and its settings; with switch=False the modality is --strip_modality (scripts.skull_strip always
    strips)."""
    if switch:
        parser.add_argument("--skull_strip", nargs="?", const="", default=None, metavar="MODALITY",
                            help="set every modality to 0 outside a brain mask found on the device from this modality "
                                 "(its extension; default: _t1.nii.gz when present, else the first) before anything "
                                 "else looks at the intensities (gts.brainmask: threshold, erode, largest component, "
                                 "dilate, close, fill)")
    else:
        parser.add_argument("--strip_modality", default="", metavar="MODALITY",
                            help="extension of the modality the mask is found from (default: _t1.nii.gz when present, "
                                 "else the first)")
    parser.add_argument("--strip_radius", type=float, default=DEFAULT_RADIUS, metavar="R",
                        help="radius in voxels of the ball the thresholded volume is eroded and dilated with")
    parser.add_argument("--strip_close", type=float, default=DEFAULT_CLOSE, metavar="R",
                        help="radius in voxels of the ball the mask is closed with (0: no closing)")
    parser.add_argument("--strip_fraction", type=float, default=DEFAULT_FRACTION, metavar="F",
                        help="where the threshold lies between the 2nd and the 98th percentile of the positive voxels")
    parser.add_argument("--strip_connectivity", type=int, choices=(6, 26), default=DEFAULT_CONNECTIVITY,
                        help="connectivity of the component that is kept")
    parser.add_argument("--strip_report", default=None, metavar="FILE.json",
                        help="write per scan the threshold, the voxel counts of every step and the mask's volume")
    return parser


def settings_from_args(args, switch=True):
    """None with --skull_strip absent, else (the index of the modality the mask comes from, the keyword arguments of
    brain_mask).  Raises ValueError for settings that cannot run, before any scan is read."""
    modality = getattr(args, "skull_strip", None) if switch else getattr(args, "strip_modality", "")
    if modality is None:
        changed = [name for name, default in (("strip_radius", DEFAULT_RADIUS), ("strip_close", DEFAULT_CLOSE),
                                              ("strip_fraction", DEFAULT_FRACTION),
                                              ("strip_connectivity", DEFAULT_CONNECTIVITY), ("strip_report", None),
                                              ("strip_mask_dir", None))
                   if getattr(args, name, default) != default]
        if changed:
            raise ValueError("--" + ", --".join(changed) + " need --skull_strip")
        return None
    check_settings(args.strip_radius, args.strip_close, args.strip_fraction, args.strip_connectivity)
    settings = dict(radius=args.strip_radius, close=args.strip_close, fraction=args.strip_fraction,
                    connectivity=args.strip_connectivity)
    return reference_index(args.modality_extensions, modality), settings


def describe(report):
    """One note for a scan's line of output: the mask's volume and what the component step saw."""
    note = (f"strip: brain {report['mask_ml']:.1f} ml ({100.0 * report['mask_fraction']:.1f}% of the positive voxels), "
            f"{report['components']} component(s) after the erosion")
    if 2 * report["second"] >= report["largest"]:
        note += (f", the second largest has {report['second']} voxels against {report['largest']}: check this scan")
    return note


def save_report(path, modality_extensions, ref_index, settings, scans):
    """--strip_report: the settings, the modality the masks were found from and, per scan id, its report."""
    import json
    import os

    with open(os.path.expanduser(path), "w") as f:
        json.dump({"modalities": list(modality_extensions), "mask_from": list(modality_extensions)[ref_index],
                   "settings": settings, "scans": scans}, f, indent=1)
        f.write("\n")
