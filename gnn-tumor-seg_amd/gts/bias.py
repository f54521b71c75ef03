"""Bias-field correction of MRI volumes on the MI355X: N4's scheme under this project's own definition (Z1-Z5,
csrc/gts_bias.hip).

The bias field is a slowly varying multiplicative intensity inhomogeneity.  Its logarithm is modelled as a sum of
uniform cubic B-spline lattices, coarse to fine.  One iteration at a level: the range and the 200-bin histogram of
the log image minus the field so far (Z2, Z3), the histogram sharpened by a Wiener deconvolution with a Gaussian
(`sharpen`, numpy on the host, 512 points), the residual between each voxel and its sharpened value fitted by Lee's
multilevel B-spline approximation (Z4) and added to the level's lattice.  At the end the field's mean over the mask is
removed and the volume divided by exp(field) (Z5).

basis, fit_weights, sharpen and the flag helpers are pure numpy and run without a GPU.  Volumes on the device are
[Z, Y, X], x fastest, as intake.stage_scan lays them out.

The level ends after `iterations` rounds or when the largest change of a control point falls below `tol`; a B-spline
lies in the hull of its control points, so that bounds the change of the field.  On the phantoms this was developed
on, the change stayed above 4e-3 and every level ran to its cap: `tol` = 1e-3 is a stop for easy cases, not a
quality setting.
"""
import numpy as np

BINS = 200
FWHM = 0.15                 # of the Gaussian the histogram is sharpened with, in log units
WIENER_NOISE = 0.01
MAX_SPANS = 32
DEFAULT_LEVELS = 4
DEFAULT_SPANS = 1
DEFAULT_ITERATIONS = 50
DEFAULT_TOL = 1e-3
DEFAULT_THRESHOLD = 0.0


def check_levels(spans0, levels):
    """Raises ValueError unless spans0 >= 1, levels >= 1 and the finest level has at most MAX_SPANS spans."""
    if int(spans0) < 1 or int(levels) < 1 or int(spans0) << (int(levels) - 1) > MAX_SPANS:
        raise ValueError(f"bias lattices: {spans0} span(s) doubled over {levels} level(s) must stay within 1..{MAX_SPANS} "
                         "spans per axis")


def basis(n, spans):
    """(cell int32 [n], weights float64 [n, 4]) of an axis of extent n cut into `spans` cells: index i lies at t =
    float64(i * spans) / float64(n), in cell floor(t) at s = t - cell, and the uniform cubic B-spline weights
        B0 = ((a a) a) / 6 with a = 1 - s,   B1 = ((3 s3 - 6 s2) + 4) / 6,   B2 = (((-3 s3 + 3 s2) + 3 s) + 1) / 6,
        B3 = s3 / 6,   s2 = s s, s3 = s2 s
    sit on the control points cell .. cell + 3.  Each row sums to 1 up to rounding."""
    i = np.arange(int(n), dtype=np.int64)
    t = (i * int(spans)).astype(np.float64) / np.float64(n)
    cell = np.floor(t)
    s = t - cell
    a = 1.0 - s
    s2 = s * s
    s3 = s2 * s
    w = np.stack([((a * a) * a) / 6.0, ((3.0 * s3 - 6.0 * s2) + 4.0) / 6.0,
                  (((-3.0 * s3 + 3.0 * s2) + 3.0 * s) + 1.0) / 6.0, s3 / 6.0], axis=1)
    return cell.astype(np.int32), w


def fit_weights(w):
    """float64 [8, n] from basis weights [n, 4]: rows 0..3 p_a = B_a^3 / sum_a B_a^2, rows 4..7 q_a = B_a^2: what one
    axis contributes to the numerator and the denominator of Lee's B-spline approximation."""
    q = w * w
    return np.concatenate([(q * w / q.sum(axis=1, keepdims=True)).T, q.T], axis=0)


def tables(shape, spans0=DEFAULT_SPANS, levels=DEFAULT_LEVELS, device=None):
    """ops.BiasTables for a volume of shape (X, Y, Z): every level's basis of every axis, on the device."""
    import torch

    from . import ops

    check_levels(spans0, levels)
    per_axis = [[basis(n, int(spans0) << level) for level in range(int(levels))] for n in shape]
    weights = np.concatenate([np.stack([w.T for _, w in axis]).reshape(-1) for axis in per_axis])
    cells = np.concatenate([np.stack([c for c, _ in axis]).reshape(-1) for axis in per_axis])
    fit = [np.concatenate([fit_weights(axis[level][1]).reshape(-1) for axis in per_axis]) for level in range(int(levels))]
    device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return ops.BiasTables(shape, spans0, levels, weights, cells, fit, device)


def sharpen(counts, lo, hi):
    """float64 [BINS]: the sharpened value E of every bin of a histogram of d over [lo, hi] (bin centres lo + i w, w =
    (hi - lo) / (BINS - 1)).  The counts are zero-padded, centred, to P = 512 points; F is the FFT of a unit-sum
    Gaussian of FWHM 0.15 log units in bins of w, wrapped around index 0; the counts are deconvolved with the Wiener
    filter G = conj(F) / (|F|^2 + 0.01), U = max(Re ifft(fft(H) G), 0), and E = Re ifft(fft(centre U) F) / Re ifft(fft(U)
    F): the mean of the sharpened distribution's values that the blur carries into the bin.  Where that denominator
    is not above 1e-12 of its maximum, E is the bin centre itself."""
    counts = np.asarray(counts, dtype=np.float64).reshape(-1)
    bins = counts.size
    p = 1
    while p < 2 * bins:
        p *= 2
    offset = (p - bins) // 2
    w = (np.float64(hi) - np.float64(lo)) / np.float64(bins - 1)
    h = np.zeros(p, dtype=np.float64)
    h[offset:offset + bins] = counts
    sigma = (FWHM / w) / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    j = np.arange(p, dtype=np.float64)
    k = np.minimum(j, p - j)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    g = g / g.sum()
    f = np.fft.fft(g)
    wiener = np.conj(f) / (np.abs(f) ** 2 + WIENER_NOISE)
    u = np.maximum(np.real(np.fft.ifft(np.fft.fft(h) * wiener)), 0.0)
    centre = np.float64(lo) + (j - offset) * w
    num = np.real(np.fft.ifft(np.fft.fft(centre * u) * f))
    den = np.real(np.fft.ifft(np.fft.fft(u) * f))
    ok = den > 1e-12 * den.max()
    e = np.where(ok, num / np.where(ok, den, 1.0), centre)
    return e[offset:offset + bins]


def correct_volume(volume, levels=DEFAULT_LEVELS, spans0=DEFAULT_SPANS, iterations=DEFAULT_ITERATIONS, tol=DEFAULT_TOL,
                   threshold=DEFAULT_THRESHOLD, want_field=False, out=None, timer=None):
    """One modality volume (a device tensor [Z, Y, X], int16 or float32) -> (corrected float32 [Z, Y, X], report);
    with want_field (corrected, field, report), field = float32 of the log field minus its mask mean.  The mask is
    where the volume is finite and above `threshold` (>= 0).  report: {"mask_voxels", "levels": [{"spans",
    "iterations", "last_change"}], "field_ratio_min", "field_ratio_max", "mean_log_field"}, the ratios being exp of the
    mean-free log field's smallest and largest value inside the mask.  Raises ValueError for an empty mask.
    out: a float32 tensor [Z, Y, X] to write the corrected volume to."""
    import torch

    from . import ops

    check_levels(spans0, levels)
    tick = timer or (lambda name: None)
    u, count = ops.bias_log(volume, threshold)
    n = int(count.item())
    if n == 0:
        raise ValueError(f"no voxel above the threshold {threshold}: nothing to estimate a bias field from")
    shape = tuple(int(d) for d in volume.shape)[::-1]
    tab = tables(shape, spans0, levels, volume.device)
    lattice = torch.zeros(tab.lattice_size(), dtype=torch.float64, device=volume.device)
    tick("Z1")
    report, flat = [], False
    for level in range(int(levels)):
        rounds, change = 0, None
        part = lattice[tab.lattice_slice(level)]
        while rounds < int(iterations) and not flat:
            lo, hi = ops.bias_range(u, tab, lattice).tolist()
            if not hi > lo:                      # every mask voxel equals the field: nothing left to explain
                flat = True
                break
            counts = ops.bias_histogram(u, tab, lattice, lo, hi).cpu().numpy()
            fit = ops.bias_fit(u, tab, lattice, level, lo, hi, sharpen(counts, lo, hi))
            part += fit[2].reshape(-1)
            change = float(fit[2].abs().max())
            rounds += 1
            if change < tol:
                break
        report.append({"spans": int(spans0) << level, "iterations": rounds, "last_change": change})
    tick("fit")
    mean = float(ops.bias_mean(u, tab, lattice)[2])
    corrected, field = ops.bias_apply(volume, tab, lattice, mean, want_field=True, out=out)
    tick("Z5")
    span = [float(v) for v in torch.aminmax(field[~torch.isnan(u)])]
    summary = {"mask_voxels": n, "levels": report, "mean_log_field": mean,
               "field_ratio_min": float(np.exp(span[0])), "field_ratio_max": float(np.exp(span[1]))}
    return (corrected, field, summary) if want_field else (corrected, summary)


def correct_scan(scan, levels=DEFAULT_LEVELS, spans0=DEFAULT_SPANS, iterations=DEFAULT_ITERATIONS, tol=DEFAULT_TOL,
                 threshold=DEFAULT_THRESHOLD, want_field=False):
    """A scan [C, Z, Y, X] on the device (int16 or float32) -> (float32 [C, Z, Y, X], one report per modality); with
    want_field (corrected, fields, reports).  Each modality is corrected on its own."""
    import torch

    out = torch.empty(scan.shape, dtype=torch.float32, device=scan.device)
    fields = torch.empty_like(out) if want_field else None
    reports = []
    for c in range(scan.shape[0]):
        got = correct_volume(scan[c].contiguous(), levels, spans0, iterations, tol, threshold, want_field=want_field,
                             out=out[c])
        if want_field:
            fields[c] = got[1]
        reports.append(got[-1])
    return (out, fields, reports) if want_field else (out, reports)


# ---- command-line flags, shared by segment_scans, preprocess_dataset, compute_dataset_stats and bias_correct ----------

def add_flags(parser, switch=True):
    """--bias_correct and its settings; switch=False leaves the switch out (scripts.bias_correct always corrects)."""
    if switch:
        parser.add_argument("--bias_correct", action="store_true",
                            help="remove each modality's bias field (slow intensity inhomogeneity) on the device before "
                                 "anything else looks at the intensities (gts.bias, N4's scheme)")
    parser.add_argument("--bias_levels", type=int, default=DEFAULT_LEVELS, help="B-spline lattice levels, coarse to fine")
    parser.add_argument("--bias_spans", type=int, default=DEFAULT_SPANS,
                        help="cells per axis of the coarsest lattice; doubles with every level, at most 32")
    parser.add_argument("--bias_iterations", type=int, default=DEFAULT_ITERATIONS, help="rounds per level at the most")
    parser.add_argument("--bias_tol", type=float, default=DEFAULT_TOL,
                        help="a level ends when no control point moves by this much (log units)")
    parser.add_argument("--bias_threshold", type=float, default=DEFAULT_THRESHOLD,
                        help="voxels above this value form the mask the field is estimated from")
    parser.add_argument("--bias_report", default=None, metavar="FILE.json",
                        help="write per scan and modality the rounds run, the last change and the field's range")
    return parser


def settings_from_args(args, switch=True):
    """None with --bias_correct absent, else the keyword arguments of correct_volume.  Raises ValueError for settings
    that cannot run, before any scan is read."""
    on = bool(getattr(args, "bias_correct", False)) if switch else True
    if not on:
        changed = [name for name, default in (("bias_levels", DEFAULT_LEVELS), ("bias_spans", DEFAULT_SPANS),
                                              ("bias_iterations", DEFAULT_ITERATIONS), ("bias_tol", DEFAULT_TOL),
                                              ("bias_threshold", DEFAULT_THRESHOLD), ("bias_report", None))
                   if getattr(args, name, default) != default]
        if changed:
            raise ValueError("--" + ", --".join(changed) + " need --bias_correct")
        return None
    check_levels(args.bias_spans, args.bias_levels)
    if args.bias_iterations < 1 or not args.bias_tol >= 0 or not (args.bias_threshold >= 0 and
                                                                    np.isfinite(args.bias_threshold)):
        raise ValueError("--bias_iterations >= 1, --bias_tol >= 0 and a finite --bias_threshold >= 0 are needed")
    return dict(levels=args.bias_levels, spans0=args.bias_spans, iterations=args.bias_iterations, tol=args.bias_tol,
                threshold=args.bias_threshold)


def describe(reports):
    """One note for a scan's line of output: the widest field range over its modalities and the rounds run."""
    low = min(r["field_ratio_min"] for r in reports)
    high = max(r["field_ratio_max"] for r in reports)
    rounds = sum(level["iterations"] for r in reports for level in r["levels"])
    return f"bias: field x{low:.3f}..x{high:.3f}, {rounds} rounds"


def save_report(path, modality_extensions, settings, scans):
    """--bias_report: the settings and, per scan id, one report per modality."""
    import json
    import os

    with open(os.path.expanduser(path), "w") as f:
        json.dump({"modalities": list(modality_extensions), "settings": settings, "scans": scans}, f, indent=1)
        f.write("\n")


def correct_image(image, **settings):
    """A host image [X, Y, Z, C] (as nifti_io.read_in_patient_sample stacks a scan) -> (the corrected float32 image of
    the same layout, one report per modality): upload, correct_scan, download."""
    import torch

    host = np.ascontiguousarray(np.asarray(image, dtype=np.float32).transpose(3, 2, 1, 0))
    device = torch.device("cuda", torch.cuda.current_device())
    out, reports = correct_scan(torch.from_numpy(host).to(device), **settings)
    return np.ascontiguousarray(out.cpu().numpy().transpose(3, 2, 1, 0)), reports
