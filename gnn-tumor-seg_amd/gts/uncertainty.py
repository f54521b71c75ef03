"""Voxel-wise uncertainty of an ensemble prediction, QU-BraTS style: three uint8 maps per scan
(whole tumour, tumour core, enhancing tumour), valued 0 (certain) to 100 (a coin toss), and the score of such maps
by how Dice behaves as uncertain voxels are filtered out.

The maps come from the kernels U1 / U1n (gts.ops.region_uncertainty_rows / _nodes, through
EnsemblePredictor.predict_*(..., return_uncertainty=True)); the score is one counting pass on the GPU (U2,
gts.ops.uncertainty_histogram) and a few float64 operations on its 3 x 4 x 101 counts here.

For a region, prediction mask P, truth mask G, map u and thresholds t_1 < ... < t_k (integers in 0..100):
the voxels with u <= t are kept and TP_t, FP_t, FN_t, TN_t counted on them;

    dice_t = 2 TP_t / (2 TP_t + FP_t + FN_t)       (1 when the denominator is 0)
    ftp_t  = (TP_100 - TP_t) / TP_100              (0 when TP_100 = 0): the true positives filtered out
    ftn_t  = (TN_100 - TN_t) / TN_100              (0 when TN_100 = 0)
    AUC    = trapezoid rule over (t / 100, value), divided by (t_k - t_1) / 100; the value itself when k = 1
    qu     = (auc_dice + (1 - auc_ftp) + (1 - auc_ftn)) / 3
"""
import numpy as np

REGIONS = ("WT", "CT", "ET")
MAP_NAMES = ("whole", "core", "enhance")         # the file name part of each region's map
DEFAULT_THRESHOLDS = (25, 50, 75, 100)
MAX_THRESHOLDS = 8
TP, FP, FN, TN = range(4)
FIELDS = ("qu", "dice_auc", "ftp_auc", "ftn_auc")


def map_file_names(scan_id):
    """The three files of a scan's maps, in region order: {id}_unc_whole.nii.gz, _unc_core, _unc_enhance."""
    return tuple(f"{scan_id}_unc_{name}.nii.gz" for name in MAP_NAMES)


def check_thresholds(thresholds):
    """The thresholds as a tuple of ints; ValueError unless they are 1..8 strictly ascending integers in 0..100."""
    values = tuple(thresholds)
    if not 1 <= len(values) <= MAX_THRESHOLDS:
        raise ValueError(f"between 1 and {MAX_THRESHOLDS} uncertainty thresholds are taken, got {len(values)}")
    if any(isinstance(v, bool) or int(v) != v or not 0 <= v <= 100 for v in values):
        raise ValueError(f"uncertainty thresholds are integers in 0..100, got {values}")
    values = tuple(int(v) for v in values)
    if any(b <= a for a, b in zip(values, values[1:])):
        raise ValueError(f"uncertainty thresholds must be strictly ascending, got {values}")
    return values


def _auc(x, y):
    if len(x) == 1:
        return float(y[0])
    area = float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0))
    return area / float(x[-1] - x[0])


def qu_from_histogram(hist, thresholds=DEFAULT_THRESHOLDS):
    """{region: {qu, dice_auc, ftp_auc, ftn_auc, dice: [...], ftp: [...], ftn: [...]}} from the counts `hist`
    [3 regions, 4 outcomes (TP, FP, FN, TN), >= 101 bins] (what gts.ops.uncertainty_histogram returns; anything
    array-like).  Pure numpy float64."""
    thresholds = check_thresholds(thresholds)
    counts = np.asarray(hist.cpu() if hasattr(hist, "cpu") else hist).astype(np.int64)
    if counts.ndim != 3 or counts.shape[:2] != (3, 4) or counts.shape[2] < 101:
        raise ValueError(f"the histogram must be [3, 4, >= 101], got {counts.shape}")
    kept = np.cumsum(counts[:, :, :101], axis=2)               # [r, outcome, t]: voxels with u <= t
    x = np.array(thresholds, dtype=np.float64) / 100.0
    scores = {}
    for r, region in enumerate(REGIONS):
        at = kept[r][:, list(thresholds)].astype(np.float64)   # [outcome, k]
        all_tp, all_tn = float(kept[r, TP, 100]), float(kept[r, TN, 100])
        denom = 2.0 * at[TP] + at[FP] + at[FN]
        dice = np.where(denom > 0, 2.0 * at[TP] / np.where(denom > 0, denom, 1.0), 1.0)
        ftp = (all_tp - at[TP]) / all_tp if all_tp > 0 else np.zeros_like(x)
        ftn = (all_tn - at[TN]) / all_tn if all_tn > 0 else np.zeros_like(x)
        dice_auc, ftp_auc, ftn_auc = _auc(x, dice), _auc(x, ftp), _auc(x, ftn)
        scores[region] = {"qu": (dice_auc + (1.0 - ftp_auc) + (1.0 - ftn_auc)) / 3.0, "dice_auc": dice_auc,
                          "ftp_auc": ftp_auc, "ftn_auc": ftn_auc, "dice": [float(v) for v in dice],
                          "ftp": [float(v) for v in ftp], "ftn": [float(v) for v in ftn]}
    return scores


def qu_scores(pred, truth, unc, thresholds=DEFAULT_THRESHOLDS):
    """qu_from_histogram of one scan: pred / truth int16 internal labels and unc uint8 [3, ...] over the same
    voxels, tensors on the GPU.  One streaming pass (U2); GtsError for a map value above 100 or a label outside
    0..3."""
    from . import ops

    thresholds = check_thresholds(thresholds)
    return qu_from_histogram(ops.uncertainty_histogram(pred, truth, unc), thresholds)
