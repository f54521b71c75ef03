"""numpy restatements of the two definitions of DESIGN.md §4u: the uncertainty of a row of class sums, and the
QU score computed from voxel masks per threshold (never from a histogram)."""
import numpy as np

REGIONS = ("WT", "CT", "ET")
REGION_CLASSES = ((1, 2, 3), (2, 3), (3,))


def row_uncertainty(sums, terms):
    """uint8 [3, rows] of fp32 class sums [rows, 4] over `terms` terms: float64 add in ascending class order,
    divide, clamp, min, multiply, rint (round-half-to-even); a NaN probability gives 100."""
    sums = np.asarray(sums)
    assert sums.dtype == np.float32 and sums.ndim == 2 and sums.shape[1] == 4
    s = sums.astype(np.float64)
    out = np.empty((3, len(s)), dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for r, classes in enumerate(REGION_CLASSES):
            total = s[:, classes[0]].copy()
            for c in classes[1:]:
                total = total + s[:, c]
            p = total / np.float64(terms)
            nan = np.isnan(p)
            p = np.minimum(np.maximum(np.where(nan, 0.5, p), 0.0), 1.0)
            u = np.rint(200.0 * np.minimum(p, 1.0 - p))
            out[r] = np.where(nan, 100.0, u).astype(np.uint8)
    return out


def region_masks(labels):
    labels = np.asarray(labels)
    return [labels != 0, (labels == 2) | (labels == 3), labels == 3]


def _auc(x, y):
    if len(x) == 1:
        return float(y[0])
    area = 0.0
    for k in range(len(x) - 1):
        area += (x[k + 1] - x[k]) * (y[k] + y[k + 1]) / 2.0
    return area / (x[-1] - x[0])


def qu_scores(pred, truth, unc, thresholds=(25, 50, 75, 100)):
    """{region: {qu, dice_auc, ftp_auc, ftn_auc, dice, ftp, ftn}} from label arrays (internal labels 0..3) and
    unc uint8 [3, ...] over the same voxels, with boolean masks per threshold."""
    pred, truth, unc = np.asarray(pred).reshape(-1), np.asarray(truth).reshape(-1), np.asarray(unc).reshape(3, -1)
    x = [t / 100.0 for t in thresholds]
    scores = {}
    for r, (P, G) in enumerate(zip(region_masks(pred), region_masks(truth))):
        everything = unc[r] <= 100
        all_tp, all_tn = int((P & G & everything).sum()), int((~P & ~G & everything).sum())
        dice, ftp, ftn = [], [], []
        for t in thresholds:
            kept = unc[r] <= t
            tp, fp = int((P & G & kept).sum()), int((P & ~G & kept).sum())
            fn, tn = int((~P & G & kept).sum()), int((~P & ~G & kept).sum())
            denom = 2 * tp + fp + fn
            dice.append(2.0 * tp / denom if denom else 1.0)
            ftp.append((all_tp - tp) / all_tp if all_tp else 0.0)
            ftn.append((all_tn - tn) / all_tn if all_tn else 0.0)
        dice_auc, ftp_auc, ftn_auc = _auc(x, dice), _auc(x, ftp), _auc(x, ftn)
        scores[REGIONS[r]] = {"qu": (dice_auc + (1.0 - ftp_auc) + (1.0 - ftn_auc)) / 3.0, "dice_auc": dice_auc,
                              "ftp_auc": ftp_auc, "ftn_auc": ftn_auc, "dice": dice, "ftp": ftp, "ftn": ftn}
    return scores


def histogram(pred, truth, unc):
    """int64 [3, 4, 102]: per region and outcome (TP, FP, FN, TN) the voxels at each map value; bin 101 = above 100."""
    pred, truth, unc = np.asarray(pred).reshape(-1), np.asarray(truth).reshape(-1), np.asarray(unc).reshape(3, -1)
    hist = np.zeros((3, 4, 102), dtype=np.int64)
    for r, (P, G) in enumerate(zip(region_masks(pred), region_masks(truth))):
        bins = np.minimum(unc[r].astype(np.int64), 101)
        for o, mask in enumerate((P & G, P & ~G, ~P & G, ~P & ~G)):
            hist[r, o] = np.bincount(bins[mask], minlength=102)
    return hist


def random_case(n, seed, tumour=0.3):
    """(pred, truth int16 [n], unc uint8 [3, n]) with every outcome and every map value present for large n."""
    rng = np.random.default_rng(seed)
    truth = np.where(rng.random(n) < tumour, rng.integers(1, 4, n), 0).astype(np.int16)
    pred = np.where(rng.random(n) < 0.8, truth, rng.integers(0, 4, n)).astype(np.int16)
    unc = rng.integers(0, 101, (3, n)).astype(np.uint8)
    unc[:, rng.random(n) < 0.4] = 0
    return pred, truth, unc
