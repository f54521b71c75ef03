"""The lesion-wise Dice / HD95 of gts.lesionwise in scipy and numpy, written straight from the
definition: per-lesion dilation and np.isin, not the identities the device route rests on, so that it checks them.

Labels are internal (0 healthy, 1 edema, 2 NET, 3 ET); regions WT (v != 0), CT (v in {2, 3}), ET (v == 3).
"""
import numpy as np
from scipy import ndimage

from model import evaluation

REGIONS = ("WT", "CT", "ET")
PENALTY_HD95 = 374.0
S26 = ndimage.generate_binary_structure(3, 3)
S18 = ndimage.generate_binary_structure(3, 2)


def region_mask(labels, region):
    labels = np.asarray(labels)
    return {"WT": labels != 0, "CT": np.isin(labels, [2, 3]), "ET": labels == 3}[region]


def dilate(mask, n):
    """n iterations of the 18-neighbour structure, clipped at the volume (border_value 0)."""
    mask = np.asarray(mask, dtype=bool)
    return ndimage.binary_dilation(mask, S18, iterations=n, border_value=0) if n > 0 else mask.copy()


def closed_form_footprint(n):
    """{ o : max |o_i| <= n, sum |o_i| <= 2 n } as a boolean cube of side 2 n + 1."""
    o = np.abs(np.arange(-n, n + 1))
    return (o[:, None, None] + o[None, :, None] + o[None, None, :]) <= 2 * n


def dilate_closed_form(mask, n):
    return ndimage.binary_dilation(np.asarray(mask, dtype=bool), closed_form_footprint(n), border_value=0)


def region_tables(pred_mask, truth_mask, dilation=3):
    """Steps 1-5 without the HD95.  dict: lesion_roots (1 + smallest C-order index of each D_k, ascending),
    vol, tp, matched_voxels, n_fp, comp_sizes (in scipy's order), masks = [(M_k, G_k)]."""
    P, G = np.asarray(pred_mask, dtype=bool), np.asarray(truth_mask, dtype=bool)
    D = dilate(G, dilation)
    d_lab, n_lesions = ndimage.label(D, S26)
    p_lab, n_comps = ndimage.label(P, S26)
    matched_any = np.zeros(n_comps + 1, dtype=bool)
    out = dict(lesion_roots=[], vol=[], tp=[], matched_voxels=[], masks=[])
    for k in range(1, n_lesions + 1):
        D_k = d_lab == k
        G_k = G & D_k
        # the definition's own D_k: the dilation of this lesion alone
        assert np.array_equal(dilate(G_k, dilation), D_k), "D_k is not the dilation of G_k"
        comps = np.unique(p_lab[D_k & P])
        matched_any[comps] = True
        M_k = np.isin(p_lab, comps) & P
        out["lesion_roots"].append(int(np.flatnonzero(D_k.ravel())[0]) + 1)
        out["vol"].append(int(G_k.sum()))
        out["tp"].append(int((P & G_k).sum()))
        out["matched_voxels"].append(int(M_k.sum()))
        out["masks"].append((M_k, G_k))
    out["n_fp"] = int(n_comps - matched_any[1:].sum())
    out["comp_sizes"] = np.bincount(p_lab.ravel(), minlength=n_comps + 1)[1:].tolist()
    return out


def region_scores(pred_mask, truth_mask, dilation=3, min_lesion_voxels=50):
    """Steps 1-7 for one region's masks (without the legacy numbers)."""
    t = region_tables(pred_mask, truth_mask, dilation)
    lesions, dice_sum, hd_sum, n_scored, n_fn = [], 0.0, 0.0, 0, 0
    for vol, tp, m, (M_k, G_k) in zip(t["vol"], t["tp"], t["matched_voxels"], t["masks"]):
        scored = vol > min_lesion_voxels
        dice = hd = None
        if scored:
            if m == 0:
                dice, hd = 0.0, PENALTY_HD95
                n_fn += 1
            else:
                dice = (2 * tp) / (m + vol)
                hd = float(evaluation.hd95(M_k, G_k))
            dice_sum += dice
            hd_sum += hd
            n_scored += 1
        lesions.append(dict(vol=vol, tp=tp, matched_voxels=m, scored=scored, dice=dice, hd95=hd))
    n_fp = t["n_fp"]
    if n_scored + n_fp == 0:
        lw_dice, lw_hd95 = 1.0, 0.0
    else:
        lw_dice = dice_sum / (n_scored + n_fp)
        lw_hd95 = (hd_sum + PENALTY_HD95 * n_fp) / (n_scored + n_fp)
    return dict(lw_dice=lw_dice, lw_hd95=lw_hd95, n_lesions=len(lesions), n_scored=n_scored, n_fp=n_fp, n_fn=n_fn,
                lesions=lesions, lesion_roots=t["lesion_roots"])


def lesionwise_scores(pred, truth, dilation=3, min_lesion_voxels=50):
    """{region: region_scores + the legacy dice and hd95} of two internal-label volumes."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    legacy = evaluation.calculate_brats_metrics(pred, truth)
    out = {}
    for r, region in enumerate(REGIONS):
        rec = region_scores(region_mask(pred, region), region_mask(truth, region), dilation, min_lesion_voxels)
        rec["dice"], rec["hd95"] = float(legacy[r]), float(legacy[3 + r])
        out[region] = rec
    return out


def blobs_and_salt(shape, seed, n_blobs=3, salt=0.002, shift=2):
    """(pred, truth) internal-label volumes: nested ellipsoid blobs in the truth, the prediction a shifted copy
    with one blob dropped, one satellite island added and salt noise; the truth also holds three specks."""
    rng = np.random.default_rng(seed)
    axes = [np.arange(n, dtype=np.float64) for n in shape]

    def paint(vol, centre, radii, scale=1.0):
        d2 = sum((((a - c) / (r * scale)) ** 2).reshape([-1 if i == k else 1 for i in range(3)])
                 for k, (a, c, r) in enumerate(zip(axes, centre, radii)))
        for bound, lab in ((1.0, 1), (0.5, 3), (0.15, 2)):
            vol[d2 < bound] = lab

    truth = np.zeros(shape, dtype=np.int16)
    pred = np.zeros(shape, dtype=np.int16)
    for b in range(n_blobs):
        centre = [rng.uniform(0.15, 0.85) * n for n in shape]
        radii = [rng.uniform(0.08, 0.2) * n + 1.5 for n in shape]
        paint(truth, centre, radii)
        if b != 1:
            paint(pred, [c + rng.uniform(-shift, shift) for c in centre], radii, rng.uniform(0.8, 1.15))
    paint(pred, [rng.uniform(0.1, 0.9) * n for n in shape], [2.5, 2.0, 2.5])
    noise = rng.random(shape) < salt
    pred[noise] = rng.integers(1, 4, int(noise.sum()))
    for _ in range(3):                                   # ground-truth specks: lesions too small to be scored
        at = tuple(int(rng.integers(0, n - 1)) for n in shape)
        truth[at[0]:at[0] + 2, at[1]:at[1] + 2, at[2]] = rng.integers(1, 4)
    return pred, truth
