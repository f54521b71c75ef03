"""The spacing-aware HD95 and surface Dice of gts.metrics in scipy and numpy, straight from the
definition: borders from binary_erosion as model/evaluation.py takes them, distances from
distance_transform_edt(sampling=units), HD95 from np.percentile of the distances in mm, surface Dice from exact
integer comparisons.  The integer units of a spacing are restated here, not imported from the code under test.

Labels are internal (0 healthy, 1 edema, 2 NET, 3 ET); regions WT (v != 0), CT (v in {2, 3}), ET (v == 3).
"""
import math

import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

from tests import lesionwise_ref

REGIONS = lesionwise_ref.REGIONS
BRUTE_FORCE_VOXELS = 24 ** 3        # volumes up to this size cross-check scipy against a brute-force minimum


def units_of(spacing_mm):
    """(units, g): the spacing in steps of 1e-4 mm divided by g, the gcd of the three and of 10000."""
    steps = [int(round(float(s) * 10000)) for s in spacing_mm]
    g = math.gcd(*steps, 10000)
    return tuple(u // g for u in steps), g


def steps_of(tolerance_mm):
    return int(round(float(tolerance_mm) * 10000))


def border(mask):
    mask = np.asarray(mask, dtype=bool)
    return mask ^ binary_erosion(mask, structure=generate_binary_structure(mask.ndim, 1), iterations=1)


def blobs(shape, rng, n_blobs=4, labels=(1, 2, 3)):
    """Nested tumour-like regions: spheres of label 1 holding smaller ones of 2 and 3 (the volumes of
    tests/test_gpu_hd95.py)."""
    grid = np.indices(shape).reshape(len(shape), -1).T.astype(np.float64)
    vol = np.zeros(int(np.prod(shape)), dtype=np.int16)
    for _ in range(n_blobs):
        centre = rng.uniform(0, shape)
        radius = rng.uniform(0.15, 0.35) * min([s for s in shape if s > 1] or [1]) + 1
        dist = np.sqrt(((grid - centre) ** 2).sum(axis=1))
        for k, lab in enumerate(labels):
            vol[dist < radius * (1 - 0.3 * k)] = lab
    return vol.reshape(shape)


def directed(from_border, to_border, units):
    """(distances, D2) from every voxel of from_border to the nearest voxel of to_border: scipy's float64
    distances under sampling = units, and the exact int64 squared distances to the feature scipy names."""
    dist, nearest = distance_transform_edt(~to_border, sampling=[float(u) for u in units], return_indices=True)
    at = np.nonzero(from_border)
    d2 = np.zeros(len(at[0]), dtype=np.int64)
    for a in range(3):
        d2 += (np.int64(units[a]) * (at[a].astype(np.int64) - nearest[a][at].astype(np.int64))) ** 2
    dist = dist[at]
    assert np.array_equal(dist, np.sqrt(d2.astype(np.float64))), "scipy's distance is not sqrt of the exact integer"
    if from_border.size <= BRUTE_FORCE_VOXELS:
        p = np.stack(at, axis=1).astype(np.int64) * np.asarray(units, dtype=np.int64)
        q = np.argwhere(to_border).astype(np.int64) * np.asarray(units, dtype=np.int64)
        brute = np.array([((q - row) ** 2).sum(axis=1).min() for row in p], dtype=np.int64).reshape(-1)
        assert np.array_equal(brute, d2), "scipy's nearest feature is not the brute-force minimum"
    return dist, d2


def mask_scores(pred_mask, truth_mask, spacing_mm, tolerances_mm=()):
    """(hd95 in mm, [NSD per tolerance]) of two boolean volumes; 0 / 300 and 1.0 / 0.0 for absent masks."""
    pred_mask, truth_mask = np.asarray(pred_mask, dtype=bool), np.asarray(truth_mask, dtype=bool)
    if not pred_mask.any() or not truth_mask.any():
        both_absent = not pred_mask.any() and not truth_mask.any()
        return (0.0 if both_absent else 300.0), [1.0 if both_absent else 0.0] * len(tolerances_mm)
    units, g = units_of(spacing_mm)
    bp, bt = border(pred_mask), border(truth_mask)
    dist_p, d2_p = directed(bp, bt, units)
    dist_t, d2_t = directed(bt, bp, units)
    hd = float(np.percentile(np.hstack((dist_p, dist_t)) * (g / 10000.0), 95))
    nsd = []
    for tol in tolerances_mm:
        t = steps_of(tol)
        within = sum(int(d) * g * g <= t * t for d in d2_p.tolist() + d2_t.tolist())      # exact Python integers
        nsd.append(within / (len(d2_p) + len(d2_t)))
    return hd, nsd


def scores(pred, truth, spacing_mm, tolerances_mm=()):
    """([hd95 mm per region], [[NSD per region] per tolerance]) of two label volumes."""
    per_region = [mask_scores(lesionwise_ref.region_mask(pred, r), lesionwise_ref.region_mask(truth, r), spacing_mm,
                              tolerances_mm) for r in REGIONS]
    return [hd for hd, _ in per_region], [[nsd[k] for _, nsd in per_region] for k in range(len(tolerances_mm))]


def lesionwise_scores(pred, truth, spacing_mm, tolerances_mm=(), dilation=3, min_lesion_voxels=50):
    """tests/lesionwise_ref.lesionwise_scores with distances in mm: hd95 and each lesion's hd95 from mask_scores,
    `nsd` and `lw_nsd` per tolerance; a missed lesion and a false-positive component count 374 and 0."""
    from model import evaluation

    pred, truth = np.asarray(pred), np.asarray(truth)
    n_tol = len(tolerances_mm)
    dices = evaluation.calculate_node_dices(pred, truth)
    out = {}
    for r, region in enumerate(REGIONS):
        P, G = lesionwise_ref.region_mask(pred, region), lesionwise_ref.region_mask(truth, region)
        t = lesionwise_ref.region_tables(P, G, dilation)
        lesions, dice_sum, hd_sum, nsd_sum, n_scored, n_fn = [], 0.0, 0.0, [0.0] * n_tol, 0, 0
        for vol, tp, m, (M_k, G_k) in zip(t["vol"], t["tp"], t["matched_voxels"], t["masks"]):
            scored = vol > min_lesion_voxels
            dice = hd = nsd = None
            if scored:
                if m == 0:
                    dice, hd, nsd = 0.0, lesionwise_ref.PENALTY_HD95, [0.0] * n_tol
                    n_fn += 1
                else:
                    dice = (2 * tp) / (m + vol)
                    hd, nsd = mask_scores(M_k, G_k, spacing_mm, tolerances_mm)
                dice_sum += dice
                hd_sum += hd
                nsd_sum = [a + b for a, b in zip(nsd_sum, nsd)]
                n_scored += 1
            lesions.append(dict(vol=vol, tp=tp, matched_voxels=m, scored=scored, dice=dice, hd95=hd, nsd=nsd))
        divisor = n_scored + t["n_fp"]
        hd, nsd = mask_scores(P, G, spacing_mm, tolerances_mm)
        out[region] = dict(
            dice=float(dices[r]), hd95=hd, nsd=nsd,
            lw_dice=dice_sum / divisor if divisor else 1.0,
            lw_hd95=(hd_sum + lesionwise_ref.PENALTY_HD95 * t["n_fp"]) / divisor if divisor else 0.0,
            lw_nsd=[a / divisor for a in nsd_sum] if divisor else [1.0] * n_tol,
            n_lesions=len(lesions), n_scored=n_scored, n_fp=t["n_fp"], n_fn=n_fn, lesions=lesions,
            lesion_roots=t["lesion_roots"])
    return out
