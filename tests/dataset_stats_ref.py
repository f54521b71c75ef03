"""Numpy restatement of one scan's share of the reference's DataPreprocessor.compute_dataset_stats
(scripts/preprocess_dataset.py:93-115), in two forms:

  reference_form  float32 throughout, as numpy evaluates the reference's lines: np.mean / np.std over the
                  [n, 4] float32 array accumulate in float32, row after row;
  exact_form      the same mask, tops and float32 division, then float64 before mean and std: the
                  statistics of the normalized values themselves, to float64 accuracy.

Volumes come from gts.synth_mri.make_sample (seeded), so fixtures store only their digests.
"""
import hashlib

import numpy as np

QUANTILE = 0.995
# (seed, shape) of the fixture's scans: one at BraTS size, the rest small
FIXTURE_SCANS = ((7, (240, 240, 155)), (11, (48, 40, 32)), (12, (33, 17, 9)), (13, (64, 60, 40)), (14, (24, 30, 20)))


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def stack(vols):
    """Four [X, Y, Z] volumes -> float32 [X, Y, Z, 4], as nifti_io.read_in_patient_sample gives a scan."""
    return np.stack([np.asarray(v, dtype=np.float32) for v in vols], axis=3)


def healthy_mask(img, lab):
    return np.logical_and(img[:, :, :, 0] > 0.001, lab == 0)


def tops(flat):
    return np.quantile(flat, QUANTILE, axis=0).astype(np.float32)


def reference_form(img, lab):
    """(mu, sigma) float32 [4]: the reference's lines 102-106 with image_processing.normalize_img's."""
    flat = img[healthy_mask(img, lab)]
    flat = flat / tops(flat)
    return np.mean(flat, axis=0), np.std(flat, axis=0)


def exact_form(img, lab):
    """(n, top float32 [4], mean float64 [4], std float64 [4])."""
    flat = img[healthy_mask(img, lab)]
    top = tops(flat)
    y = (flat / top).astype(np.float64)
    return flat.shape[0], top, np.mean(y, axis=0), np.std(y, axis=0)


def ulp32(x):
    """Spacing of float32 at |x| (per element), as float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)
