"""Tiny synthetic samples for the refinement-CNN tests: processed sample folders (`{id}_input.nii.gz`,
`{id}_label.nii.gz`) and a logits folder (`{id}_logits.nii.gz`) as generate_gnn_predictions writes it."""
import os

import numpy as np

from data_processing import nifti_io


def make(seed, shape=(20, 18, 14)):
    """(image float32 [X, Y, Z, 4], labels int16 [X, Y, Z] in 0..3, logits float32 [X, Y, Z, 4])."""
    rng = np.random.default_rng(seed)
    axes = [np.linspace(-1, 1, n) for n in shape]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    c = rng.uniform(-0.2, 0.2, 3)
    d2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    lab = np.zeros(shape, dtype=np.int16)
    lab[d2 < 0.35] = 1
    lab[d2 < 0.15] = 2
    lab[d2 < 0.05] = 3
    img = (rng.standard_normal(shape + (4,)) + lab[..., None] * 0.5).astype(np.float32)
    logits = rng.standard_normal(shape + (4,)).astype(np.float32)
    logits[..., 0] += 1.0
    noisy = np.clip(lab + rng.integers(-1, 2, shape) * (rng.random(shape) < 0.2), 0, 3)
    logits[noisy > 0, 0] -= 2.0
    for k in range(1, 4):
        logits[noisy == k, k] += 2.0
    return img, lab, logits


def write(data_dir, logit_dir, ids, shape=(20, 18, 14), missing_logits=()):
    os.makedirs(logit_dir, exist_ok=True)
    for i, mri in enumerate(ids):
        img, lab, logits = make(100 + i, shape)
        folder = os.path.join(data_dir, mri)
        os.makedirs(folder, exist_ok=True)
        nifti_io.save_as_nifti(img, os.path.join(folder, f"{mri}_input.nii.gz"))
        nifti_io.save_as_nifti(lab, os.path.join(folder, f"{mri}_label.nii.gz"))
        if mri not in missing_logits:
            nifti_io.save_as_nifti(logits, os.path.join(logit_dir, f"{mri}_logits.nii.gz"))
