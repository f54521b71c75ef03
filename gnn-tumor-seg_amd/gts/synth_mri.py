"""Seeded synthetic BraTS-like MRI samples for tests and tools/measure_graphgen.py.

Four modalities at 240 x 240 x 155 (flair, t1, t1ce, t2): a noisy ellipsoid "brain" on a zero
background with a tumour blob, intensities on an int16-like scale as BraTS ships them, and a
label volume in BraTS coding {0, 1, 2, 4}.  Not the benchmark's generator (gts/synth.py).
"""
import os

import numpy as np

BRATS_SHAPE = (240, 240, 155)
MODALITY_EXTS = ("_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz")


def make_sample(seed, shape=BRATS_SHAPE):
    """(intensities float32 [X, Y, Z, 4], labels int16 [X, Y, Z] in {0, 1, 2, 4})."""
    rng = np.random.default_rng(seed)
    axes = [np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in shape]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    r = rng.uniform(0.6, 0.75, 3).astype(np.float32)
    brain = (x / r[0]) ** 2 + (y / r[1]) ** 2 + (z / r[2]) ** 2 < 1.0
    c = rng.uniform(-0.25, 0.25, 3).astype(np.float32)
    d2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    core, tumour, edema = d2 < 0.006, d2 < 0.02, d2 < 0.045
    img = np.zeros(shape + (4,), dtype=np.float32)
    for m in range(4):
        base = 300.0 + 80.0 * m + 60.0 * np.sin(4.0 * x + m) * np.cos(3.0 * y)
        v = base + 25.0 * rng.standard_normal(shape, dtype=np.float32) + 250.0 * edema + 200.0 * tumour
        img[..., m] = np.where(brain, np.rint(np.maximum(v, 1.0)), 0.0)
    labels = np.zeros(shape, dtype=np.int16)
    labels[brain & edema] = 2
    labels[brain & tumour] = 4
    labels[brain & core] = 1
    return img, labels


def write_sample(root, sample_id, seed, shape=BRATS_SHAPE, label_ext="_seg.nii.gz"):
    """Write one sample as BraTS NIfTI files under root/sample_id/; returns the folder."""
    from data_processing.nifti_io import save_as_nifti

    img, labels = make_sample(seed, shape)
    folder = os.path.join(root, sample_id)
    os.makedirs(folder, exist_ok=True)
    for m, ext in enumerate(MODALITY_EXTS):
        save_as_nifti(img[..., m].astype(np.int16), os.path.join(folder, sample_id + ext))
    save_as_nifti(labels, os.path.join(folder, sample_id + label_ext))
    return folder


def make_prediction(seed, shape=BRATS_SHAPE, n_blobs=3, salt=0.001):
    """A predicted label volume as a supervoxel GNN leaves it, int16 in BraTS coding: `n_blobs` nested
    tumour blobs (edema 2 around enhancing 4 around core 1) plus salt noise, a fraction `salt` of the
    voxels set to a random tumour label (the lone false positives a connected-component filter removes)."""
    rng = np.random.default_rng(seed)
    axes = [np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in shape]
    labels = np.zeros(shape, dtype=np.int16)
    for _ in range(n_blobs):
        c = rng.uniform(-0.45, 0.45, 3).astype(np.float32)
        s = rng.uniform(0.6, 1.4, 3).astype(np.float32)
        d2 = (((axes[0] - c[0]) / s[0]) ** 2)[:, None, None] + (((axes[1] - c[1]) / s[1]) ** 2)[None, :, None] \
            + (((axes[2] - c[2]) / s[2]) ** 2)[None, None, :]
        for radius2, lab in ((0.045, 2), (0.02, 4), (0.006, 1)):
            labels[d2 < radius2] = lab
    noise = rng.random(shape, dtype=np.float32) < salt
    labels[noise] = rng.choice(np.array([1, 2, 4], dtype=np.int16), size=int(noise.sum()))
    return labels
