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


HEAD_SCALE = 0.8                                   # the head phantom's brain radii against make_sample's: room for the scalp
HEAD_SHELLS = (1.08, 1.23, 1.45)                   # outer radius of CSF, skull and scalp in units of the brain's
HEAD_CSF, HEAD_SKULL, HEAD_SCALP, HEAD_POCKET = 130.0, 18.0, 760.0, 35.0


def make_head_sample(seed, shape=BRATS_SHAPE):
    """(intensities float32 [X, Y, Z, 4], labels int16 [X, Y, Z] in {0, 1, 2, 4}, intracranial bool [X, Y, Z]): a scan
    with its skull on, for gts.brainmask.  The brain and tumour are make_sample's recipe with the radii scaled by
    HEAD_SCALE, inside a CSF shell, a dark skull shell and a bright scalp shell (HEAD_SHELLS: their thicknesses scale
    with the shape), two tissue bridges two voxels wide through CSF and skull (emissary-vessel style: what makes a plain
    threshold-and-largest-component keep the scalp), a dark CSF pocket inside the brain and positive noise in the air.
    intracranial = brain + CSF shell: what a brain mask should be."""
    rng = np.random.default_rng(seed)
    axes = [np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in shape]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    r = rng.uniform(0.6, 0.75, 3).astype(np.float32) * np.float32(HEAD_SCALE)
    q = (x / r[0]) ** 2 + (y / r[1]) ** 2 + (z / r[2]) ** 2
    brain = q < 1.0
    csf, skull, scalp = (q < np.float32(s * s) for s in HEAD_SHELLS)
    c = rng.uniform(-0.25, 0.25, 3).astype(np.float32) * np.float32(HEAD_SCALE)
    d2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    core, tumour, edema = d2 < 0.006, d2 < 0.02, d2 < 0.045
    pocket = ((x + c[0]) ** 2 + (y + c[1]) ** 2 + (z - np.float32(0.5) * c[2]) ** 2 < 0.004) & brain & ~edema
    ix, iy, iz = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    mid = [n // 2 for n in shape]
    two = lambda i, m: (i == m) | (i == m + 1)      # noqa: E731
    bridge = ((two(iy, mid[1]) & two(iz, mid[2]) & (ix > mid[0])) | (two(ix, mid[0]) & two(iz, mid[2]) & (iy < mid[1])))
    bridge &= skull & ~brain
    img = np.zeros(shape + (4,), dtype=np.float32)
    for m in range(4):
        base = 300.0 + 80.0 * m + 60.0 * np.sin(4.0 * x + m) * np.cos(3.0 * y)
        noise = rng.standard_normal(shape, dtype=np.float32)
        v = base + 25.0 * noise + 250.0 * edema + 200.0 * tumour
        air = np.rint(np.abs(6.0 * noise))
        head = np.where(brain | bridge, v, np.where(csf, HEAD_CSF + 10.0 * noise, np.where(
            skull, HEAD_SKULL + 4.0 * noise, HEAD_SCALP + 40.0 * m + 30.0 * noise)))
        head = np.where(pocket, HEAD_POCKET + 5.0 * noise, head)
        img[..., m] = np.where(scalp, np.rint(np.maximum(head, 1.0)), air)
    labels = np.zeros(shape, dtype=np.int16)
    labels[brain & edema] = 2
    labels[brain & tumour] = 4
    labels[brain & core] = 1
    return img, labels, np.ascontiguousarray(csf)


def write_head_sample(root, sample_id, seed, shape=BRATS_SHAPE, label_ext="_seg.nii.gz", mask_ext=None):
    """Write one head phantom as BraTS NIfTI files (int16) under root/sample_id/, with mask_ext also the true
    intracranial mask; returns (the folder, the intracranial mask)."""
    from data_processing.nifti_io import save_as_nifti

    img, labels, intracranial = make_head_sample(seed, shape)
    folder = os.path.join(root, sample_id)
    os.makedirs(folder, exist_ok=True)
    for m, ext in enumerate(MODALITY_EXTS):
        save_as_nifti(img[..., m].astype(np.int16), os.path.join(folder, sample_id + ext))
    save_as_nifti(labels, os.path.join(folder, sample_id + label_ext))
    if mask_ext:
        save_as_nifti(intracranial.astype(np.int16), os.path.join(folder, sample_id + mask_ext))
    return folder, intracranial
