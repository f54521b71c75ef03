"""Minimal NIfTI-1 (.nii / .nii.gz) reader and writer.

The reference goes through nibabel (data_processing/nifti_io.py:42-57), which is not
available here; this module writes/reads single-file NIfTI-1 volumes with the fixed BraTS
affine the reference uses and returns arrays the same way (`np.array(dataobj, dtype)`).
Header layout: the NIfTI-1 specification (nifti1.h), field by field; pinned byte for byte by
tests/test_nifti_bytes.py against a header assembled by hand from that specification.
PARITY UNPINNED against nibabel itself (absent; the reference holds no .nii fixture): fields
the specification leaves to the writer (scl_slope 1.0 here, NaN in nibabel — both mean "no
scaling"; descrip) may differ; every reader-relevant field is the spec's.
"""
import gzip
import os
import struct

import numpy as np

BRATS_AFFINE = np.array([
    [-1.0, -0.0, -0.0, -0.0],
    [-0.0, -1.0, -0.0, 239.0],
    [0.0, 0.0, 1.0, 0.0],
    [0.0, 0.0, 0.0, 1.0],
])

# NIfTI datatype code <-> numpy dtype, bits per voxel
_CODES = {
    2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64,
    256: np.int8, 512: np.uint16, 768: np.uint32, 1024: np.int64, 1280: np.uint64,
}
_BY_DTYPE = {np.dtype(v): k for k, v in _CODES.items()}


def _quaternion_bcd(affine):
    """(b, c, d) of the unit quaternion of the affine's rotation part (NIfTI-1 spec, nifti1.h
    "METHOD 2"; a = sqrt(1 - b^2 - c^2 - d^2) >= 0).  Columns are normalised; an improper
    rotation has its third column flipped (that sign is qfac = pixdim[0])."""
    r = np.array(affine, dtype=np.float64)[:3, :3]
    r = r / np.sqrt((r * r).sum(axis=0))
    if np.linalg.det(r) < 0:
        r[:, 2] = -r[:, 2]
    a = r[0, 0] + r[1, 1] + r[2, 2] + 1.0
    if a > 0.5:
        a = 0.5 * np.sqrt(a)
        b, c, d = 0.25 * (r[2, 1] - r[1, 2]) / a, 0.25 * (r[0, 2] - r[2, 0]) / a, 0.25 * (r[1, 0] - r[0, 1]) / a
    else:
        xd, yd, zd = 1.0 + r[0, 0] - (r[1, 1] + r[2, 2]), 1.0 + r[1, 1] - (r[0, 0] + r[2, 2]), \
            1.0 + r[2, 2] - (r[0, 0] + r[1, 1])
        if xd > 1.0:
            b = 0.5 * np.sqrt(xd)
            c, d, a = 0.25 * (r[0, 1] + r[1, 0]) / b, 0.25 * (r[0, 2] + r[2, 0]) / b, 0.25 * (r[2, 1] - r[1, 2]) / b
        elif yd > 1.0:
            c = 0.5 * np.sqrt(yd)
            b, d, a = 0.25 * (r[0, 1] + r[1, 0]) / c, 0.25 * (r[1, 2] + r[2, 1]) / c, 0.25 * (r[0, 2] - r[2, 0]) / c
        else:
            d = 0.5 * np.sqrt(zd)
            b, c, a = 0.25 * (r[0, 2] + r[2, 0]) / d, 0.25 * (r[1, 2] + r[2, 1]) / d, 0.25 * (r[1, 0] - r[0, 1]) / d
        if a < 0.0:
            b, c, d = -b, -c, -d
    return float(b), float(c), float(d)


def _open(fp, mode):
    if not str(fp).endswith(".gz"):
        return open(fp, mode)
    # no time stamp in the gzip header: the same volume gives the same bytes whenever it is written (two datasets built from
    # the same scans are compared byte for byte, and a second's tick between the two writes must not tell them apart)
    return gzip.GzipFile(fp, mode, mtime=0) if "w" in mode else gzip.open(fp, mode)


def save_as_nifti(img, fp, affine=BRATS_AFFINE):
    img = np.asarray(img)
    if img.dtype == np.bool_:
        img = img.astype(np.uint8)
    if img.dtype not in _BY_DTYPE:
        raise ValueError(f"unsupported dtype for NIfTI: {img.dtype}")
    if not 1 <= img.ndim <= 7:
        raise ValueError("NIfTI supports 1 to 7 dimensions")
    dim = [img.ndim] + list(img.shape) + [1] * (7 - img.ndim)
    affine = np.asarray(affine, dtype=np.float64)
    pixdim = [1.0] * 8
    pixdim[0] = -1.0 if np.linalg.det(affine[:3, :3]) < 0 else 1.0
    pixdim[1:4] = [float(n) for n in np.sqrt((affine[:3, :3] ** 2).sum(axis=0))]   # voxel spacings: the column norms
    hdr = bytearray(348)
    struct.pack_into("<i", hdr, 0, 348)
    hdr[38:39] = b"r"                            # `regular`: unused by NIfTI-1, set by Analyze-lineage writers
    struct.pack_into("<8h", hdr, 40, *dim)
    struct.pack_into("<hh", hdr, 70, _BY_DTYPE[img.dtype], img.dtype.itemsize * 8)
    struct.pack_into("<8f", hdr, 76, *pixdim)
    struct.pack_into("<f", hdr, 108, 352.0)      # vox_offset
    struct.pack_into("<ff", hdr, 112, 1.0, 0.0)  # scl_slope, scl_inter
    struct.pack_into("<hh", hdr, 252, 0, 2)      # qform_code 0 (unknown), sform_code 2 (aligned)
    # the quaternion / offset fields carry the same transform (ignored while qform_code is 0)
    struct.pack_into("<3f", hdr, 256, *_quaternion_bcd(affine))
    struct.pack_into("<3f", hdr, 268, *[float(affine[r][3]) for r in range(3)])
    for r in range(3):
        struct.pack_into("<4f", hdr, 280 + 16 * r, *[float(x) for x in affine[r]])
    hdr[344:348] = b"n+1\0"
    with _open(fp, "wb") as f:
        f.write(bytes(hdr) + b"\0\0\0\0")
        f.write(np.asfortranarray(img).tobytes(order="F"))


def read_nifti(fp, data_type):
    with _open(fp, "rb") as f:
        raw = f.read()
    endian = "<" if struct.unpack_from("<i", raw, 0)[0] == 348 else ">"
    dim = struct.unpack_from(endian + "8h", raw, 40)
    code, _bits = struct.unpack_from(endian + "hh", raw, 70)
    if code not in _CODES:
        raise ValueError(f"unsupported NIfTI datatype code {code}")
    vox_offset = int(struct.unpack_from(endian + "f", raw, 108)[0])
    slope, inter = struct.unpack_from(endian + "ff", raw, 112)
    shape = tuple(dim[1:1 + dim[0]])
    dt = np.dtype(_CODES[code]).newbyteorder(endian)
    data = np.frombuffer(raw, dtype=dt, count=int(np.prod(shape)), offset=max(vox_offset, 352))
    data = data.reshape(shape, order="F")
    if slope not in (0.0, 1.0) or inter != 0.0:
        if slope != 0.0 and not np.isnan(slope):
            data = data * slope + inter
    return np.array(data, dtype=data_type)


def _quaternion_rotation(b, c, d):
    """The rotation matrix of the unit quaternion (a, b, c, d), a = sqrt(1 - b^2 - c^2 - d^2) >= 0 (nifti1.h
    "METHOD 2"): the inverse of _quaternion_bcd."""
    a = np.sqrt(max(0.0, 1.0 - (b * b + c * c + d * d)))
    return np.array([
        [a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
        [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
        [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b],
    ])


def read_affine(fp):
    """(affine, source): the 4x4 float64 voxel-to-world transform of a NIfTI-1 file and the header field it came
    from, by the specification's order of preference: "sform" (sform_code > 0: the srow_* rows), else "qform"
    (qform_code > 0: quaternion, pixdim[1..3], qfac = pixdim[0] with 0 counting as +1, and the qoffsets), else
    "pixdim" (diag(pixdim[1..3]), origin 0)."""
    with _open(fp, "rb") as f:
        raw = f.read(348)
    if len(raw) < 348:
        raise ValueError(f"{fp}: shorter than a NIfTI-1 header")
    endian = "<" if struct.unpack_from("<i", raw, 0)[0] == 348 else ">"
    pixdim = struct.unpack_from(endian + "8f", raw, 76)
    qform_code, sform_code = struct.unpack_from(endian + "hh", raw, 252)
    affine = np.eye(4)
    if sform_code > 0:
        for r in range(3):
            affine[r] = struct.unpack_from(endian + "4f", raw, 280 + 16 * r)
        return affine, "sform"
    if qform_code > 0:
        b, c, d = (float(v) for v in struct.unpack_from(endian + "3f", raw, 256))
        scale = np.array(pixdim[1:4], dtype=np.float64)
        scale[2] *= -1.0 if pixdim[0] < 0 else 1.0
        affine[:3, :3] = _quaternion_rotation(b, c, d) * scale
        affine[:3, 3] = struct.unpack_from(endian + "3f", raw, 268)
        return affine, "qform"
    affine[:3, :3] = np.diag(np.array(pixdim[1:4], dtype=np.float64))
    return affine, "pixdim"


RAW_DTYPES = (np.dtype(np.int16), np.dtype(np.float32))


def _header(raw):
    endian = "<" if struct.unpack_from("<i", raw, 0)[0] == 348 else ">"
    dim = struct.unpack_from(endian + "8h", raw, 40)
    code, _bits = struct.unpack_from(endian + "hh", raw, 70)
    vox_offset = int(struct.unpack_from(endian + "f", raw, 108)[0])
    slope, inter = struct.unpack_from(endian + "ff", raw, 112)
    return endian, tuple(dim[1:1 + dim[0]]), code, vox_offset, slope, inter


def read_nifti_raw(fp):
    """The volume as the file stores it, without conversion: a read-only x-fastest (Fortran order)
    view of the decoded bytes, when the file holds little-endian int16 or float32 and no scaling
    applies (read_nifti's rule).  Any other file comes back as read_nifti(fp, np.float32).  Either
    way np.float32 of the result equals read_nifti(fp, np.float32)."""
    with _open(fp, "rb") as f:
        raw = f.read()
    endian, shape, code, vox_offset, slope, inter = _header(raw)
    scaled = (slope not in (0.0, 1.0) or inter != 0.0) and slope != 0.0 and not np.isnan(slope)
    dt = np.dtype(_CODES.get(code, np.uint8))
    if endian != "<" or scaled or code not in _CODES or dt not in RAW_DTYPES:
        return read_nifti(fp, np.float32)
    data = np.frombuffer(raw, dtype=dt, count=int(np.prod(shape)), offset=max(vox_offset, 352))
    return data.reshape(shape, order="F")



def _files_with_suffix(folder, suffix, recursive):
    """Sorted paths under folder whose name ends with suffix."""
    if recursive:
        found = [os.path.join(root, f) for root, _, files in os.walk(folder) for f in files]
    else:
        found = [os.path.join(folder, f) for f in os.listdir(folder)]
    return sorted(p for p in found if p.endswith(suffix))


def read_in_patient_sample(scan_dir, modality_exts):
    """One scan's modalities as float32, channel last in the order of modality_exts (a single
    modality is returned without a channel axis).  Counterpart of reference nifti_io.py:12-29:
    files are searched below scan_dir, and every suffix must match exactly one of them."""
    channels = []
    for ext in modality_exts:
        paths = _files_with_suffix(scan_dir, ext, recursive=True)
        if len(paths) != 1:
            raise FileNotFoundError(f"{scan_dir}: {len(paths)} files end with {ext!r}, expected exactly one")
        channels.append(read_nifti(paths[0], np.float32))
    return channels[0] if len(channels) == 1 else np.stack(channels, axis=3)


def find_modality_files(scan_dir, modality_exts):
    """Path of each modality of a scan, in the order of modality_exts: read_in_patient_sample's rule
    (searched below scan_dir, every suffix must match exactly one file)."""
    paths = []
    for ext in modality_exts:
        found = _files_with_suffix(scan_dir, ext, recursive=True)
        if len(found) != 1:
            raise FileNotFoundError(f"{scan_dir}: {len(found)} files end with {ext!r}, expected exactly one")
        paths.append(found[0])
    return paths


def read_in_patient_sample_raw(scan_dir, modality_exts):
    """One scan's modalities as read_nifti_raw returns them (stored dtype, x-fastest), one array per
    modality in the order of modality_exts."""
    return [read_nifti_raw(p) for p in find_modality_files(scan_dir, modality_exts)]


def read_in_labels(scan_dir, label_ext):
    """One scan's int16 label volume (reference nifti_io.py:32-39): the first file directly in
    scan_dir whose name ends with label_ext."""
    paths = _files_with_suffix(scan_dir, label_ext, recursive=False)
    if not paths:
        raise FileNotFoundError(f"{scan_dir}: no label file ending with {label_ext!r}")
    return read_nifti(paths[0], np.int16)
