"""Host side of the conform stage (gts/conform.py, data_processing/nifti_io.read_affine): header geometry, the
plan and its index tables, and the argument checks of gts_conform_gather.  No GPU."""
import ctypes
import gzip
import struct

import numpy as np
import pytest

from tests import conform_ref as R

AFFINES = {
    "brats": None,      # filled from nifti_io below
    "ras_origin": np.array([[1.0, 0, 0, -90.5], [0, 1.0, 0, -126.25], [0, 0, 1.0, -72.0], [0, 0, 0, 1.0]]),
    # input axes run along world z (up), x (towards left), y (towards anterior) at 5 x 0.9375 x 0.75 mm
    "permuted_anisotropic": R.make_affine((2, 0, 1), (1, -1, 1), (5.0, 0.9375, 0.75), (12.5, -3.0, 40.0)),
}


def _affine(name):
    from data_processing import nifti_io

    return nifti_io.BRATS_AFFINE if name == "brats" else AFFINES[name]


def _patch_header(src, dst, edit):
    with gzip.open(src, "rb") as f:
        raw = bytearray(f.read())
    edit(raw)
    with gzip.open(dst, "wb") as f:
        f.write(bytes(raw))


@pytest.mark.parametrize("name", sorted(AFFINES))
def test_read_affine_returns_what_was_written(tmp_path, name):
    from data_processing import nifti_io

    A = _affine(name)
    fp = str(tmp_path / "v.nii.gz")
    nifti_io.save_as_nifti(np.zeros((3, 4, 5), dtype=np.int16), fp, affine=A)
    got, source = nifti_io.read_affine(fp)
    assert source == "sform" and got.dtype == np.float64 and got.shape == (4, 4)
    assert np.array_equal(got, np.asarray(A, dtype=np.float32).astype(np.float64))   # the header stores float32
    with gzip.open(fp, "rb") as f:
        pixdim = struct.unpack_from("<8f", f.read(348), 76)
    assert np.allclose(pixdim[1:4], np.sqrt((np.asarray(A)[:3, :3] ** 2).sum(axis=0)), rtol=1e-7)


@pytest.mark.parametrize("name", sorted(AFFINES))
def test_quaternion_path_gives_the_same_affine(tmp_path, name):
    """sform_code 0, qform_code 1: method 2 of the specification.  The BraTS affine is a proper rotation, the
    RAS one too; the permuted one is improper (qfac = -1)."""
    from data_processing import nifti_io

    A = np.asarray(_affine(name), dtype=np.float64)
    fp, fq = str(tmp_path / "s.nii.gz"), str(tmp_path / "q.nii.gz")
    nifti_io.save_as_nifti(np.zeros((3, 4, 5), dtype=np.int16), fp, affine=A)
    _patch_header(fp, fq, lambda raw: struct.pack_into("<hh", raw, 252, 1, 0))
    got, source = nifti_io.read_affine(fq)
    assert source == "qform"
    assert np.abs(got - A).max() <= 1e-6 * max(1.0, np.abs(A).max())
    if name == "permuted_anisotropic":
        assert np.linalg.det(A[:3, :3]) < 0          # the case that needs qfac = -1


def test_qfac_zero_counts_as_plus_one(tmp_path):
    from data_processing import nifti_io

    A = AFFINES["ras_origin"]
    fp, fq = str(tmp_path / "s.nii.gz"), str(tmp_path / "q.nii.gz")
    nifti_io.save_as_nifti(np.zeros((2, 2, 2), dtype=np.int16), fp, affine=A)

    def edit(raw):
        struct.pack_into("<hh", raw, 252, 1, 0)
        struct.pack_into("<f", raw, 76, 0.0)
    _patch_header(fp, fq, edit)
    assert np.abs(nifti_io.read_affine(fq)[0] - A).max() <= 1e-6 * 126.25


def test_no_codes_gives_pixdim_diagonal(tmp_path):
    from data_processing import nifti_io

    fp, fq = str(tmp_path / "s.nii.gz"), str(tmp_path / "q.nii.gz")
    nifti_io.save_as_nifti(np.zeros((2, 2, 2), dtype=np.int16), fp, affine=AFFINES["permuted_anisotropic"])
    _patch_header(fp, fq, lambda raw: struct.pack_into("<hh", raw, 252, 0, 0))
    got, source = nifti_io.read_affine(fq)
    assert source == "pixdim"
    assert np.array_equal(got, np.diag([5.0, 0.9375, 0.75, 1.0]))


def test_big_endian_header_is_read(tmp_path):
    from data_processing import nifti_io

    A = AFFINES["permuted_anisotropic"]
    hdr = bytearray(352)
    struct.pack_into(">i", hdr, 0, 348)
    struct.pack_into(">8h", hdr, 40, 3, 2, 2, 2, 1, 1, 1, 1)
    struct.pack_into(">hh", hdr, 70, 4, 16)
    struct.pack_into(">8f", hdr, 76, -1.0, 5.0, 0.9375, 0.75, 1.0, 1.0, 1.0, 1.0)
    struct.pack_into(">f", hdr, 108, 352.0)
    struct.pack_into(">hh", hdr, 252, 0, 2)
    for r in range(3):
        struct.pack_into(">4f", hdr, 280 + 16 * r, *[float(x) for x in A[r]])
    hdr[344:348] = b"n+1\0"
    fp = str(tmp_path / "be.nii")
    with open(fp, "wb") as f:
        f.write(bytes(hdr) + np.arange(8, dtype=">i2").tobytes())
    got, source = nifti_io.read_affine(fp)
    assert source == "sform" and np.array_equal(got, A)


def _rotation(axis, degrees):
    th = np.radians(degrees)
    c, s = np.cos(th), np.sin(th)
    m = np.eye(4)
    i, j = [k for k in range(3) if k != axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


@pytest.mark.parametrize("oblique", [False, True])
def test_plan_recovers_all_48_orientations(oblique):
    from gts import conform

    s = (0.8, 1.0, 2.5)
    shape = (7, 5, 6)
    for perm, signs in R.ORIENTATIONS:
        A = R.make_affine(perm, signs, s, (3.0, -2.0, 7.0))
        if oblique:
            A = _rotation(1, 3.0) @ A
        pl = conform.plan(A, shape)
        assert pl.perm == tuple(perm) and pl.flips == R.flips_of(perm, signs), (perm, signs)
        assert np.allclose(pl.spacing, s, rtol=1e-12) and pl.spacing[1] == 1.0
        assert pl.shape == shape and pl.out_shape == R.conformed_shape(shape, perm, pl.spacing)
        assert pl.source == R.source_of(perm)
        if oblique:
            assert abs(pl.obliquity_deg - 3.0) < 0.01
        else:
            assert pl.obliquity_deg == 0.0
        assert not pl.is_identity


def test_plan_axis_codes_and_description():
    from data_processing import nifti_io
    from gts import conform

    assert conform.plan(nifti_io.BRATS_AFFINE, (240, 240, 155)).axis_codes == "LPS"
    ras = conform.plan(AFFINES["ras_origin"], (4, 4, 4))
    assert ras.axis_codes == "RAS" and ras.flips == (True, True, False) and not ras.resamples
    assert ras.describe() == "conform: RAS -> LPS, spacing (1, 1, 1) mm, obliquity 0.0°"
    assert conform.plan(AFFINES["permuted_anisotropic"], (4, 4, 4)).axis_codes == "SLA"


def test_plan_ties_go_to_the_smallest_permutation():
    from gts import conform

    A = _rotation(2, 45.0)                 # x and y columns score the same on world x and world y
    assert conform.plan(A, (3, 3, 3)).perm == (0, 1, 2)


@pytest.mark.parametrize("bad", [0.0, np.nan, np.inf])
def test_plan_refuses_a_degenerate_spacing(bad):
    from gts import conform

    A = np.diag([1.0, bad, 1.0, 1.0])
    with pytest.raises(ValueError, match="spacing"):
        conform.plan(A, (4, 4, 4))


def test_near_unit_spacing_snaps_and_brats_is_identity():
    from data_processing import nifti_io
    from gts import conform

    A = np.array(nifti_io.BRATS_AFFINE, dtype=np.float64)
    assert conform.plan(A, (240, 240, 155)).is_identity
    A[:3, :3] *= 1.00005
    pl = conform.plan(A, (240, 240, 155))
    assert pl.spacing == (1.0, 1.0, 1.0) and pl.is_identity and pl.out_shape == (240, 240, 155)
    A[:3, :3] *= 1.001
    pl = conform.plan(A, (240, 240, 155))
    assert pl.spacing[0] != 1.0 and not pl.is_identity
    assert pl.describe().startswith("conform: LPS -> LPS, spacing (1.00105")
    assert conform.plan(nifti_io.BRATS_AFFINE, (5, 6, 7)).describe() == "conform: identity"


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("s", [0.5, 1, 1.2, 2, 3])
@pytest.mark.parametrize("reverse", [False, True])
def test_tables(n, s, reverse):
    from gts import conform

    tb = conform.forward_tables(n, s, reverse)
    n_out = int(np.floor((n - 1) * s)) + 1
    assert tb.n_out == n_out == len(tb.idx1) == len(tb.t)
    assert tb.idx0.dtype == np.int32 and tb.idx1.dtype == np.int32 and tb.t.dtype == np.float64
    assert np.all((tb.t >= 0) & (tb.t < 1))
    i0, i1, t = R.axis_samples(n, s, reverse)
    assert np.array_equal(tb.idx0, i0) and np.array_equal(tb.idx1, i1) and np.array_equal(tb.t, t)
    r0 = n - 1 - tb.idx0 if reverse else tb.idx0
    r1 = n - 1 - tb.idx1 if reverse else tb.idx1
    assert r0.min() >= 0 and r1.max() <= n - 1 and np.all((r1 == r0 + 1) | (r1 == n - 1))
    assert r0[0] == 0 and tb.t[0] == 0
    assert (n_out - 1) / s <= n - 1                  # the last sample lies inside the input
    if s == 1:
        assert np.array_equal(r0, np.arange(n)) and not tb.t.any()
    inv = conform.inverse_tables(n, s, reverse, n_out)
    assert inv.n_out == n and not inv.t.any() and np.array_equal(inv.idx0, inv.idx1)
    assert inv.idx0.min() >= 0 and inv.idx0.max() <= n_out - 1
    r = np.arange(n)[::-1] if reverse else np.arange(n)
    assert np.array_equal(inv.idx0, np.minimum(np.floor(r * np.float64(s) + 0.5), n_out - 1))


def test_modalities_must_agree():
    from gts import conform

    A = AFFINES["ras_origin"]
    near = A.copy()
    near[0, 3] += 9e-4
    pl = conform.plan_for_modalities([A, near, A, A], [(4, 5, 6)] * 4)
    assert pl.axis_codes == "RAS" and pl.shape == (4, 5, 6)
    far = A.copy()
    far[1, 1] += 2e-3
    with pytest.raises(ValueError, match="disagree"):
        conform.plan_for_modalities([A, A, far, A], [(4, 5, 6)] * 4)
    with pytest.raises(ValueError, match="one shape"):
        conform.plan_for_modalities([A] * 4, [(4, 5, 6), (4, 5, 6), (4, 5, 7), (4, 5, 6)])


def test_uncrop_to_shape():
    from data_processing.image_processing import uncrop_to_shape

    crop = np.ix_(np.array([False, True, True, False, True]), np.array([True, False, True]), np.array([False, True]))
    pred = np.arange(6, dtype=np.int16).reshape(3, 2, 1) + 1
    full = uncrop_to_shape(crop, pred, (5, 3, 2))
    assert full.dtype == np.int16 and full.shape == (5, 3, 2) and int((full != 0).sum()) == 6
    assert np.array_equal(full[crop], pred)


def test_cpu_tensors_are_refused(hip_lib):
    import torch

    import gts
    from gts import conform

    pl = conform.plan(AFFINES["ras_origin"], (4, 5, 6))
    with pytest.raises(gts.GtsError, match="MI355X only"):
        conform.conform_scan(torch.zeros((4, 6, 5, 4), dtype=torch.int16), pl)
    with pytest.raises(gts.GtsError, match="MI355X only"):
        conform.conform_labels(torch.zeros((6, 5, 4), dtype=torch.int16), pl)
    with pytest.raises(gts.GtsError, match="MI355X only"):
        conform.unconform_labels(torch.zeros((6, 5, 4), dtype=torch.int16), pl)
    ident = conform.plan(np.diag([-1.0, -1.0, 1.0, 1.0]), (4, 5, 6))
    with pytest.raises(gts.GtsError, match="MI355X only"):
        conform.conform_scan(torch.zeros((4, 6, 5, 4), dtype=torch.int16), ident)


def test_argument_errors_do_not_need_a_gpu(hip_lib):
    one = ctypes.c_void_p(16)

    def call(src=one, dtype=4, C=4, dims=(5, 6, 7), axes=(0, 1, 2), out=(5, 6, 7), idx0=one, idx1=one, t=one, mode=0,
             dst=one):
        return hip_lib.gts_conform_gather(src, dtype, C, *dims, *axes, *out, idx0, idx1, t, mode, dst, None)

    assert call(src=None) == -1 and call(dst=None) == -1 and call(idx0=None) == -1
    assert call(mode=1, idx1=None) == -1 and call(mode=2, t=None) == -1
    assert call(dims=(0, 6, 7)) == -2 and call(dims=(5, -1, 7)) == -2 and call(out=(5, 6, 0)) == -2
    assert call(C=-1) == -2 and call(dims=(70000, 6, 7)) == -2
    assert call(dims=(2048, 2048, 512)) == -2                       # 2^31 voxels
    assert call(axes=(0, 1, 1)) == -3 and call(axes=(0, 1, 3)) == -3 and call(axes=(-1, 1, 2)) == -3
    assert call(dtype=8) == -3 and call(mode=3) == -3 and call(mode=-1) == -3
    assert call(dtype=16, mode=2) == -3                             # nearest is for int16 labels
    assert call(C=0) == 0                                           # zero-sized: accepted, nothing launched
    assert b"NULL" in hip_lib.gts_error_string(call(src=None))
