"""Host half of the co-registration (gts/register.py, gts/conform.conformed_affine): the frame
arithmetic, the mutual information, the reference search of tests/register_ref.py on a phantom with a known motion,
and the CLI flags.  No GPU."""
import functools

import numpy as np
import pytest

from tests import conform_ref as C
from tests import register_ref as R

SPACINGS = [(1, 1, 2), (0.5, 0.5, 1), (1.2, 0.8, 3.0), (0.9375, 0.9375, 5)]     # test_gpu_conform.py's
PHANTOM_SHAPE = (40, 36, 32)
TRUE_MOTION = (1.5, -2.0, 1.0, 3.0, -2.0, 4.0)
# mean displacement over brain voxels (voxels = mm here) after the search, measured with tests/register_ref.py and
# recorded in DESIGN.md 4v (2.77 - 2.78 before, maxima 0.37 / 0.53 / 0.51 after); the test's bound is twice the mean
MEASURED_MEAN = {5: 0.2171, 7: 0.2912, 11: 0.2737}


def test_conformed_affine_agrees_with_the_plan_tables():
    from gts import conform

    shape = (7, 5, 6)
    worst = 0.0
    for perm, signs in C.ORIENTATIONS:
        for spacing in SPACINGS:
            affine = C.make_affine(perm, signs, spacing, (4.0, -7.5, 11.0))
            pl = conform.plan(affine, shape)
            W = conform.conformed_affine(pl, affine)
            # where the tables put conformed index i of axis w along the input axis it reads
            pos = [tb.idx0 + tb.t * (tb.idx1.astype(np.float64) - tb.idx0) for tb in pl.forward]
            for idx in np.ndindex(*pl.out_shape):
                at = np.zeros(4)
                at[3] = 1.0
                for w in range(3):
                    at[pl.source[w]] = pos[w][idx[w]]
                gap = np.abs(W @ np.array(idx + (1.0,)) - affine @ at).max()
                worst = max(worst, float(gap))
    assert worst <= 1e-9, worst


def test_header_transform_on_identical_grids_is_the_plans_map():
    from gts import conform, register

    shape = (9, 8, 5)
    for perm, signs in C.ORIENTATIONS[::5]:
        affine = C.make_affine(perm, signs, (1.2, 0.8, 3.0), (4.0, -7.5, 11.0))
        pl = conform.plan(affine, shape)
        T = register.header_transform(pl, affine, affine)
        assert T.shape == (3, 4) and T.dtype == np.float64 and T.flags["C_CONTIGUOUS"]
        pos = [tb.idx0 + tb.t * (tb.idx1.astype(np.float64) - tb.idx0) for tb in pl.forward]
        for idx in [(0, 0, 0), tuple(n - 1 for n in pl.out_shape), (1, 2, 1)]:
            want = np.zeros(3)
            for w in range(3):
                want[pl.source[w]] = pos[w][idx[w]]
            assert np.abs(T @ np.array(idx + (1.0,)) - want).max() <= 1e-9
        zero = register.header_transform(pl, affine, affine, np.zeros(6))
        assert np.abs(zero - T).max() <= 1e-12


def test_header_transform_undoes_a_rigid_offset_in_the_affine():
    """Modality k's header says its grid is the reference grid moved by a known rigid motion M: A_k = M . A_ref.  The
    point of the reference frame at world p then has the index inv(A_k) p, and header_transform must find it."""
    from data_processing import nifti_io
    from gts import conform, register

    a_ref = np.array(nifti_io.BRATS_AFFINE, dtype=np.float64)
    shape = (20, 18, 16)
    pl = conform.plan(a_ref, shape)
    assert pl.is_identity
    M = register.rigid((3.0, -1.5, 2.0, 5.0, -3.0, 8.0), (10.0, 20.0, 5.0))
    assert np.allclose(M[:3, :3] @ M[:3, :3].T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(M[:3, :3]), 1.0)
    a_k = M @ a_ref
    T = register.header_transform(pl, a_ref, a_k)
    for idx in [(0.0, 0.0, 0.0), (19.0, 17.0, 15.0), (3.0, 9.0, 4.0)]:
        world = a_ref @ np.array(idx + (1.0,))
        index_k = T @ np.array(idx + (1.0,))
        assert np.abs(a_k @ np.append(index_k, 1.0) - world).max() <= 1e-9
    # and the search's own parameters: R(params) with the inverse motion about the same centre puts it back
    centre = (conform.conformed_affine(pl, a_ref) @ np.array([9.5, 8.5, 7.5, 1.0]))[:3]
    params = (1.0, 2.0, -3.0, 4.0, 5.0, -6.0)
    a_moved = register.rigid(params, centre) @ a_ref
    back = register.header_transform(pl, a_ref, a_moved, params)
    assert np.abs(back - np.eye(4)[:3]).max() <= 1e-9


def test_rotation_order_and_units():
    from gts import register

    assert np.allclose(register.rotation(0, 0, 90) @ [1, 0, 0], [0, 1, 0], atol=1e-15)
    assert np.allclose(register.rotation(90, 0, 0) @ [0, 1, 0], [0, 0, 1], atol=1e-15)
    assert np.allclose(register.rotation(0, 90, 0) @ [0, 0, 1], [1, 0, 0], atol=1e-15)
    # Rz . Ry . Rx: x is applied first
    assert np.allclose(register.rotation(90, 0, 90) @ [0, 1, 0], [0, 0, 1], atol=1e-15)
    assert np.array_equal(register.rotation(0, 0, 0), np.eye(3))


def _counts(table, outside=0):
    return np.concatenate([np.asarray(table, dtype=np.int64).ravel(), [outside]])


@pytest.mark.parametrize("bins", [16, 32, 64])
def test_mutual_information_on_hand_made_tables(bins):
    from gts import register

    independent = np.outer(np.arange(1, bins + 1), np.arange(2, bins + 2))          # p = px py in every cell
    assert abs(register.mutual_information(_counts(independent, 7))) <= 1e-12
    diagonal = np.eye(bins, dtype=np.int64) * 5
    assert abs(register.mutual_information(_counts(diagonal)) - np.log(bins)) <= 1e-12
    empty = register.mutual_information(_counts(np.zeros((bins, bins)), 99))
    assert isinstance(empty, float) and empty == 0.0
    rng = np.random.default_rng(bins)
    tables = rng.integers(0, 50, (3, bins, bins)) * (rng.random((3, bins, bins)) < 0.3)
    rows = np.stack([_counts(t, 3) for t in tables])
    got = register.mutual_information(rows)
    assert got.shape == (3,) and got.dtype == np.float64
    for g, row in zip(got, rows):
        assert g == R.mutual_information(row)           # the same sum in the same order: the same bits
        assert g >= 0.0


def phantom(seed):
    """(fixed, moving, base_transform, brain mask, the moving volume's true map): modality 2 of a synthetic scan, and
    modality 0 carried by TRUE_MOTION, both on a 1 mm LPS grid."""
    from data_processing import nifti_io
    from gts import conform, register, synth_mri

    img, _ = synth_mri.make_sample(seed, PHANTOM_SHAPE)
    affine = np.array(nifti_io.BRATS_AFFINE, dtype=np.float64)
    pl = conform.plan(affine, PHANTOM_SHAPE)
    family = functools.partial(register.header_transform, pl, affine, affine)
    carried = family(np.array(TRUE_MOTION))
    fixed = np.ascontiguousarray(img[..., 2])
    moving = R.affine_resample(img[..., 0], carried, PHANTOM_SHAPE)
    return fixed, moving, family, fixed > 0, carried


def displacement(found, carried, mask):
    """Mean and maximum over the masked voxels of |S(T x) - x| in voxels: S carried the moving volume, T was found."""
    S, T = np.vstack([carried, [0, 0, 0, 1.0]]), np.vstack([found, [0, 0, 0, 1.0]])
    x = np.stack(np.nonzero(mask) + (np.ones(int(mask.sum())),)).astype(np.float64)
    d = np.sqrt((((S @ T) @ x - x)[:3] ** 2).sum(axis=0))
    return float(d.mean()), float(d.max())


@pytest.mark.parametrize("seed", sorted(MEASURED_MEAN))
def test_reference_search_recovers_a_known_motion(seed):
    fixed, moving, family, brain, carried = phantom(seed)
    before, _ = displacement(np.eye(4)[:3], carried, brain)
    params, score, launches, outside = R.search(fixed, moving, family, (2, 1), 32)
    mean, worst = displacement(family(params), carried, brain)
    print(f"seed {seed}: before {before:.4f}, mean {mean:.4f}, max {worst:.4f} voxel, {launches} launches, "
          f"MI {score:.6f}, outside {outside:.4f}, params {np.round(params, 4).tolist()}")
    assert before > 2.0
    assert mean <= 2.0 * MEASURED_MEAN[seed]
    assert np.all(np.abs(params[3:]) < 15.0) and 0.0 <= outside < 0.5 and score > 0.0


def test_coregister_flags():
    from scripts import segment_scans

    base = ["-d", "in", "-o", "out", "-g", "gnn.pt"]
    plain = segment_scans.parse_args(base)
    assert plain.conform is False and plain.coregister is None and plain.coregister_ref is None
    conform_only = segment_scans.parse_args(base + ["--conform"])
    assert conform_only.conform is True and conform_only.coregister_ref is None
    on = segment_scans.parse_args(base + ["--coregister"])
    assert on.conform is True and on.coregister_ref == 0 and on.coregister_header_only is False
    assert on.coregister_levels == [4, 2] and on.coregister_bins == 32 and on.coregister_max_rotate == 15.0
    named = segment_scans.parse_args(base + ["--coregister", "_t1ce.nii.gz", "--coregister_levels", "2", "1",
                                             "--coregister_bins", "64", "--coregister_header_only",
                                             "--coregister_report", "r.json", "--coregister_max_rotate", "5"])
    assert named.conform is True and named.coregister_ref == 2 and named.coregister_levels == [2, 1]
    assert named.coregister_bins == 64 and named.coregister_header_only and named.coregister_report == "r.json"
    assert named.coregister_max_rotate == 5.0
    for bad in (["--coregister", "_nope.nii.gz"], ["--coregister_header_only"], ["--coregister_report", "r.json"],
                ["--coregister", "--coregister_levels", "0"]):
        with pytest.raises(ValueError):
            segment_scans.parse_args(base + bad)
    assert segment_scans.main(base + ["--coregister", "_nope.nii.gz"]) == 2


def test_flags_at_their_defaults_leave_load_as_it_was(tmp_path, monkeypatch):
    """Without --coregister, Segmenter.load takes the paths it took: stage_scan alone, or the shared plan with the
    ValueError for grids that differ."""
    from data_processing import nifti_io
    from scripts import segment_scans

    base = ["-d", str(tmp_path), "-o", str(tmp_path / "out"), "-g", "gnn.pt"]
    vol = np.arange(4 * 3 * 2, dtype=np.int16).reshape(4, 3, 2)
    other = np.array(nifti_io.BRATS_AFFINE, dtype=np.float64)
    other[0, 3] = 2.0
    for ext, affine in zip(("_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"),
                           (nifti_io.BRATS_AFFINE,) * 3 + (other,)):
        nifti_io.save_as_nifti(np.asfortranarray(vol), str(tmp_path / ("S" + ext)), affine=affine)

    def segmenter(flags):
        seg = segment_scans.Segmenter.__new__(segment_scans.Segmenter)      # the host stage needs no nets and no GPU
        seg.args = segment_scans.parse_args(base + flags)
        seg.conform = bool(seg.args.conform)
        seg.coregister_ref = seg.args.coregister_ref
        return seg

    staged = segmenter([]).load(str(tmp_path))
    assert tuple(staged.shape) == (4, 2, 3, 4)
    with pytest.raises(ValueError, match="disagree by 2"):
        segmenter(["--conform"]).load(str(tmp_path))
    volumes, plan, affines = segmenter(["--coregister", "_t2.nii.gz"]).load(str(tmp_path))
    assert plan is None and len(volumes) == 4 and all(tuple(v.shape) == (2, 3, 4) for v in volumes)
    assert np.array_equal(affines[3], other) and np.array_equal(volumes[0].numpy(), vol.T)
