"""The texture kernels on the MI355X (gts/texture.py, csrc/gts_texture.hip) against
tests/texture_ref.py: root, n, lo, hi, levels, hist and glcm equal the numpy definition exactly, for int16 and
float32 scans and at grid_blocks 0, 1 and 7; the float64 features, being derived from equal tables, are equal too
(tests/test_texture_host.py holds `derive` to the exact reference and checks what the reference costs)."""
import json

import numpy as np
import pytest
import torch

from tests import measure_ref
from tests import texture_ref as ref

pytestmark = pytest.mark.gpu

GRIDS = (0, 1, 7)
KEYS = ("root", "n", "lo", "hi", "levels", "hist", "glcm")


def _dev(vol):
    return torch.from_numpy(np.ascontiguousarray(vol)).cuda()


def _assert_equal(got, want, note):
    for key in KEYS:
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (note, key, got[key].shape)
        assert np.array_equal(got[key], want[key]), (note, key, got[key].ravel()[:8], want[key].ravel()[:8])
    assert (got["hist"].sum(axis=1) == got["n"]).all(), note


def _check(labels, image, region="WT", connectivity=26, grids=GRIDS, want=None, both_dtypes=True, **binning):
    """lesion_texture at every grid against the reference, for the image as it is and (int16 images) as float32."""
    from gts import texture

    images = [image] + ([image.astype(np.float32)] if both_dtypes and image.dtype == np.int16 else [])
    for img in images:
        expect = want if want is not None and img is image else \
            ref.lesion_texture(labels, img, region, connectivity, binning.get("bins", 32), binning.get("bin_width"),
                               binning.get("min_lesion_voxels", 1))
        for grid in grids:
            got = texture.lesion_texture(_dev(labels), _dev(img), region, connectivity, grid_blocks=grid, **binning)
            _assert_equal(got, expect, (img.dtype, region, connectivity, grid, binning))
    return expect


# 1. closed forms
@pytest.mark.parametrize("name", sorted(ref.box_cases()))
def test_constant_box_closed_form(hip_lib, name):
    labels, image = ref.box_cases()[name]
    want = _check(labels, image)
    extent = (3, 3, 1) if name == "unit-axis" else ref.BOX
    assert want["levels"].tolist() == [1] and want["hist"].tolist() == [[int(np.prod(extent))]]
    assert want["glcm"][0, :, 0, 0].tolist() == [2 * np.prod([e - abs(s) for e, s in zip(extent, delta)])
                                                 for delta in ref.DIRECTIONS]


# 2. ramp and checkerboard
def test_ramp_and_checkerboard(hip_lib):
    labels, image, (a, b, c) = ref.ramp_case()
    want = _check(labels, image, bins=a)
    for d, (dx, dy, dz) in enumerate(ref.DIRECTIONS):
        per_step = (b - abs(dy)) * (c - abs(dz))
        off = np.eye(a, k=1, dtype=np.int64) + np.eye(a, k=-1, dtype=np.int64)
        assert np.array_equal(want["glcm"][0, d], per_step * off if dx else 2 * per_step * np.eye(a, dtype=np.int64))
    labels, image, _ = ref.checkerboard_case()
    want = _check(labels, image, region="CT", bins=2)
    for d, delta in enumerate(ref.DIRECTIONS):
        if sum(abs(s) for s in delta) == 1:                  # the face directions: purely off-diagonal
            assert want["glcm"][0, d, 0, 0] == 0 == want["glcm"][0, d, 1, 1] and want["glcm"][0, d, 0, 1] > 0


# 3. the same root, not the same mask
def test_lesions_that_touch_do_not_pair(hip_lib):
    labels, image = ref.touching_case()
    six = _check(labels, image, connectivity=6)
    whole = _check(labels, image, connectivity=26)
    assert len(six["root"]) == 3 and len(whole["root"]) == 1
    assert six["glcm"].sum() == 3 * ref.lesion_texture(labels[:2, :2, :3], image[:2, :2, :3], "WT", 6)["glcm"].sum()
    assert whole["glcm"].sum() > six["glcm"].sum()


# 4. chunk edges
@pytest.mark.parametrize("voxels", [2047, 2048, 2049, 4097])
def test_chunk_edges(hip_lib, voxels):
    from gts import texture

    chunk = texture.CHUNK
    assert voxels in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)
    labels, image = ref.chunk_case(voxels, chunk)
    want = _check(labels, image, both_dtypes=False)
    assert want["n"].tolist() == [voxels] and len(texture.work_units(want["n"])) == 13 * -(-voxels // chunk)
    assert (want["hist"] > 0).sum() == 32


# 5. level edges
@pytest.mark.parametrize("bins", [1, 2, 32, 128])
def test_bin_numbers(hip_lib, bins):
    name, labels, image = ref.cached_selection()[21]         # 1 x 40 x 33 at 0.31, float32
    assert image.dtype == np.float32
    want = _check(labels, image, bins=bins, min_lesion_voxels=2)
    top = want["levels"] == bins
    assert top.any() and (want["hist"][top, bins - 1] >= 1).all()       # the voxel equal to hi lands in N - 1
    labels, image, _ = ref.ramp_case()
    flat = _check(labels, np.full(image.shape, -7, dtype=np.int16), bins=bins)           # hi == lo
    assert flat["levels"].tolist() == [1] and flat["hist"].shape == (1, 1)


def test_bin_widths(hip_lib):
    from gts import GtsError, texture

    line = np.full((1, 1, 130), 1, dtype=np.int16)
    ramp = np.arange(130, dtype=np.int16).reshape(1, 1, 130) - 40
    line[0, 0, 128:] = 0
    want = _check(line, ramp, bin_width=1.0)                 # exactly 128 levels
    assert want["levels"].tolist() == [128] and want["hist"].tolist() == [[1] * 128]
    line[0, 0, 128] = 1
    for image in (ramp, ramp.astype(np.float32)):
        with pytest.raises(GtsError, match="root 1 spans 129 levels.*widen the bins"):
            texture.lesion_texture(_dev(line), _dev(image), "WT", bin_width=1.0)
    _check(line, ramp, bin_width=1.5)
    block = np.full((2, 3, 4), 2, dtype=np.int16)            # negative and fractional values, some on bin boundaries
    values = np.float32([-2.5, -2.0, -1.99, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.49, 1.5, 1.51, 2.0, 2.5, 3.0,
                         -1.0, -1.5, -0.75, 0.1, 0.2, 0.3, -0.1, -0.2]).reshape(2, 3, 4)
    want = _check(block, values, bin_width=0.5)
    assert want["levels"].tolist() == [12] and want["hist"][0, 0] == 1 and want["hist"][0, 4] == 4   # floor, not trunc
    _check(block, values, bin_width=0.25)
    _check(block, values, bins=11)                           # (v - lo) * 11 / 5.5: every half lies on a boundary


# 6. selection
@pytest.mark.parametrize("index", range(len(ref.selection_cases())), ids=[c[0] for c in ref.selection_cases()])
def test_selection_on_random_volumes(hip_lib, index):
    name, labels, image = ref.cached_selection()[index]
    for connectivity in (6, 26):
        for least in (1, 5):
            want = ref.cached_selection_table(index, connectivity, least)
            got = _check(labels, image, connectivity=connectivity, want=want, both_dtypes=False,
                         min_lesion_voxels=least)
            assert (got["n"] >= least).all()
    _check(labels, image, region="ET", grids=(0,), both_dtypes=False, min_lesion_voxels=2)


# 7. contention
@pytest.mark.parametrize("name", sorted(ref.contention_cases()))
def test_contention(hip_lib, name):
    labels, image, bins = ref.contention_cases()[name]
    want = _check(labels, image, bins=bins, both_dtypes=False)
    assert want["n"].tolist() == [4096]
    if name == "constant":                                   # every add of a direction goes to one counter
        assert want["glcm"][0, :, 0, 0].tolist() == [2 * np.prod([16 - abs(s) for s in d]) for d in ref.DIRECTIONS]
    else:
        assert want["levels"].tolist() == [128] and (want["glcm"][0] > 0).sum() > 13 * 3000


# 8. non-finite values
def test_non_finite_values(hip_lib):
    from gts import GtsError, texture

    labels = np.zeros((6, 7, 8), dtype=np.int16)
    labels[1:4, 1:4, 1:4] = 1                                # root 66, 27 voxels
    labels[5, 6, 6:8] = 2                                    # root 335, 2 voxels
    image = ref.random_image(labels.shape, np.float32, 5)
    for bad in (np.nan, np.inf, -np.inf):
        inside = image.copy()
        inside[2, 2, 2] = bad
        for least in (1, 5):
            with pytest.raises(GtsError, match="1 NaN or Inf voxel.*root 66"):
                texture.lesion_texture(_dev(labels), _dev(inside), "WT", min_lesion_voxels=least)
        outside = image.copy()
        outside[5, 6, 7] = outside[0, 0, 0] = outside[4, 4, 4] = bad      # an unselected lesion and the background
        want = _check(labels, outside, min_lesion_voxels=5)
        assert want["root"].tolist() == [66]
        with pytest.raises(GtsError, match="root 335"):
            texture.lesion_texture(_dev(labels), _dev(outside), "WT")


def test_empty_regions_and_wrapper_checks(hip_lib):
    from gts import GtsError, texture

    labels = np.zeros((4, 5, 6), dtype=np.int16)
    labels[0, 0, 0] = 1
    image = np.ones(labels.shape, dtype=np.int16)
    for kwargs in (dict(region="ET"), dict(min_lesion_voxels=2)):
        got = texture.lesion_texture(_dev(labels), _dev(image), kwargs.pop("region", "WT"), **kwargs)
        assert got["root"].shape == (0,) and got["hist"].shape == (0, 1) and got["glcm"].shape == (0, 13, 1, 1)
    with pytest.raises(GtsError, match="shape"):
        texture.lesion_texture(_dev(labels), _dev(image[:3]), "WT")
    with pytest.raises(GtsError, match="not supported"):
        texture.lesion_texture(_dev(labels), _dev(image.astype(np.int32)), "WT")
    feats = texture.texture_features(_dev(labels), _dev(image), "WT")
    assert len(feats) == 1 and feats[0]["joint_entropy"] is None and feats[0]["levels"] == 1


# 9. the report and the CLI
def _scan(seed, shape):
    rng = np.random.default_rng(seed)
    labels = np.where(rng.random(shape) < 0.3, rng.choice([1, 2, 3], shape), 0).astype(np.int16)
    return labels, ref.random_image(shape, np.int16, seed), ref.random_image(shape, np.float32, seed + 1)


def _want_report(labels, images, spacing, least, **binning):
    """measure_ref's report with every listed lesion's texture from the reference tables."""
    from gts import texture

    report = measure_ref.tumour_report(labels, spacing, 26, least)
    for region in measure_ref.REGIONS:
        rows = {}
        for name, image in images.items():
            table = ref.lesion_texture(labels, image, region, 26, min_lesion_voxels=least, **binning)
            for k in range(len(table["root"])):
                row = texture.derive(table, k)
                rows.setdefault(row.pop("root"), {})[name] = row
                row.pop("n")
        for m in report[region]["lesions"]:
            m["texture"] = rows[m["root"]]
    return report


def test_report_carries_the_standalone_tables(hip_lib):
    from gts import measure, texture

    labels, t1, t2 = _scan(3, (11, 9, 10))
    images = {"t1": t1, "t2": t2}
    plain = measure.tumour_report(_dev(labels), (1, 1, 2.5), 26, 3)
    got = measure.tumour_report(_dev(labels), (1, 1, 2.5), 26, 3, texture={k: _dev(v) for k, v in images.items()},
                                texture_bins=16)
    assert got == _want_report(labels, images, (1, 1, 2.5), 3, bins=16)
    for region in measure_ref.REGIONS:
        alone = {name: {f.pop("root"): f for f in texture.texture_features(_dev(labels), _dev(image), region, bins=16,
                                                                           min_lesion_voxels=3)}
                 for name, image in images.items()}
        assert len(got[region]["lesions"]) == len(alone["t1"]) > 0
        for m, bare in zip(got[region]["lesions"], plain[region]["lesions"]):
            assert {k: v for k, v in m.items() if k != "texture"} == bare
            assert all(dict(m["texture"][name], n=m["n"]) == alone[name][m["root"]] for name in images)


def test_cli_writes_what_the_reference_predicts(hip_lib, tmp_path):
    from data_processing import labels as label_maps
    from data_processing import nifti_io
    from scripts import measure_tumours as cli

    preds, scans = tmp_path / "preds", tmp_path / "scans"
    preds.mkdir()
    want, bare, exts = {}, [], ["_t1.nii.gz", "_flair.nii.gz"]
    for scan_id, seed, shape in (("scan_a", 1, (9, 8, 7)), ("scan_b", 2, (6, 10, 8))):
        labels, t1, flair = _scan(seed, shape)
        nifti_io.save_as_nifti(labels, str(preds / f"{scan_id}.nii.gz"))
        (scans / scan_id).mkdir(parents=True)
        nifti_io.save_as_nifti(t1, str(scans / scan_id / f"{scan_id}_t1.nii.gz"))
        nifti_io.save_as_nifti(flair, str(scans / scan_id / f"{scan_id}_flair.nii.gz"))
        internal = label_maps.swap_labels_from_brats_any(labels)         # the file holds the 2023 convention
        report = _want_report(internal, {"t1": t1, "flair": flair}, (1.0, 1.0, 1.0), 2, bin_width=50.0)
        want[scan_id] = dict(spacing_mm=[1.0, 1.0, 1.0], regions=report)
        bare += cli.rows_of(scan_id, measure_ref.tumour_report(internal, (1.0, 1.0, 1.0), 26, 2))
    out_csv, out_json, plain_csv = tmp_path / "out" / "r.csv", tmp_path / "out" / "r.json", tmp_path / "out" / "p.csv"
    base = ["-s", str(preds), "--min_lesion_voxels", "2"]
    argv = base + ["-o", str(out_csv), "--json", str(out_json), "--texture", str(scans), "--texture_modalities"] + \
        exts + ["--texture_bin_width", "50"]
    assert cli.main(argv) == 0
    lines = out_csv.read_text().splitlines()
    rows = [row for scan_id in sorted(want) for row in cli.rows_of(scan_id, want[scan_id]["regions"], cli.REGIONS,
                                                                   False, ["t1", "flair"])]
    assert lines == [",".join(cli.HEADER + cli.texture_header(exts))] + [",".join(row) for row in rows]
    assert len(lines) > 12 and json.loads(out_json.read_text()) == json.loads(json.dumps(want))
    assert cli.main(base + ["-o", str(plain_csv)]) == 0      # without the flag: the report as it was
    assert plain_csv.read_text().splitlines() == [",".join(cli.HEADER)] + [",".join(row) for row in bare]
    # a scan whose modality has another shape, one on another grid and one without its file are left out
    labels, t1, flair = _scan(4, (5, 6, 7))
    moved = nifti_io.BRATS_AFFINE.copy()
    moved[0, 3] += 0.5
    for scan_id, t1_volume, affine, with_flair in (("scan_c", t1[:4], nifti_io.BRATS_AFFINE, True),
                                                   ("scan_d", t1, moved, True),
                                                   ("scan_e", t1, nifti_io.BRATS_AFFINE, False)):
        nifti_io.save_as_nifti(labels, str(preds / f"{scan_id}.nii.gz"))
        (scans / scan_id).mkdir()
        nifti_io.save_as_nifti(t1_volume, str(scans / scan_id / f"{scan_id}_t1.nii.gz"), affine)
        if with_flair:
            nifti_io.save_as_nifti(flair, str(scans / scan_id / f"{scan_id}_flair.nii.gz"))
    assert cli.main(argv) == 1
    assert out_csv.read_text().splitlines() == lines
    assert sorted(json.loads(out_json.read_text())) == ["scan_a", "scan_b"]
