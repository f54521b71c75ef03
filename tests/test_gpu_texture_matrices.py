"""The run, zone and neighbourhood kernels on the MI355X (X4-X6, csrc/gts_texture_matrices.hip) against
tests/texture_matrices_ref.py: every integer of glrlm, zones, gldm, ngtdm_n and ngtdm_s equals the scipy / numpy
definition, for int16 and float32 scans and at grid_blocks 0, 1 and 7; the identities that give back the histogram
hold; every other key equals the call without `matrices`.  The float features, derived from equal tables, are held to
the exact reference by tests/test_texture_matrices_host.py."""
import json

import numpy as np
import pytest
import torch

from tests import measure_ref
from tests import texture_matrices_ref as mref
from tests import texture_ref as ref

pytestmark = pytest.mark.gpu

GRIDS = (0, 1, 7)
BASE_KEYS = ("root", "n", "lo", "hi", "levels", "hist", "glcm")


def _dev(vol):
    return torch.from_numpy(np.ascontiguousarray(vol)).cuda()


def _assert_equal(got, want, note):
    for key in mref.TABLE_KEYS:
        assert got[key].dtype == np.int64 and got[key].shape == want[key].shape, (note, key, got[key].shape,
                                                                                  want[key].shape)
        assert np.array_equal(got[key], want[key]), (note, key, np.argwhere(got[key] != want[key])[:4])
    assert mref.identities_hold(got), note


def _check(labels, image, region="WT", connectivity=26, grids=GRIDS, want=None, both_dtypes=True, alpha=0, **binning):
    """lesion_texture with every family at every grid against the reference, for the image as it is and (int16
    images) as float32, whose levels are the same; the other keys against the call without `matrices`."""
    from gts import texture

    if want is None:
        want = mref.lesion_matrices(labels, image, region, connectivity, binning.get("bins", 32),
                                    binning.get("bin_width"), binning.get("min_lesion_voxels", 1), alpha)
    images = [image] + ([image.astype(np.float32)] if both_dtypes and image.dtype == np.int16 else [])
    for img in images:
        plain = texture.lesion_texture(_dev(labels), _dev(img), region, connectivity, **binning)
        assert set(plain) == set(BASE_KEYS) | {"bins", "bin_width"}
        for grid in grids:
            note = (img.dtype, region, connectivity, grid, alpha, binning)
            got = texture.lesion_texture(_dev(labels), _dev(img), region, connectivity, grid_blocks=grid,
                                         matrices=texture.MATRICES, dependence_alpha=alpha, **binning)
            _assert_equal(got, want, note)
            assert set(got) == set(plain) | set(mref.TABLE_KEYS), note
            for key in BASE_KEYS:
                assert got[key].dtype == plain[key].dtype and np.array_equal(got[key], plain[key]), (note, key)
            assert (got["bins"], got["bin_width"]) == (plain["bins"], plain["bin_width"]), note
    return want


def _columns(row):
    return {int(c): int(row[c]) for c in np.flatnonzero(row)}


# 1. closed forms
@pytest.mark.parametrize("name", sorted(ref.box_cases()))
def test_constant_box_closed_form(hip_lib, name):
    labels, image = ref.box_cases()[name]
    want = _check(labels, image)
    extent = (3, 3, 1) if name == "unit-axis" else ref.BOX
    assert want["zones"].tolist() == [[0, 0, int(np.prod(extent)), 1]] and want["ngtdm_s"].sum() == 0
    if name != "unit-axis":
        assert _columns(want["glrlm"][0, 0, 0]) == {4: 6} and _columns(want["gldm"][0, 0]) == {7: 8, 11: 16, 17: 6}


# 2. ramp and checkerboard
def test_ramp_and_checkerboard(hip_lib):
    labels, image, (a, b, c) = ref.ramp_case()
    want = _check(labels, image, bins=a)
    assert want["zones"].tolist() == [[0, g, b * c, 1] for g in range(a)]            # one slab per level
    assert want["glrlm"][0, ref.DIRECTIONS.index((1, 0, 0)), :, 0].tolist() == [b * c] * a
    labels, image, _ = ref.checkerboard_case()
    want = _check(labels, image, region="CT", bins=2)
    assert want["zones"].tolist() == [[0, 0, 30, 1], [0, 1, 30, 1]]
    assert _columns(want["ngtdm_s"][0, 1]) == {7: 16, 11: 72, 17: 99, 26: 42}


# 3. the same root, not the same mask
@pytest.mark.parametrize("bins", [1, 32])
def test_lesions_that_touch_share_nothing(hip_lib, bins):
    labels, image = ref.touching_case()
    six = _check(labels, image, connectivity=6, bins=bins)
    whole = _check(labels, image, connectivity=26, bins=bins)
    assert len(six["root"]) == 3 and len(whole["root"]) == 1
    if bins == 1:        # the levels coincide: a diagonal run, a zone or a neighbourhood that ignored the root would join
        assert six["zones"].tolist() == [[k, 0, 12, 1] for k in range(3)] and whole["zones"].tolist() == [[0, 0, 36, 1]]
        assert six["glrlm"].shape[3] == 3 and whole["glrlm"].shape[3] > 3
        assert six["ngtdm_n"][:, 0, 12:].sum() == 0 and whole["ngtdm_n"][0, 0, 12:].sum() > 0


# 4. chunk edges
@pytest.mark.parametrize("voxels", [2047, 2048, 2049, 4097])
def test_chunk_edges(hip_lib, voxels):
    from gts import texture

    labels, image = ref.chunk_case(voxels, texture.CHUNK)
    want = _check(labels, image, both_dtypes=False)
    assert want["n"].tolist() == [voxels] and len(texture.chunk_units(want["n"])) == -(-voxels // texture.CHUNK)
    assert want["gldm"].sum() == voxels == want["ngtdm_n"].sum()


# 5. level edges
@pytest.mark.parametrize("bins", [1, 2, 32, 128])
def test_bin_numbers(hip_lib, bins):
    name, labels, image = ref.cached_selection()[21]         # 1 x 40 x 33 at 0.31, float32
    want = _check(labels, image, bins=bins, min_lesion_voxels=2)
    assert (want["levels"] == bins).any() and want["gldm"].shape[1] == bins


def test_bin_width_of_128_levels(hip_lib):
    line = np.full((1, 1, 130), 1, dtype=np.int16)
    ramp = np.arange(130, dtype=np.int16).reshape(1, 1, 130) - 40
    line[0, 0, 128:] = 0
    want = _check(line, ramp, bin_width=1.0)                 # exactly 128 levels, every voxel a run and a zone
    assert want["levels"].tolist() == [128] and want["zones"].tolist() == [[0, g, 1, 1] for g in range(128)]
    assert want["glrlm"].shape == (1, 13, 128, 1) and want["ngtdm_s"][0, 127].sum() == 1
    block = np.full((2, 3, 4), 2, dtype=np.int16)
    values = np.float32([-2.5, -2.0, -1.99, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.49, 1.5, 1.51, 2.0, 2.5, 3.0,
                         -1.0, -1.5, -0.75, 0.1, 0.2, 0.3, -0.1, -0.2]).reshape(2, 3, 4)
    _check(block, values, bin_width=0.5)


# 6. contention
@pytest.mark.parametrize("name", sorted(ref.contention_cases()))
def test_contention(hip_lib, name):
    labels, image, bins = ref.contention_cases()[name]
    want = _check(labels, image, bins=bins, both_dtypes=False)
    if name == "constant":                                   # one zone, and every run of a direction on one counter
        assert want["zones"].tolist() == [[0, 0, 4096, 1]] and want["glrlm"].shape == (1, 13, 1, 16)
        # 256 full lines along Z and along Y; along (0, 1, -1) one full diagonal per plane of constant x
        assert want["glrlm"][0, :3, 0, 15].tolist() == [256, 16, 256] and want["gldm"][0, 0, 26] == 14 ** 3
    else:
        assert want["levels"].tolist() == [128] and len(want["zones"]) > 128


# 7. a run longer than a workgroup and than the LDS run tile; a zone that is one long chain; union-find depth
def test_line_and_serpentine(hip_lib):
    want = _check(*mref.line_case())
    assert want["glrlm"].shape == (1, 13, 1, 300) and want["glrlm"][0, 0, 0, 299] == 1
    assert want["zones"].tolist() == [[0, 0, 300, 1]]
    want = _check(*mref.serpentine_case())
    assert want["zones"].tolist() == [[0, 0, 275, 1], [0, 31, 157, 1]]
    across = np.ascontiguousarray(mref.line_case(70)[0].transpose(2, 0, 1))             # the line along X: 70 Z lines
    want = _check(across, np.full(across.shape, 5, dtype=np.int16))
    assert want["zones"].tolist() == [[0, 0, 70, 1]] and want["glrlm"][0, ref.DIRECTIONS.index((1, 0, 0)), 0, 69] == 1


# 8. the tolerance of the dependence
@pytest.mark.parametrize("alpha", [0, 1, 128])
def test_dependence_alpha(hip_lib, alpha):
    name, labels, image = ref.cached_selection()[9]          # 16 x 16 x 16 at 0.31
    want = _check(labels, image, alpha=alpha, both_dtypes=False, min_lesion_voxels=5)
    if alpha == 128:                                         # every neighbour depends
        assert np.array_equal(want["gldm"], want["ngtdm_n"])
    labels, image, _ = ref.ramp_case()
    want = _check(labels, image, bins=6, alpha=alpha)
    assert (want["gldm"][0, :, 26].sum() > 0) == (alpha >= 1)


# 9. selection
@pytest.mark.parametrize("index", range(len(ref.selection_cases())), ids=[c[0] for c in ref.selection_cases()])
def test_selection_on_random_volumes(hip_lib, index):
    name, labels, image = ref.cached_selection()[index]
    for connectivity in (6, 26):
        for least in (1, 5):
            want = mref.cached_selection_matrices(index, connectivity, least)
            _check(labels, image, connectivity=connectivity, want=want, both_dtypes=False, min_lesion_voxels=least)


def test_empty_region(hip_lib):
    from gts import texture

    labels = np.zeros((4, 5, 6), dtype=np.int16)
    labels[0, 0, 0] = 1
    image = np.ones(labels.shape, dtype=np.int16)
    for kwargs in (dict(region="ET"), dict(min_lesion_voxels=2)):
        got = texture.lesion_texture(_dev(labels), _dev(image), kwargs.pop("region", "WT"),
                                     matrices=texture.MATRICES, **kwargs)
        assert {key: got[key].shape for key in mref.TABLE_KEYS} == dict(
            glrlm=(0, 13, 1, 1), zones=(0, 4), gldm=(0, 1, 27), ngtdm_n=(0, 1, 27), ngtdm_s=(0, 1, 27))
        assert got["glcm"].shape == (0, 13, 1, 1) and all(got[key].dtype == np.int64 for key in mref.TABLE_KEYS)
    got = texture.lesion_texture(_dev(labels), _dev(image), "WT", matrices=("glszm",))
    assert got["zones"].tolist() == [[0, 0, 1, 1]] and "glrlm" not in got and "gldm" not in got
    feats = texture.texture_features(_dev(labels), _dev(image), "WT", matrices=("ngtdm", "glszm"))
    assert feats[0]["ngtdm_coarseness"] is None and feats[0]["glszm_zone_percentage"] == 1.0
    assert "glrlm_run_entropy" not in feats[0]


# 10. the report and the CLI
def _scan(seed, shape):
    rng = np.random.default_rng(seed)
    labels = np.where(rng.random(shape) < 0.3, rng.choice([1, 2, 3], shape), 0).astype(np.int16)
    return labels, ref.random_image(shape, np.int16, seed), ref.random_image(shape, np.float32, seed + 1)


def _want_report(labels, images, spacing, least, alpha, **binning):
    """measure_ref's report with every listed lesion's texture from the reference tables."""
    from gts import texture

    report = measure_ref.tumour_report(labels, spacing, 26, least)
    for region in measure_ref.REGIONS:
        rows = {}
        for name, image in images.items():
            table = mref.lesion_matrices(labels, image, region, 26, min_lesion_voxels=least, dependence_alpha=alpha,
                                         **binning)
            for k in range(len(table["root"])):
                row = texture.derive(table, k)
                rows.setdefault(row.pop("root"), {})[name] = row
                row.pop("n")
        for m in report[region]["lesions"]:
            m["texture"] = rows[m["root"]]
    return report


def test_report_carries_the_new_families(hip_lib):
    from gts import measure, texture

    labels, t1, t2 = _scan(3, (11, 9, 10))
    images = {"t1": t1, "t2": t2}
    tensors = {k: _dev(v) for k, v in images.items()}
    plain = measure.tumour_report(_dev(labels), (1, 1, 2.5), 26, 3, texture=tensors, texture_bins=16)
    got = measure.tumour_report(_dev(labels), (1, 1, 2.5), 26, 3, texture=tensors, texture_bins=16,
                                texture_matrices=texture.MATRICES, texture_dependence_alpha=1)
    assert got == _want_report(labels, images, (1, 1, 2.5), 3, 1, bins=16)
    new = set(texture.GLRLM_KEYS + texture.GLSZM_KEYS + texture.GLDM_KEYS + texture.NGTDM_KEYS)
    for region in measure_ref.REGIONS:
        assert len(got[region]["lesions"]) == len(plain[region]["lesions"]) > 0
        for m, bare in zip(got[region]["lesions"], plain[region]["lesions"]):
            for name in images:
                assert set(m["texture"][name]) == set(bare["texture"][name]) | new
                assert {k: v for k, v in m["texture"][name].items() if k not in new} == bare["texture"][name]
    some = measure.tumour_report(_dev(labels), (1, 1, 2.5), 26, 3, texture=tensors, texture_bins=16,
                                 texture_matrices=("glszm",))
    assert set(some["WT"]["lesions"][0]["texture"]["t1"]) == set(plain["WT"]["lesions"][0]["texture"]["t1"]) | \
        set(texture.GLSZM_KEYS)


def test_cli_writes_what_the_reference_predicts(hip_lib, tmp_path):
    from data_processing import labels as label_maps
    from data_processing import nifti_io
    from scripts import measure_tumours as cli

    preds, scans = tmp_path / "preds", tmp_path / "scans"
    preds.mkdir()
    want, exts = {}, ["_t1.nii.gz", "_flair.nii.gz"]
    for scan_id, seed, shape in (("scan_a", 1, (9, 8, 7)), ("scan_b", 2, (6, 10, 8))):
        labels, t1, flair = _scan(seed, shape)
        nifti_io.save_as_nifti(labels, str(preds / f"{scan_id}.nii.gz"))
        (scans / scan_id).mkdir(parents=True)
        nifti_io.save_as_nifti(t1, str(scans / scan_id / f"{scan_id}_t1.nii.gz"))
        nifti_io.save_as_nifti(flair, str(scans / scan_id / f"{scan_id}_flair.nii.gz"))
        internal = label_maps.swap_labels_from_brats_any(labels)         # the file holds the 2023 convention
        report = _want_report(internal, {"t1": t1, "flair": flair}, (1.0, 1.0, 1.0), 2, 1, bin_width=50.0)
        want[scan_id] = dict(spacing_mm=[1.0, 1.0, 1.0], regions=report)
    out = tmp_path / "out"
    base = ["-s", str(preds), "--min_lesion_voxels", "2", "--texture", str(scans), "--texture_modalities"] + exts + \
        ["--texture_bin_width", "50"]
    argv = base + ["-o", str(out / "r.csv"), "--json", str(out / "r.json"), "--texture_matrices", "all",
                   "--texture_dependence_alpha", "1"]
    assert cli.main(argv) == 0
    lines = (out / "r.csv").read_text().splitlines()
    rows = [row for scan_id in sorted(want) for row in cli.rows_of(scan_id, want[scan_id]["regions"], cli.REGIONS,
                                                                   False, ["t1", "flair"], cli.TEXTURE_MATRICES)]
    assert lines == [",".join(cli.HEADER + cli.texture_header(exts, cli.TEXTURE_MATRICES))] + \
        [",".join(row) for row in rows]
    assert len(lines) > 12 and json.loads((out / "r.json").read_text()) == json.loads(json.dumps(want))
    # without the new flags: the columns of --texture alone, which the longer rows begin with
    assert cli.main(base + ["-o", str(out / "p.csv")]) == 0
    width = len(cli.HEADER) + 2 * 37
    before = (out / "p.csv").read_text().splitlines()
    assert before[0] == ",".join(cli.HEADER + cli.texture_header(exts))
    assert before == [",".join(line.split(",")[:width]) for line in lines]
    assert cli.main(base + ["-o", str(out / "z.csv"), "--texture_matrices", "ngtdm", "glszm"]) == 0
    some = (out / "z.csv").read_text().splitlines()
    assert some[0] == ",".join(cli.HEADER + cli.texture_header(exts, ["glszm", "ngtdm"]))
    assert len(some) == len(lines) and len(some[1].split(",")) == width + 2 * 21
