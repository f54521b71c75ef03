"""The measurement kernels on the MI355X (gts/measure.py, csrc/gts_measure.hip) against
tests/measure_ref.py: every field of the integer table equals the unpruned numpy definition, and the float64
quantities, being the same expressions over the same integers, equal it bit for bit.  No reference lesion exceeds
4 096 voxels (tests/test_measure_host.py checks what the reference costs)."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import measure_ref as ref

pytestmark = pytest.mark.gpu

KEYS = ("root", "n", "n_class", "box", "coord_sum", "faces", "d3", "plane_z", "plane_d2", "plane_w")


def _dev(vol):
    return torch.from_numpy(np.ascontiguousarray(vol)).cuda()


def _assert_equal(got, want, units, scale, note):
    from gts import measure

    assert got["units"] == units and got["scale_mm"] == scale, note
    for key in KEYS:
        assert got[key].dtype == np.int64 and got[key].shape == want[key].shape, (note, key, got[key].shape)
        assert np.array_equal(got[key], want[key]), (note, key, got[key].tolist()[:8], want[key].tolist()[:8])
    assert [measure.derive(got, k) for k in range(len(got["n"]))] == \
        [ref.derive(want, k, units, scale) for k in range(len(want["n"]))], note


def _check(name, regions=ref.REGIONS, spacings=((1, 1, 1),), connectivities=(26,), grids=(0,)):
    from gts import measure

    dev = _dev(ref.cached_volumes()[name])
    for spacing in spacings:
        units, scale = ref.spacing_units(spacing)
        for region in regions:
            for connectivity in connectivities:
                want = ref.cached_table(name, region, units, connectivity)
                for grid in grids:
                    got = measure.lesion_table(dev, region, spacing, connectivity, grid_blocks=grid)
                    _assert_equal(got, want, units, scale, (name, region, spacing, connectivity, grid))


@pytest.mark.parametrize("p", ref.RANDOM_P)
@pytest.mark.parametrize("shape", ref.RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_volumes(hip_lib, shape, p):
    _check(f"random-{'x'.join(map(str, shape))}-{p}", spacings=ref.SPACINGS, connectivities=(6, 26))


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_pair_tile_edges(hip_lib, count):
    """Every voxel of a checkerboard is a candidate: lists of T - 1, T, T + 1 and 2 T + 1 for M3's tile."""
    from gts import _lib, measure

    tile = _lib.const("GTS_MEASURE_PAIR_TILE")
    assert count in (tile - 1, tile, tile + 1, 2 * tile + 1)
    name = f"board3-{count}"
    got = measure.lesion_table(_dev(ref.cached_volumes()[name]), "WT")
    assert got["n"].tolist() == [count] == got["candidates"].tolist()
    _check(name, spacings=((1, 1, 1), (1, 0.5, 2.5)))
    _check(name, regions=("WT",), connectivities=(6,))       # every voxel its own lesion: more rows than 2x2x2 cells
    assert len(ref.cached_table(name, "WT", (1, 1, 1), 6)["n"]) == count


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_plane_tile_edges(hip_lib, count):
    """A one-slice checkerboard footprint: in-plane lists of T - 1, T, T + 1 and 2 T + 1 for M4's tile."""
    from gts import _lib, measure

    tile = _lib.const("GTS_MEASURE_PLANE_TILE")
    assert count in (tile - 1, tile, tile + 1, 2 * tile + 1)
    name = f"board2-{count}"
    got = measure.lesion_table(_dev(ref.cached_volumes()[name]), "WT")
    assert got["n"].tolist() == [count] and got["plane_candidates"] == count
    _check(name, spacings=((1, 1, 1), (0.9375, 0.9375, 5)))


def test_table_capacity_one_lesion_per_cell(hip_lib):
    want = ref.cached_table("lattice", "WT", (1, 1, 1), 26)
    assert len(want["n"]) == 1000 and not want["d3"].any() and not want["plane_w"].any()
    _check("lattice", connectivities=(6, 26))


@pytest.mark.parametrize("shape_name", ["box", "ellipsoid", "tie"])
def test_closed_forms_at_corner_face_and_interior(hip_lib, shape_name):
    from gts import measure

    pinned = dict(box=(30, [12, 20, 30], 21, 20, 16), ellipsoid=(464, [112, 112, 224], 131, 130, 130),
                  tie=(5, [6, 6, 10], 5, 5, 4))[shape_name]
    names = [f"{shape_name}-{where}" for where in ("corner", "face", "interior")]
    names += ["tie-alone"] if shape_name == "tie" else []
    for name in names:
        got = measure.lesion_table(_dev(ref.cached_volumes()[name]), "ET")
        assert (got["n"].tolist(), got["faces"].tolist(), got["d3"].tolist(), got["plane_d2"].tolist(),
                got["plane_w"].tolist()) == ([pinned[0]], [pinned[1]], [pinned[2]], [pinned[3]], [pinned[4]]), name
        _check(name, spacings=ref.SPACINGS, connectivities=(6, 26))
    if shape_name == "tie":
        assert ref.cached_volumes()["tie-alone"].shape == (3, 3, 1)


def test_lesion_touching_all_six_faces(hip_lib):
    want = ref.cached_table("faces", "WT", (1, 1, 1), 26)
    assert want["box"][want["n"].argmax()].tolist() == [0, 9, 0, 8, 0, 7]
    _check("faces", spacings=ref.SPACINGS, connectivities=(6, 26))


def _multiset(table, keys):
    cols = [table[k].reshape(len(table["n"]), -1) for k in keys]
    return sorted(map(tuple, np.concatenate(cols, axis=1).tolist()))


@pytest.mark.parametrize("name", ["random-13x17x9-0.31", "tie-interior", "ellipsoid-face"])
def test_mirror_invariance(hip_lib, name):
    from gts import measure

    vol = ref.cached_volumes()[name]
    spacing = (1, 0.5, 2.5)
    units, scale = ref.spacing_units(spacing)
    plain = measure.lesion_table(_dev(vol), "WT", spacing)
    kept = ["n", "faces", "d3", "plane_d2", "plane_w"]
    for axis in range(3):
        flipped = np.ascontiguousarray(np.flip(vol, axis))
        got = measure.lesion_table(_dev(flipped), "WT", spacing)
        _assert_equal(got, ref.lesion_table(flipped, "WT", units), units, scale, (name, axis))
        keys = kept + (["plane_z"] if axis < 2 else [])       # the lesions come in another order: compare as multisets
        assert _multiset(got, keys) == _multiset(plain, keys), (name, axis)


@pytest.mark.parametrize("name", ["lattice", "random-16x16x16-0.45", "random-33x5x20-0.2", "board3-513", "board2-513"])
def test_launch_geometry(hip_lib, name):
    _check(name, regions=("WT", "CT"), spacings=((0.9375, 0.9375, 5),), grids=(1, 7, 0, 4096))


def test_limits_and_empty_regions(hip_lib):
    from gts import GtsError, measure

    lib = hip_lib
    line = torch.zeros((4097, 1, 1), dtype=torch.int16, device="cuda")
    line[5:9] = 3
    fine = measure.lesion_table(line, "ET", (37.0727, 1, 1))        # 4096 * 370 727 < 2^30.5, the last unit that fits
    assert fine["units"] == (370727, 10000, 10000) and fine["n"].tolist() == [4]
    assert fine["d3"].tolist() == [9 * 370727 ** 2] and fine["plane_w"].tolist() == [0]
    with pytest.raises(GtsError, match="outside the kernels' limits"):
        measure.lesion_table(line, "ET", (99.9999, 1, 1))            # units (999 999, 10 000, 10 000): 2 B >= 2^62
    x, y, z = line.shape
    ws, ints = lib.gts_measure_workspace(x, y, z), lib.gts_measure_table_i64s(x, y, z, 26)
    workspace = torch.zeros(ws, dtype=torch.uint8, device="cuda")
    table = torch.zeros(ints, dtype=torch.int64, device="cuda")
    work = torch.zeros(4, dtype=torch.int32, device="cuda")
    units = (ctypes.c_int64 * 3)(999999, 10000, 10000)
    assert lib.gts_measure_diameters(x, y, z, units, work.data_ptr(), 1, table.data_ptr(), ints, workspace.data_ptr(),
                                     ws, 0, None) == -2
    assert lib.gts_measure_planes(x, y, z, units, work.data_ptr(), 1, table.data_ptr(), 1, table.data_ptr(), ints,
                                  workspace.data_ptr(), ws, 0, None) == -2
    torch.cuda.synchronize()
    assert not table.any()                                            # nothing ran
    for vol, region in ((torch.zeros((6, 5, 4), dtype=torch.int16, device="cuda"), "WT"),
                        (torch.ones((6, 5, 4), dtype=torch.int16, device="cuda"), "ET")):
        got = measure.lesion_table(vol, region, (1, 0.5, 2.5))
        want = ref.lesion_table(vol.cpu().numpy(), region, (2, 1, 5))
        _assert_equal(got, want, (2, 1, 5), 0.5, region)
        assert len(got["n"]) == 0 and got["box"].shape == (0, 6) and got["plane_candidates"] == 0
        assert measure.lesion_measurements(vol, region) == []
    report = measure.tumour_report(torch.ones((6, 5, 4), dtype=torch.int16, device="cuda"), (1, 0.5, 2.5))
    assert report == ref.tumour_report(np.ones((6, 5, 4), dtype=np.int16), (1, 0.5, 2.5))
    assert report["WT"]["n_lesions"] == 1 and report["CT"]["lesions"] == [] and report["ET"]["ml"] == 0.0


def test_report_lists_large_lesions_and_counts_all(hip_lib):
    from gts import measure

    vol = ref.cached_volumes()["random-13x17x9-0.1"]
    for connectivity, least in ((26, 1), (26, 4), (6, 2)):
        got = measure.tumour_report(_dev(vol), (0.9375, 0.9375, 5), connectivity, least)
        assert got == ref.tumour_report(vol, (0.9375, 0.9375, 5), connectivity, least)
    assert got["WT"]["n_lesions"] > len(got["WT"]["lesions"]) > 0


def test_cli_writes_what_the_reference_predicts(hip_lib, tmp_path):
    from data_processing import labels as label_maps
    from data_processing import nifti_io
    from scripts import measure_tumours as cli

    rng = np.random.default_rng(11)
    old = np.where(rng.random((12, 11, 7)) < 0.25, rng.choice([1, 2, 4], (12, 11, 7)), 0).astype(np.int16)
    new = np.where(rng.random((9, 10, 8)) < 0.4, rng.choice([1, 2, 3], (9, 10, 8)), 0).astype(np.int16)
    empty = np.zeros((5, 6, 7), dtype=np.int16)
    coarse = np.diag([0.9375, 0.9375, 5.0, 1.0])
    preds = tmp_path / "preds"
    preds.mkdir()
    nifti_io.save_as_nifti(old, str(preds / "scan_a.nii.gz"), coarse)
    nifti_io.save_as_nifti(new, str(preds / "scan_b.nii.gz"))
    nifti_io.save_as_nifti(empty, str(preds / "scan_c.nii.gz"))
    want = {}
    for scan_id, vol, spacing in (("scan_a", old, (0.9375, 0.9375, 5.0)), ("scan_b", new, (1.0, 1.0, 1.0)),
                                  ("scan_c", empty, (1.0, 1.0, 1.0))):
        assert cli.spacing_of(str(preds / f"{scan_id}.nii.gz")) == spacing
        internal = label_maps.swap_labels_from_brats_any(vol)
        want[scan_id] = dict(spacing_mm=list(spacing), regions=ref.tumour_report(internal, spacing, 26, 2))
    out_csv, out_json = tmp_path / "out" / "report.csv", tmp_path / "out" / "report.json"
    argv = ["-s", str(preds), "-o", str(out_csv), "--json", str(out_json), "--min_lesion_voxels", "2"]
    assert cli.main(argv) == 0
    lines = out_csv.read_text().splitlines()
    rows = [row for scan_id in sorted(want) for row in cli.rows_of(scan_id, want[scan_id]["regions"])]
    assert lines == [",".join(cli.HEADER)] + [",".join(row) for row in rows]
    assert sum(line.split(",")[2] == "total" for line in lines) == 9 and len(lines) > 20
    assert json.loads(out_json.read_text()) == json.loads(json.dumps(want))
    both = old.copy()
    both[0, 0, :2] = (3, 4)
    nifti_io.save_as_nifti(both, str(preds / "scan_d.nii.gz"))
    assert cli.main(argv + ["--regions", "ET"]) == 1
    lines = out_csv.read_text().splitlines()
    assert {line.split(",")[0] for line in lines[1:]} == {"scan_a", "scan_b", "scan_c"}
    assert {line.split(",")[1] for line in lines[1:]} == {"ET"}
    assert sorted(json.loads(out_json.read_text())) == ["scan_a", "scan_b", "scan_c"]
