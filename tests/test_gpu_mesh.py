"""The mesh kernels on the MI355X (gts/mesh.py, csrc/gts_mesh.hip) against tests/mesh_ref.py: every
array and every table entry equals the numpy statement of the definition exactly, order included; the smoothed
positions and the per-triangle terms equal its ordered float64 loop bit for bit; per-lesion sums stay within
n 2^-52 sum|term| of math.fsum over the reference's terms and are the same bits at every grid_blocks and on every run."""
import math

import numpy as np
import pytest
import torch

from tests import measure_ref
from tests import mesh_ref as ref

pytestmark = pytest.mark.gpu


def _dev(vol):
    return torch.from_numpy(np.ascontiguousarray(vol)).cuda()


def _assert_raw(got, want, note):
    for key in ("vertices_half", "faces", "face_lesion"):
        g = got[key].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == want[key].shape, (note, key, g.shape, want[key].shape)
        assert np.array_equal(g, want[key]), (note, key)
    for key in ("root", "triangles", "classes", "v6"):
        assert got[key].dtype == np.int64 and got[key].shape == want[key].shape, (note, key, got[key].shape)
        assert np.array_equal(got[key], want[key]), (note, key, got[key].tolist()[:8], want[key].tolist()[:8])
    assert not got["classes"][:, 7].any(), note


def _check(name, regions=("WT",), connectivities=(26,), grids=(0,), spacing=(1, 1, 1)):
    from gts import mesh

    dev = _dev(ref.volumes()[name])
    units, scale = measure_ref.spacing_units(spacing)
    for region in regions:
        for connectivity in connectivities:
            want = ref.cached_mesh(name, region, (1, 1, 1), connectivity)
            for grid in grids:
                got = mesh.region_mesh(dev, region, spacing, connectivity, smooth_iterations=0, grid_blocks=grid)
                note = (name, region, connectivity, grid)
                assert got["units"] == units and got["scale_mm"] == scale, note
                _assert_raw(got, want, note)
            positions = ref.positions_mm(want["vertices_half"], units, scale)      # of the last grid: 0 iterations
            assert np.array_equal(got["vertices_mm"].cpu().numpy(), positions), note
            area, volume = ref.face_terms(positions, want["faces"])
            assert np.array_equal(got["face_area_mm2"].cpu().numpy(), area), note
            assert np.array_equal(got["face_volume_mm3"].cpu().numpy(), volume), note
            features = mesh.shape_features(got)
            assert [f["mesh_area_mm2"] for f in features] == [ref.raw_area_mm2(c, units, scale) for c in want["classes"]]
            assert [f["mesh_triangles"] for f in features] == want["triangles"].tolist()
    return got


@pytest.mark.parametrize("connectivity", [26, 6])
def test_all_256_configurations(hip_lib, connectivity):
    want = ref.cached_mesh("configurations", "WT", (1, 1, 1), connectivity)
    assert len(want["root"]) >= 255 and int(want["v6"].sum()) == ref.closed_form_v48(ref.volumes()["configurations"] != 0)
    _check("configurations", connectivities=(connectivity,), grids=(0, 2))


@pytest.mark.parametrize("p", measure_ref.RANDOM_P)
@pytest.mark.parametrize("shape", measure_ref.RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_volumes(hip_lib, shape, p):
    """measure_ref's random volumes at each of its spacings (two of the three are anisotropic): the integers at every
    grid_blocks and both connectivities, the positions and per-triangle terms at every spacing."""
    name = f"random-{'x'.join(map(str, shape))}-{p}"
    _check(name, connectivities=(6, 26), grids=(1, 3, 0), spacing=measure_ref.SPACINGS[0])
    for spacing in measure_ref.SPACINGS[1:]:
        _check(name, spacing=spacing)
    _check(name, regions=("CT", "ET"), spacing=measure_ref.SPACINGS[1])


def test_volume_border(hip_lib):
    got = _check("six-faces", connectivities=(26, 6), grids=(0, 1))
    vertices = got["vertices_half"].cpu().numpy()
    shape = ref.volumes()["six-faces"].shape
    assert vertices.min(axis=0).tolist() == [-1, -1, -1]
    assert vertices.max(axis=0).tolist() == [2 * n - 1 for n in shape]
    _check("faces", regions=measure_ref.REGIONS, connectivities=(26, 6))
    assert _check("plate", regions=("WT", "CT"))["vertices_half"].shape[0] > 0
    one = _check("one", regions=measure_ref.REGIONS)
    assert one["triangles"].tolist() == [24] and one["v6"].tolist() == [24] and one["vertices_half"].shape == (14, 3)


@pytest.mark.parametrize("z1", [63, 64, 65])
def test_cell_rows_at_the_wave_edge(hip_lib, z1):
    """Cell rows of Z + 1 = 63, 64, 65: the lane that takes its lower z face from the lane before it sits at every
    position of the wave relative to a row's start."""
    assert ref.volumes()[f"row-{z1}"].shape[2] + 1 == z1
    _check(f"row-{z1}", connectivities=(26, 6), grids=(0, 1))


@pytest.mark.parametrize("what,count", sorted(ref.COUNT_RECIPES))
def test_counts_at_the_workgroup_edge(hip_lib, what, count):
    """Active cells, vertices and triangles one below, at and one above the workgroup size, and at twice it plus one;
    vertex counts are even and triangle counts multiples of 4 (tests/mesh_ref.py), so their nearest counts stand in."""
    from gts import mesh

    block = 256
    near = {"cells": (block - 1, block, block + 1, 2 * block + 1), "vertices": (block - 2, block, block + 2, 2 * block + 2),
            "triangles": (block - 4, block, block + 4, 2 * block + 4)}[what]
    assert count in near
    name = f"{what}-{count}"
    got = _check(name, connectivities=(26, 6), grids=(0, 1))
    have = dict(cells=ref.active_cells(ref.volumes()[name] != 0), vertices=got["vertices_half"].shape[0],
                triangles=got["faces"].shape[0])
    assert have[what] == count
    smooth = mesh.region_mesh(_dev(ref.volumes()[name]), "WT", smooth_iterations=1)      # T4 and T5 at the same edges
    want = ref.cached_mesh(name, "WT", (1, 1, 1), 26)
    rows = ref.neighbours(want["faces"], len(want["vertices_half"]))
    assert np.array_equal(smooth["vertices_mm"].cpu().numpy(),
                          ref.smooth(ref.positions_mm(want["vertices_half"], (1, 1, 1), 1.0), rows, 1))


def test_empty_region(hip_lib, tmp_path):
    from gts import mesh

    vol = np.zeros((5, 6, 7), dtype=np.int16)
    vol[1:3, 2:4, 3:5] = 1
    for region, iterations in (("ET", 20), ("CT", 0)):
        got = mesh.region_mesh(_dev(vol), region, (1, 0.5, 2.5), smooth_iterations=iterations)
        assert got["vertices_half"].shape == (0, 3) and got["vertices_mm"].shape == (0, 3)
        assert got["faces"].shape == (0, 3) and got["face_lesion"].shape == (0,) and got["root"].shape == (0,)
        assert got["classes"].shape == (0, 8) and mesh.shape_features(got) == []
        path = str(tmp_path / f"{region}.ply")
        mesh.write_ply(path, got, np.eye(4))
        _, vertices, faces, lesion = ref.read_ply(path)
        assert vertices.shape == (0, 3) and faces.shape == (0, 3) and lesion.shape == (0,)
    assert mesh.region_mesh(_dev(np.zeros((1, 1, 1), dtype=np.int16)), "WT")["faces"].shape == (0, 3)


def test_table_capacity_one_lesion_per_cell(hip_lib):
    want = ref.cached_mesh("lattice", "WT", (1, 1, 1), 26)
    assert len(want["root"]) == 1000 and want["triangles"].tolist() == [24] * 1000 and want["v6"].tolist() == [24] * 1000
    _check("lattice", connectivities=(26, 6), grids=(0, 1))


def _smoothing_case(name, spacing, connectivity=26):
    units, scale = measure_ref.spacing_units(spacing)
    want = ref.cached_mesh(name, "WT", (1, 1, 1), connectivity)
    rows = ref.neighbours(want["faces"], len(want["vertices_half"]))
    return want, rows, ref.positions_mm(want["vertices_half"], units, scale)


@pytest.mark.parametrize("name,spacing", [("ellipsoid-interior", (1, 1, 1)), ("random-13x17x9-0.2", (0.9375, 0.9375, 5))])
def test_smoothing(hip_lib, name, spacing):
    from gts import mesh

    dev = _dev(ref.volumes()[name])
    want, rows, start = _smoothing_case(name, spacing)
    raw = mesh.region_mesh(dev, "WT", spacing, smooth_iterations=0)
    assert np.array_equal(raw["vertices_mm"].cpu().numpy(), start)
    positions, done = start, 0
    for iterations in (1, 2, 20):
        positions, done = ref.smooth(positions, rows, iterations - done), iterations      # the loop goes on from 2 to 20
        area, volume = ref.face_terms(positions, want["faces"])
        runs = [mesh.region_mesh(dev, "WT", spacing, smooth_iterations=iterations, grid_blocks=grid)
                for grid in (0, 1, 3, 0)]
        sums = [mesh.lesion_sums(run) for run in runs]
        for run, (got_area, got_volume) in zip(runs, sums):
            assert np.array_equal(run["vertices_mm"].cpu().numpy(), positions), (name, iterations)
            assert np.array_equal(run["face_area_mm2"].cpu().numpy(), area), (name, iterations)
            assert np.array_equal(run["face_volume_mm3"].cpu().numpy(), volume), (name, iterations)
            assert np.array_equal(run["vertices_half"].cpu().numpy(), want["vertices_half"])
            assert got_area.tobytes() == sums[0][0].tobytes() and got_volume.tobytes() == sums[0][1].tobytes()
        for k in range(len(want["root"])):
            for got, terms in ((sums[0][0][k], area[want["face_lesion"] == k]),
                               (sums[0][1][k], volume[want["face_lesion"] == k])):
                bound = len(terms) * 2.0 ** -52 * math.fsum(np.abs(terms))
                print(f"{name} it {iterations} lesion {k}: sum {got!r}, fsum {math.fsum(terms)!r}, bound {bound:.3e}")
                assert abs(got - math.fsum(terms)) <= bound, (name, iterations, k)
        features = mesh.shape_features(runs[0])
        assert [f["smooth_area_mm2"] for f in features] == sums[0][0].tolist()
        for f, a, v in zip(features, sums[0][0].tolist(), sums[0][1].tolist()):
            assert f["smooth_volume_ml"] == v / 1000.0 and f["surface_to_volume_per_mm"] == a / v
            assert f["sphericity"] == (36.0 * math.pi * v * v) ** (1.0 / 3.0) / a


def test_the_ball_is_rounder_after_smoothing(hip_lib):
    from gts import mesh

    got = mesh.region_mesh(_dev(ref.volumes()["ball8"]), "ET")
    (f,) = mesh.shape_features(got)
    sphere = 4.0 * math.pi * 64.0
    assert f["mesh_triangles"] == 7104 and got["v6"].tolist() == [100752]
    assert abs(f["mesh_area_mm2"] / sphere - 1.249) < 5e-4 and abs(f["smooth_area_mm2"] / sphere - 1.039) < 5e-4
    assert abs(f["smooth_volume_ml"] / f["mesh_volume_ml"] - 1.0) < 0.005 and 0.95 < f["sphericity"] < 1.0


def _totals(table):
    return (int(table["triangles"].sum()), int(table["v6"].sum()), table["classes"].sum(axis=0).tolist(),
            sorted(zip(table["triangles"].tolist(), table["v6"].tolist())))


def test_symmetries_of_the_kuhn_triangulation(hip_lib):
    """The six Kuhn tetrahedra of a cell are mapped onto themselves by every permutation of the axes and by the point
    reflection (all three axes mirrored at once), which both keep the main diagonal 000 - 111; a mirror of one or two
    axes moves the diagonal, so the triangulation, and with it the triangle count and the mesh volume, changes.  Under
    a permutation the class counts permute with the axes; under the point reflection they stay."""
    from gts import mesh

    vol = measure_ref.random_volume((13, 17, 9), 0.2)
    base = mesh.region_mesh(_dev(vol), "WT", smooth_iterations=0)
    triangles, v6, classes, lesions = _totals(base)
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        got = _totals(mesh.region_mesh(_dev(vol.transpose(perm)), "WT", smooth_iterations=0))
        permuted = [0] * 8
        for k in range(1, 8):
            n = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
            moved = tuple(n[perm[a]] for a in range(3))           # the new axis a is the old axis perm[a]
            permuted[4 * moved[0] + 2 * moved[1] + moved[2] - 1] = classes[k - 1]
        assert got == (triangles, v6, permuted, lesions), perm
    assert _totals(mesh.region_mesh(_dev(vol[::-1, ::-1, ::-1]), "WT", smooth_iterations=0)) == \
        (triangles, v6, classes, lesions)
    for flip in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):               # not symmetries: the device follows the reference
        mirrored = np.ascontiguousarray(np.flip(vol, flip))
        want = ref.region_mesh(mirrored, "WT")
        got = mesh.region_mesh(_dev(mirrored), "WT", smooth_iterations=0)
        _assert_raw(got, want, flip)
    assert int(ref.region_mesh(np.ascontiguousarray(vol[::-1]), "WT")["v6"].sum()) != v6


@pytest.mark.parametrize("connectivity", [26, 6])
@pytest.mark.parametrize("name", ["lattice", "random-13x17x9-0.31", "zeros-4x4x4", "six-faces"])
def test_tumour_report_through_one_front_end(hip_lib, monkeypatch, name, connectivity):
    """tumour_report(mesh=True) labels each region once and hands the roots to both tables: three component passes a
    scan, and every number and array what lesion_table and region_mesh give when called one by one."""
    from gts import components, measure, mesh

    dev = _dev(np.zeros((4, 4, 4), dtype=np.int16) if name == "zeros-4x4x4" else ref.volumes()[name])
    spacing = (0.9375, 0.9375, 5)
    want, surfaces = {}, {}
    for region in measure_ref.REGIONS:
        surfaces[region] = mesh.region_mesh(dev, region, spacing, connectivity, smooth_iterations=3)
        want[region] = measure.report_from_table(measure.lesion_table(dev, region, spacing, connectivity), 1,
                                                 mesh.shape_features(surfaces[region]))
    calls, labelling = [], components.roots_unchecked

    def counting(*args, **kwargs):
        calls.append(args[2])
        return labelling(*args, **kwargs)

    monkeypatch.setattr(components, "roots_unchecked", counting)
    meshes = {}
    got = measure.tumour_report(dev, spacing, connectivity, mesh=True, smooth_iterations=3, meshes=meshes)
    assert calls == [connectivity] * 3, calls
    assert got == want                                   # Python's ==: every float bit for bit (no NaN among them)
    assert sorted(meshes) == sorted(measure_ref.REGIONS)
    for region in measure_ref.REGIONS:
        for key in ("faces", "face_lesion", "vertices_mm"):
            assert np.array_equal(meshes[region][key].cpu().numpy(), surfaces[region][key].cpu().numpy()), (region, key)


def test_cli_with_and_without_mesh(hip_lib, tmp_path):
    from data_processing import labels as label_maps
    from data_processing import nifti_io
    from gts import measure, mesh
    from scripts import measure_tumours as cli

    rng = np.random.default_rng(5)
    a = np.zeros((12, 11, 9), dtype=np.int16)
    a[2:9, 3:8, 2:7] = np.where(rng.random((7, 5, 5)) < 0.8, rng.choice([1, 2, 4], (7, 5, 5)), 0)
    a[10, 9, 8] = 4
    b = np.where(rng.random((9, 10, 8)) < 0.3, rng.choice([1, 2, 3], (9, 10, 8)), 0).astype(np.int16)
    coarse = np.array([[0, -0.9375, 0, 3.0], [0.9375, 0, 0, -7.0], [0, 0, 5.0, 11.0], [0, 0, 0, 1.0]])
    preds, meshes = tmp_path / "preds", tmp_path / "meshes"
    preds.mkdir()
    nifti_io.save_as_nifti(a, str(preds / "scan_a.nii.gz"), coarse)
    nifti_io.save_as_nifti(b, str(preds / "scan_b.nii.gz"))
    nifti_io.save_as_nifti(np.zeros((4, 4, 4), dtype=np.int16), str(preds / "scan_c.nii.gz"))
    cases = (("scan_a", a, (0.9375, 0.9375, 5.0)), ("scan_b", b, (1.0, 1.0, 1.0)),
             ("scan_c", np.zeros((4, 4, 4), dtype=np.int16), (1.0, 1.0, 1.0)))
    plain_csv, wide_csv = tmp_path / "plain.csv", tmp_path / "wide.csv"
    plain_json, wide_json = tmp_path / "plain.json", tmp_path / "wide.json"
    assert cli.main(["-s", str(preds), "-o", str(plain_csv), "--json", str(plain_json)]) == 0
    assert cli.main(["-s", str(preds), "-o", str(wide_csv), "--json", str(wide_json), "--mesh", "--mesh_smooth", "3",
                     "--mesh_dir", str(meshes)]) == 0
    plain_rows, wide_rows = [], []
    for scan_id, vol, spacing in cases:
        dev = _dev(label_maps.swap_labels_from_brats_any(vol))
        report = measure.tumour_report(dev, spacing)
        plain_rows += cli.rows_of(scan_id, report)
        for region in measure_ref.REGIONS:
            surface = mesh.region_mesh(dev, region, spacing, smooth_iterations=3)
            features = mesh.shape_features(surface)
            by_root = dict(zip(surface["root"].tolist(), features))
            for rank, lesion in enumerate(report[region]["lesions"], 1):
                wide_rows.append([scan_id, region, str(rank)] + [cli._cell(by_root[lesion["root"]][k]) for k in cli.MESH_HEADER])
            wide_rows.append([scan_id, region, "total"] + [""] * 7)
            _, world, faces, lesion = ref.read_ply(str(meshes / f"{scan_id}_{region}.ply"))
            assert np.array_equal(faces, surface["faces"].cpu().numpy()) and ref.is_closed_manifold(faces)
            assert np.array_equal(lesion, surface["face_lesion"].cpu().numpy())
            affine, _ = nifti_io.read_affine(str(preds / f"{scan_id}.nii.gz"))
            index = surface["vertices_mm"].cpu().numpy() / np.array(spacing)
            assert np.array_equal(world, (index @ affine[:3, :3].T + affine[:3, 3]).astype(np.float32))
    # without the flag: byte for byte rows_of over tumour_report, as before the feature
    assert plain_csv.read_text() == "".join(",".join(row) + "\n" for row in [cli.HEADER] + plain_rows)
    lines = [line.split(",") for line in wide_csv.read_text().splitlines()]
    assert lines[0] == cli.HEADER + cli.MESH_HEADER
    assert [line[:len(cli.HEADER)] for line in lines[1:]] == plain_rows
    assert [line[:3] + line[len(cli.HEADER):] for line in lines[1:]] == wide_rows
    assert any(row[3] != "" and float(row[3]) > 0 for row in wide_rows)
    import json
    plain, wide = json.loads(plain_json.read_text()), json.loads(wide_json.read_text())
    for scan_id in plain:
        for region in measure_ref.REGIONS:
            for m_plain, m_wide in zip(plain[scan_id]["regions"][region]["lesions"], wide[scan_id]["regions"][region]["lesions"]):
                assert {k: v for k, v in m_wide.items() if k not in cli.MESH_HEADER} == m_plain
                assert set(m_wide) - set(m_plain) == set(cli.MESH_HEADER)
