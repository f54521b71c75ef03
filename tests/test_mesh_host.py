"""The tumour surfaces without a GPU (gts/mesh.py, csrc/gts_mesh.hip): tests/mesh_ref.py, the numpy
statement of the definition, against closed forms it does not share code with (the (0, 1, 4, 7, 8) volume rule,
Euler characteristics, the pinned ball); the PLY writer; the CLI's rows with and without --mesh; and the entry
points' refusals, which happen before anything touches the device."""
import ctypes
import math

import numpy as np
import pytest

from tests import measure_ref
from tests import mesh_ref as ref


read_ply = ref.read_ply


def test_all_256_cell_configurations():
    """Each configuration alone in a 2 x 2 x 2 volume: a closed manifold, a positive volume equal to the tetrahedron
    rule's, and no normal outside the seven classes."""
    for m in range(1, 256):
        mask = np.array([(m >> d) & 1 for d in range(8)], dtype=bool).reshape(2, 2, 2)
        vertices, faces, roots = ref.surface(mask)
        assert ref.is_closed_manifold(faces), m
        table = ref.integer_table(vertices, faces, roots)
        assert table["v6"].tolist() == [ref.closed_form_v48(mask)] and table["v6"][0] > 0, m
        assert table["classes"][0, 7] == 0 and table["classes"][0].sum() == len(faces) == table["triangles"][0], m
    vertices, faces, _ = ref.surface(np.zeros((2, 2, 2), dtype=bool))
    assert vertices.shape == (0, 3) and faces.shape == (0, 3)


def test_count_recipes_hit_their_counts():
    for (what, count), codes in ref.COUNT_RECIPES.items():
        mask = ref.count_volume(codes) != 0
        vertices, faces, _ = ref.surface(mask)
        assert dict(cells=ref.active_cells(mask), vertices=len(vertices), triangles=len(faces))[what] == count, (what, count)
        assert len(vertices) % 2 == 0 and len(faces) % 4 == 0


def test_lone_voxel():
    vertices, faces, roots = ref.surface(np.ones((1, 1, 1), dtype=bool))
    assert len(faces) == 24 and len(vertices) == 14
    assert ref.integer_table(vertices, faces, roots)["v6"].tolist() == [24]         # 48 x 1/2
    assert vertices.min() == -1 and vertices.max() == 1
    assert ref.euler_characteristic(len(vertices), faces) == 2


def test_euler_characteristic_of_a_ball_and_a_ring():
    vertices, faces, _ = ref.surface(ref.ball(64, 21))
    assert ref.is_closed_manifold(faces) and ref.euler_characteristic(len(vertices), faces) == 2
    ring = np.ones((3, 3, 1), dtype=bool)
    ring[1, 1, 0] = False
    vertices, faces, _ = ref.surface(ring)
    assert ref.is_closed_manifold(faces) and ref.euler_characteristic(len(vertices), faces) == 0


def test_pinned_ball():
    """x^2 + y^2 + z^2 <= 64 in 21^3 at unit spacing: the prototype's integers.  The quadrilateral of a two-two case is
    a parallelogram, so none of them depends on its split or on the orientation rule."""
    mask = ref.ball(64, 21)
    assert int(mask.sum()) == 2109
    vertices, faces, roots = ref.surface(mask)
    table = ref.integer_table(vertices, faces, roots)
    assert len(faces) == 7104 and table["triangles"].tolist() == [7104]
    # classes 1..7 = 4|nx| + 2|ny| + |nz|: (0,0,1) (0,1,0) (0,1,1) (1,0,0) (1,0,1) (1,1,0) (1,1,1)
    assert table["classes"][0].tolist() == [1724, 1724, 508, 1724, 508, 508, 408, 0]
    assert table["v6"].tolist() == [100752] and 100752 == 48 * 2099 == ref.closed_form_v48(mask)
    sphere = 4.0 * math.pi * 64.0
    raw = ref.raw_area_mm2(table["classes"][0], (1, 1, 1), 1.0)
    assert abs(raw / sphere - 1.249) < 5e-4
    face_faces = 6 * 2109 - 2 * sum(int((mask[tuple(slice(1, None) if a == b else slice(None) for b in range(3))] &
                                         mask[tuple(slice(None, -1) if a == b else slice(None) for b in range(3))]).sum())
                                    for a in range(3))
    assert abs(face_faces / sphere - 1.47) < 5e-3
    rows = ref.neighbours(faces, len(vertices))
    assert 3 <= min(map(len, rows)) and max(map(len, rows)) <= 12              # at most 6 tetrahedra x 2 triangles
    smooth = ref.smooth(ref.positions_mm(vertices, (1, 1, 1), 1.0), rows, 20)
    area, volume = ref.face_terms(smooth, faces)
    assert abs(math.fsum(area) / sphere - 1.039) < 5e-4
    assert abs(math.fsum(volume) / 2099.0 - 1.0) < 0.005
    raw_area, raw_volume = ref.face_terms(ref.positions_mm(vertices, (1, 1, 1), 1.0), faces)
    assert abs(math.fsum(raw_area) - raw) < 1e-9 * raw and abs(math.fsum(raw_volume) - 2099.0) < 1e-9


def test_lesions_are_closed_at_26_and_totals_hold_at_6():
    vol = measure_ref.random_volume((13, 17, 9), 0.2)
    for connectivity in (26, 6):
        mesh = ref.region_mesh(vol, "WT", (1, 1, 1), connectivity)
        assert ref.is_closed_manifold(mesh["faces"])
        assert int(mesh["v6"].sum()) == ref.closed_form_v48(vol != 0)
        want = measure_ref.lesion_table(vol, "WT", (1, 1, 1), connectivity)["root"]
        assert mesh["root"].tolist() == want.tolist()                       # gts.measure's lesions, in its order
        if connectivity == 26:
            for k in range(len(mesh["root"])):
                assert ref.is_closed_manifold(mesh["faces"][mesh["face_lesion"] == k]), k
    assert not all(ref.is_closed_manifold(mesh["faces"][mesh["face_lesion"] == k]) for k in range(len(mesh["root"])))


def _host_mesh(mask, units=(1, 1, 1), scale=1.0, iterations=2):
    vertices, faces, roots = ref.surface(mask, ref.lesion_roots(mask, 26))
    table = ref.integer_table(vertices, faces, roots)
    mm = ref.smooth(ref.positions_mm(vertices, units, scale), ref.neighbours(faces, len(vertices)), iterations)
    area, volume = ref.face_terms(mm, faces)
    return dict(vertices_half=vertices, vertices_mm=mm, faces=faces,
                face_lesion=np.searchsorted(table["root"], roots).astype(np.int32), face_area_mm2=area,
                face_volume_mm3=volume, units=units, scale_mm=scale, smooth_iterations=iterations, **table)


def test_ply_reads_back(tmp_path):
    from gts import mesh

    mask = np.zeros((4, 5, 6), dtype=bool)
    mask[1:3, 1:4, 2:5] = True
    mask[0, 0, 0] = True
    m = _host_mesh(mask, (2, 1, 3), 0.5)
    path = str(tmp_path / "a.ply")
    mesh.write_ply(path, m)
    comments, vertices, faces, lesion = read_ply(path)
    assert any("frame: millimetres" in c for c in comments) and any("2 Taubin" in c for c in comments)
    assert np.array_equal(vertices, m["vertices_mm"].astype(np.float32))
    assert np.array_equal(faces, m["faces"]) and np.array_equal(lesion, m["face_lesion"]) and set(lesion) == {0, 1}
    affine = np.array([[0, -1.0, 0, 10], [1.0, 0, 0, -20], [0, 0, 1.5, 5], [0, 0, 0, 1]])
    mesh.write_ply(path, m, affine)
    comments, world, faces, _ = read_ply(path)
    assert any("NIfTI world" in c for c in comments) and np.array_equal(faces, m["faces"])
    index = m["vertices_mm"] / (np.array([2, 1, 3]) * 0.5)
    assert np.array_equal(world, (index @ affine[:3, :3].T + affine[:3, 3]).astype(np.float32))
    with pytest.raises(mesh._lib.GtsError):
        mesh.write_ply(path, m, np.eye(3))
    empty = _host_mesh(np.zeros((2, 2, 2), dtype=bool))
    mesh.write_ply(path, empty)
    _, vertices, faces, lesion = read_ply(path)
    assert vertices.shape == (0, 3) and faces.shape == (0, 3) and lesion.shape == (0,)
    assert mesh.shape_features(empty) == []


def test_shape_features_of_a_ball():
    from gts import mesh

    m = _host_mesh(ref.ball(64, 21), iterations=20)
    (f,) = mesh.shape_features(m)
    assert tuple(f) == mesh.FEATURE_KEYS
    assert f["mesh_triangles"] == 7104 and f["mesh_volume_ml"] == 2099.0 / 1000.0
    assert f["mesh_area_mm2"] == ref.raw_area_mm2(m["classes"][0], (1, 1, 1), 1.0)
    area, volume = float(np.bincount(m["face_lesion"], m["face_area_mm2"])[0]), float(np.bincount(m["face_lesion"], m["face_volume_mm3"])[0])
    assert f["smooth_area_mm2"] == area and f["smooth_volume_ml"] == volume / 1000.0
    assert f["sphericity"] == (36.0 * math.pi * volume * volume) ** (1.0 / 3.0) / area and 0.95 < f["sphericity"] < 1.0
    assert f["surface_to_volume_per_mm"] == area / volume


def test_rows_and_header_are_unchanged_without_mesh():
    from gts import mesh
    from scripts import measure_tumours as cli

    assert cli.HEADER == ["id", "region", "lesion", "n_lesions", "root", "voxels", "volume_ml", "ml_label1", "ml_label2",
                          "ml_label3", "centroid_x_mm", "centroid_y_mm", "centroid_z_mm", "extent_x_mm", "extent_y_mm",
                          "extent_z_mm", "face_area_mm2", "diameter_mm", "plane_z", "plane_major_mm", "plane_minor_mm",
                          "plane_product_mm2"]
    assert tuple(cli.MESH_HEADER) == mesh.FEATURE_KEYS
    vol = measure_ref.embed(measure_ref.box_block(), (8, 8, 8), (1, 2, 3))
    report = measure_ref.tumour_report(vol)
    plain = cli.rows_of("a", report)
    assert all(len(row) == len(cli.HEADER) for row in plain) and len(plain) == 6
    assert plain[0][:7] == ["a", "WT", "1", "", "84", "30", "0.03"]
    features = {key: 0.5 for key in mesh.FEATURE_KEYS}
    with_features = {r: dict(rec, lesions=[dict(m, **features) for m in rec["lesions"]]) for r, rec in report.items()}
    assert cli.rows_of("a", with_features) == plain                      # the keys alone change nothing
    wide = cli.rows_of("a", with_features, mesh=True)
    assert [row[:len(cli.HEADER)] for row in wide] == plain
    assert wide[0][len(cli.HEADER):] == ["0.5"] * 7 and wide[1][len(cli.HEADER):] == [""] * 7
    args = cli.build_parser().parse_args(["-s", "x", "-o", "y"])
    assert (args.mesh, args.mesh_smooth, args.mesh_dir) == (False, 20, None)


def test_entry_points_refuse_bad_arguments_before_the_device(hip_lib):
    one, units = ctypes.c_void_p(16), (ctypes.c_int64 * 3)(1, 1, 1)
    bad_units = (ctypes.c_int64 * 3)(1, 0, 1)
    assert hip_lib.gts_mesh_workspace(0, 4, 4) == 0 and hip_lib.gts_mesh_workspace(4098, 4, 4) == 0
    assert hip_lib.gts_mesh_workspace(1290, 1290, 1290) == 0 and hip_lib.gts_mesh_workspace(4, 4, 4) > 0
    assert hip_lib.gts_mesh_table_i64s(4, 4, 4, 18) == 0 and hip_lib.gts_mesh_table_i64s(4, 4, 4, 26) == 8 + 12 * 8
    assert hip_lib.gts_mesh_table_i64s(4, 4, 4, 6) == 8 + 12 * 32
    big = 1 << 40
    assert hip_lib.gts_mesh_classify(None, 4, 4, 4, 26, one, big, one, big, 0, None) == -1
    assert hip_lib.gts_mesh_classify(one, 0, 4, 4, 26, one, big, one, big, 0, None) == -2
    assert hip_lib.gts_mesh_classify(one, 4, 4, 4, 26, one, big, one, 16, 0, None) == -2
    assert hip_lib.gts_mesh_classify(one, 4, 4, 4, 26, one, big, one, big, -1, None) == -2
    assert hip_lib.gts_mesh_classify(one, 4, 4, 4, 18, one, big, one, big, 0, None) == -3
    assert hip_lib.gts_mesh_classify(one, 4, 4, 4, 26, one, 8, one, big, 0, None) == -2
    assert hip_lib.gts_mesh_emit(one, 4, 4, 4, one, big, None, 5, one, one, 5, 0, None) == -1
    assert hip_lib.gts_mesh_emit(one, 4, 4, 4, one, big, one, 1 << 31, one, one, 5, 0, None) == -2
    assert hip_lib.gts_mesh_emit(one, 4, 4, 4, one, big, one, 5, one, one, 1 << 30, 0, None) == -2
    assert hip_lib.gts_mesh_emit(one, 4, 4, 4, one, big, None, 0, None, None, 0, 0, None) == 0      # an empty region
    assert hip_lib.gts_mesh_relabel(None, 5, one, 1, 0, None) == -1 and hip_lib.gts_mesh_relabel(None, 0, None, 0, 0, None) == 0
    assert hip_lib.gts_mesh_adjacency(one, 5, 5, None, one, one, big, 0, None) == -1
    assert hip_lib.gts_mesh_adjacency(one, 5, 5, one, one, one, 16, 0, None) == -2
    assert hip_lib.gts_mesh_adjacency_workspace(-1) == 0 and hip_lib.gts_mesh_adjacency_workspace(1 << 31) == 0
    assert hip_lib.gts_mesh_positions(one, 5, None, 1.0, one, 0, None) == -1
    assert hip_lib.gts_mesh_positions(one, 5, bad_units, 1.0, one, 0, None) == -3
    assert hip_lib.gts_mesh_positions(one, 5, units, float("nan"), one, 0, None) == -3
    assert hip_lib.gts_mesh_positions(one, 5, units, 0.0, one, 0, None) == -3
    assert hip_lib.gts_mesh_positions(None, 0, units, 1.0, None, 0, None) == 0
    assert hip_lib.gts_mesh_smooth(one, one, 5, 5, None, one, 0.5, -0.53, 1, 0, None) == -1
    assert hip_lib.gts_mesh_smooth(one, one, 5, 5, one, one, 0.5, -0.53, -1, 0, None) == -2
    assert hip_lib.gts_mesh_smooth(one, one, 5, 5, one, one, float("inf"), -0.53, 1, 0, None) == -3
    assert hip_lib.gts_mesh_smooth(one, None, 0, 0, None, None, 0.5, -0.53, 20, 0, None) == 0
    assert hip_lib.gts_mesh_terms(None, one, 5, 5, one, one, 0, None) == -1
    assert hip_lib.gts_mesh_terms(one, one, 5, 5, one, one, 1 << 31, None) == -2
    assert hip_lib.gts_mesh_terms(None, None, 0, 0, None, None, 0, None) == 0


def test_wrapper_refuses_bad_arguments_before_the_device():
    import torch

    from gts import _lib, mesh

    vol = torch.zeros((3, 3, 3), dtype=torch.int16)
    with pytest.raises(_lib.GtsError, match="MI355X only"):
        mesh.region_mesh(vol, "WT")
    for kwargs in (dict(region="XT"), dict(connectivity=18), dict(smooth_iterations=-1), dict(smooth_iterations=1.5),
                   dict(grid_blocks=-1)):
        args = dict(region="WT")
        args.update(kwargs)
        with pytest.raises(_lib.GtsError):
            mesh.region_mesh(vol, **args)
    with pytest.raises(_lib.GtsError):
        mesh.region_mesh(vol.float(), "WT")
