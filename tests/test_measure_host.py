"""The host side of the per-lesion measurements (gts/measure.py): the numpy reference of the
definition (tests/measure_ref.py) on closed forms worked out by hand, the hull-vertex pruning the kernels rely on,
the argument checks of the entry points and wrappers (nothing is launched), the host's work-unit plan and the rules
of scripts/measure_tumours.py.  No GPU."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import measure_ref as ref


def _only(table):
    assert len(table["n"]) == 1
    return {k: v[0].tolist() for k, v in table.items()}


# 1. closed forms
def test_box_by_hand():
    vol = ref.embed(ref.box_block(), (8, 7, 5), (1, 2, 1))        # [1:6, 2:5, 1:3]
    got = _only(ref.lesion_table(vol, "WT"))
    assert (got["n"], got["faces"], got["d3"]) == (30, [12, 20, 30], 21)        # 21 = 4^2 + 2^2 + 1^2
    assert (got["plane_z"], got["plane_d2"], got["plane_w"]) == (1, 20, 16)
    assert got["box"] == [1, 6, 2, 5, 1, 3] and got["n_class"] == [0, 0, 30]
    assert got["coord_sum"] == [30 * 3, 30 * 3, 15 * 1 + 15 * 2]
    assert got["root"] == 1 + (1 * 7 + 2) * 5 + 1
    for a, b in ((2, 2), (3, 7), (6, 4), (9, 2)):                  # an a x b rectangle: W = 2 (a - 1)(b - 1)
        pts = np.argwhere(np.ones((a, b), dtype=bool)).astype(np.int64)
        assert ref.plane_measure(pts)[:2] == ((a - 1) ** 2 + (b - 1) ** 2, 2 * (a - 1) * (b - 1))


def test_digital_ellipsoid_by_hand():
    block = ref.ellipsoid_block()
    got = _only(ref.lesion_table(ref.embed(block, block.shape, (0, 0, 0)), "WT"))
    assert (got["n"], got["faces"], got["d3"]) == (464, [112, 112, 224], 131)
    assert (got["plane_z"], got["plane_d2"], got["plane_w"]) == (2, 130, 130)
    for z in (2, 3):                                               # its widest slices
        assert ref.plane_measure(np.argwhere(block[:, :, z]).astype(np.int64)) == (130, 130, 8)


def test_tie_rule_takes_the_widest_pair():
    pts = np.argwhere(ref.tie_block()[:, :, 0]).astype(np.int64)
    assert ref.plane_measure(pts) == (5, 4, 2)
    widths = []
    for a, b in (((0, 1), (2, 2)), ((1, 0), (2, 2))):              # the two pairs at squared distance 5
        d = np.array(b) - np.array(a)
        proj = pts[:, 0] * -d[1] + pts[:, 1] * d[0]
        widths.append(int(proj.max() - proj.min()))
    assert sorted(widths) == [3, 4]
    for flipped in (pts * [-1, 1] + [2, 0], pts * [1, -1] + [0, 2], pts[:, ::-1]):      # mirrored, transposed
        assert ref.plane_measure(np.ascontiguousarray(flipped)) == (5, 4, 2)
    got = _only(ref.lesion_table(ref.embed(ref.tie_block(), (3, 3, 1), (0, 0, 0)), "ET"))
    assert (got["n"], got["d3"], got["plane_z"], got["plane_d2"], got["plane_w"]) == (5, 5, 0, 5, 4)


def test_spacing_scales_the_integers():
    from gts import metrics

    spacing = (0.9375, 0.9375, 5)
    assert [round(s * 10000) for s in spacing] == [9375, 9375, 50000]
    units, scale = metrics.spacing_units(spacing)
    assert (units, scale) == ((15, 15, 80), 0.0625) == ref.spacing_units(spacing)
    vol = ref.embed(ref.box_block(), (8, 7, 5), (1, 2, 1))
    got = _only(ref.lesion_table(vol, "WT", units))
    assert got["d3"] == 15 * 15 * (16 + 4) + 80 * 80 * 1
    assert (got["plane_d2"], got["plane_w"]) == (15 * 15 * 20, 15 * 15 * 16)
    m = ref.derive(ref.lesion_table(vol, "WT", units), 0, units, scale)
    assert m["volume_mm3"] == 30 * 0.9375 * 0.9375 * 5 and m["volume_ml"] == m["volume_mm3"] / 1000.0
    assert m["extent_mm"] == [5 * 0.9375, 3 * 0.9375, 10.0]
    assert m["centroid_voxel"] == [3.0, 3.0, 1.5] and m["centroid_mm"] == [3 * 0.9375, 3 * 0.9375, 7.5]
    assert m["face_area_mm2"] == 12 * 0.9375 * 5 + 20 * 0.9375 * 5 + 30 * 0.9375 * 0.9375
    assert m["diameter_mm"] == np.sqrt(got["d3"]) * 0.0625
    assert m["plane_major_mm"] == np.sqrt(15 * 15 * 20) * 0.0625 and m["plane_product_mm2"] == 16 * 0.9375 * 0.9375
    assert abs(m["plane_major_mm"] - np.sqrt(20.0) * 0.9375) < 1e-12       # sqrt rounds once either way
    assert abs(m["plane_major_mm"] * m["plane_minor_mm"] - m["plane_product_mm2"]) < 1e-12


def test_derive_equals_the_reference():
    from gts import measure

    vol = ref.random_volume((13, 17, 9), 0.2)
    for spacing in ref.SPACINGS:
        units, scale = ref.spacing_units(spacing)
        table = ref.lesion_table(vol, "WT", units)
        mine = dict(table, units=units, scale_mm=scale)
        for k in range(len(table["n"])):
            assert measure.derive(mine, k) == ref.derive(table, k, units, scale)
        want = ref.tumour_report(vol, spacing, min_lesion_voxels=3)["WT"]
        assert measure.report_from_table(mine, 3) == want
        assert all(m["n"] >= 3 for m in want["lesions"]) and want["n_lesions"] == len(table["n"]) > len(want["lesions"])


# 2. the pruning
def test_hull_vertex_pruning_is_exact():
    rng = np.random.default_rng(7)
    slices = 0
    for trial in range(24):
        shape = tuple(int(v) for v in rng.integers(1, 9, 3))
        units = np.array([(1, 1, 1), (15, 15, 80), (2, 1, 5)][trial % 3], dtype=np.int64)
        pts = np.argwhere(rng.random(shape) < (0.3, 0.6, 0.9)[trial % 3]).astype(np.int64)
        if len(pts) == 0:
            continue
        kept = ref.candidates(pts, 3)
        assert 1 <= len(kept) <= len(pts)
        assert ref.diameter2(kept * units) == ref.diameter2(pts * units)
        for z in np.unique(pts[:, 2]):
            foot = pts[pts[:, 2] == z][:, :2]
            assert ref.plane_measure(ref.candidates(foot, 2) * units[:2])[:2] == ref.plane_measure(foot * units[:2])[:2]
            slices += 1
    assert slices > 80
    from scipy import ndimage

    ball = ((np.indices((40, 40, 40)) - 19.5) ** 2).sum(axis=0) <= 18 * 18       # radius 18 about a voxel corner
    assert int((ball & ~ndimage.binary_erosion(ball)).sum()) == 3264
    assert len(ref.candidates(np.argwhere(ball).astype(np.int64), 3)) == 960


# 3. the reference stays cheap on every volume of the GPU tests
def test_reference_cost_of_the_gpu_cases():
    from scipy import ndimage

    largest, where = 0, None
    for name, vol in ref.cached_volumes().items():
        for region in ref.REGIONS:
            lab, count = ndimage.label(ref.region_mask(vol, region), structure=np.ones((3, 3, 3)))
            top = int(np.bincount(lab.ravel())[1:].max()) if count else 0
            if top > largest:
                largest, where = top, (name, region)
    assert 2000 < largest <= ref.MAX_LESION_VOXELS        # 16^3 at p = 0.7 percolates into one lesion
    start = time.perf_counter()
    ref.lesion_table(ref.cached_volumes()[where[0]], where[1], (15, 15, 80), 26)
    assert time.perf_counter() - start < 5.0, "the dearest reference call of the GPU cases"
    for planar in (False, True):
        for count, extent in ref.tile_boxes(256, planar).items():
            vol = ref.checkerboard_box(extent, 2 if planar else 3)
            table = ref.lesion_table(vol, "WT")
            assert table["n"].tolist() == [count]
            pts = np.argwhere(vol != 0).astype(np.int64)
            assert len(ref.candidates(pts if not planar else pts[:, :2], 2 if planar else 3)) == count
    lattice = ref.lesion_table(ref.lattice_volume(), "WT")
    assert len(lattice["n"]) == 1000 and not lattice["d3"].any() and not lattice["plane_w"].any()
    faces = ref.lesion_table(ref.face_touching_volume(), "WT")
    assert faces["box"][faces["n"].argmax()].tolist() == [0, 9, 0, 8, 0, 7]


# 4. argument checks, nothing launched
P = ctypes.c_void_p(16)         # never dereferenced: every call below is refused before a launch


def _units(*u):
    return (ctypes.c_int64 * 3)(*u)


def test_entry_points_refuse_in_order(hip_lib):
    lib = hip_lib
    from gts import _lib

    assert _lib.const("GTS_MEASURE_PAIR_TILE") == 256 == _lib.const("GTS_MEASURE_PLANE_TILE")
    ws = lib.gts_measure_workspace(8, 8, 8)
    ints = lib.gts_measure_table_i64s(8, 8, 8, 26)
    assert ws > 0 and ints == 8 + 24 * 64 and lib.gts_measure_table_i64s(8, 8, 8, 6) == 8 + 24 * 256
    assert lib.gts_measure_workspace(0, 8, 8) == 0 == lib.gts_measure_workspace(4098, 1, 1)
    assert lib.gts_measure_workspace(4097, 4097, 127) > 0 and lib.gts_measure_workspace(4097, 4097, 128) == 0
    assert lib.gts_measure_table_i64s(8, 8, 8, 18) == 0
    one = _units(1, 1, 1)
    # M1: labels, roots, X, Y, Z, region, connectivity, table, table_i64s, workspace, workspace_bytes, grid_blocks, stream
    m1 = lib.gts_measure_tables_i16
    assert m1(None, P, 8, 8, 8, 9, 9, P, 0, P, 0, -1, None) == -1
    assert m1(P, None, 8, 8, 8, 0, 26, P, ints, P, ws, 0, None) == -1
    assert m1(P, P, 8, 8, 8, 0, 26, None, ints, P, ws, 0, None) == -1
    assert m1(P, P, 8, 8, 8, 0, 26, P, ints, None, ws, 0, None) == -1
    assert m1(P, P, 0, 8, 8, 9, 9, P, ints, P, ws, 0, None) == -2          # shape before kinds
    assert m1(P, P, 4098, 1, 1, 0, 26, P, 1 << 40, P, 1 << 40, 0, None) == -2
    assert m1(P, P, 8, 8, 8, 9, 26, P, ints, P, ws, -1, None) == -2
    assert m1(P, P, 8, 8, 8, 9, 26, P, ints, P, ws - 1, 0, None) == -2
    assert m1(P, P, 8, 8, 8, 3, 26, P, ints, P, ws, 0, None) == -3
    assert m1(P, P, 8, 8, 8, -1, 26, P, ints, P, ws, 0, None) == -3
    assert m1(P, P, 8, 8, 8, 0, 18, P, ints, P, ws, 0, None) == -3
    assert m1(P, P, 8, 8, 8, 0, 26, P, ints - 1, P, ws, 0, None) == -2
    assert m1(P, P, 8, 8, 8, 0, 6, P, ints, P, ws, 0, None) == -2           # a table sized for 26 is too short for 6
    # M2: roots, X, Y, Z, table, table_i64s, workspace, workspace_bytes, grid_blocks, stream
    m2 = lib.gts_measure_candidates
    assert m2(None, 8, 8, 8, P, ints, P, ws, 0, None) == -1 == m2(P, 8, 8, 8, None, ints, P, ws, 0, None)
    assert m2(P, 8, 8, 8, P, ints, None, ws, 0, None) == -1
    for bad in ((8, 8, -1, ints, ws, 0), (8, 8, 8, ints - 1, ws, 0), (8, 8, 8, ints, ws - 1, 0),
                (8, 8, 8, ints, ws, 1 << 31)):
        x, y, z, t, w, g = bad
        assert m2(P, x, y, z, P, t, P, w, g, None) == -2
    # M3: X, Y, Z, units, work, n_work, table, table_i64s, workspace, workspace_bytes, grid_blocks, stream
    m3 = lib.gts_measure_diameters
    assert m3(8, 8, 8, None, P, 1, P, ints, P, ws, 0, None) == -1 == m3(8, 8, 8, one, None, 1, P, ints, P, ws, 0, None)
    assert m3(8, 8, 8, one, P, 1, None, ints, P, ws, 0, None) == -1 == m3(8, 8, 8, one, P, 1, P, ints, None, ws, 0, None)
    assert m3(8, 8, 0, _units(0, 1, 1), P, 1, P, ints, P, ws, 0, None) == -2
    assert m3(8, 8, 8, _units(0, 1, 1), P, -1, P, ints, P, ws, 0, None) == -2
    assert m3(8, 8, 8, _units(0, 1, 1), P, 1, P, ints, P, ws, 0, None) == -3
    assert m3(8, 8, 8, _units(1, 1, 1000001), P, 1, P, ints, P, ws, 0, None) == -3
    assert m3(8, 8, 8, one, None, 0, P, ints, P, ws, 0, None) == 0             # no unit: nothing to launch
    # M4: X, Y, Z, units, work, n_work, slices, n_slices, table, table_i64s, workspace, workspace_bytes, grid_blocks, stream
    m4 = lib.gts_measure_planes
    assert m4(8, 8, 8, None, P, 1, P, 1, P, ints, P, ws, 0, None) == -1
    assert m4(8, 8, 8, one, None, 1, P, 1, P, ints, P, ws, 0, None) == -1
    assert m4(8, 8, 8, one, P, 1, None, 1, P, ints, P, ws, 0, None) == -1
    assert m4(8, 8, 8, one, P, 1, P, 1, None, ints, P, ws, 0, None) == -1
    assert m4(8, 8, 8, one, P, 1, P, 513, P, ints, P, ws, 0, None) == -2        # more slice rows than voxels
    assert m4(8, 8, 8, _units(1, -1, 1), P, 1, P, 1, P, ints, P, ws, -1, None) == -2
    assert m4(8, 8, 8, _units(1, -1, 1), P, 1, P, 1, P, ints, P, ws, 0, None) == -3
    assert m4(8, 8, 8, one, None, 0, None, 0, P, ints, P, ws, 0, None) == 0


def test_the_overflow_bound_is_a_shape_refusal(hip_lib):
    lib = hip_lib
    # B = u^2 (N - 1)^2 along x alone: 2 B < 2^62 iff u (N - 1) < 2^30.5 = 1 518 500 249.99
    assert lib.gts_measure_check(4097, 1, 1, _units(370727, 1, 1)) == 0           # 4096 u = 1 518 497 792
    assert lib.gts_measure_check(4097, 1, 1, _units(370728, 1, 1)) == -2          # 4096 u = 1 518 501 888
    assert lib.gts_measure_check(4097, 1, 1, _units(1000000, 1, 1)) == -2
    assert lib.gts_measure_check(1, 1, 1, _units(1000000, 1000000, 1000000)) == 0
    assert lib.gts_measure_check(240, 240, 155, _units(100000, 100000, 100000)) == 0        # BraTS at 10 mm
    assert lib.gts_measure_check(8, 8, 8, _units(0, 1, 1)) == -3 and lib.gts_measure_check(8, 8, 8, None) == -1
    assert lib.gts_measure_check(0, 8, 8, _units(0, 1, 1)) == -2
    ws, ints = lib.gts_measure_workspace(4097, 1, 1), lib.gts_measure_table_i64s(4097, 1, 1, 26)
    big = _units(1000000, 1, 1)
    assert lib.gts_measure_diameters(4097, 1, 1, big, P, 1, P, ints, P, ws, 0, None) == -2
    assert lib.gts_measure_planes(4097, 1, 1, big, P, 1, P, 1, P, ints, P, ws, 0, None) == -2


def test_wrappers_refuse_with_their_own_messages(hip_lib):
    from gts import GtsError, measure

    vol = torch.zeros((4, 5, 6), dtype=torch.int16)
    for call in (lambda v, **kw: measure.lesion_table(v, kw.pop("region", "WT"), **kw),
                 lambda v, **kw: measure.lesion_measurements(v, kw.pop("region", "WT"), **kw),
                 lambda v, **kw: measure.tumour_report(v, **kw)):
        with pytest.raises(GtsError, match="MI355X only"):
            call(vol)
        with pytest.raises(GtsError, match="takes int16 labels"):
            call(vol.to(torch.int32))
        with pytest.raises(GtsError, match="three axes"):
            call(vol[0])
        with pytest.raises(GtsError, match="connectivity 18"):
            call(vol, connectivity=18)
        with pytest.raises(GtsError, match="spacing"):
            call(vol, spacing_mm=(1, 0, 1))
        with pytest.raises(GtsError, match="spacing"):
            call(vol, spacing_mm=(1, 1))
    with pytest.raises(GtsError, match="region 'TC'"):
        measure.lesion_table(vol, "TC")
    with pytest.raises(GtsError, match="region 3"):
        measure.lesion_measurements(vol, 3)
    with pytest.raises(GtsError, match="grid_blocks"):
        measure.lesion_table(vol, "WT", grid_blocks=-1)
    with pytest.raises(GtsError, match="takes a torch tensor"):
        measure.lesion_table(vol.numpy(), "WT")


# 5. the plan of the pairwise work
def test_work_units_cover_every_tile_pair_and_slice_once():
    from gts import measure

    rows = np.zeros((5, measure.ROW_I64), dtype=np.int64)
    rows[:, 17] = [1, 2, 256, 257, 700]                      # candidates: 0, 1, 1, 2 and 3 tiles
    pairs, planes = measure._work_units(rows, np.array([1, 3, 1, 2, 4]))
    assert pairs.dtype == np.int32 == planes.dtype
    want = {(1, 0, 0), (2, 0, 0)} | {(3, i, j) for i in range(2) for j in range(i, 2)} | \
        {(4, i, j) for i in range(3) for j in range(i, 3)}
    assert len(pairs) == len(want) and {tuple(p) for p in pairs.tolist()} == want
    assert planes.tolist() == [[0, 0], [1, 0], [1, 1], [1, 2], [2, 0], [3, 0], [3, 1], [4, 0], [4, 1], [4, 2], [4, 3]]
    none, one = measure._work_units(rows[:1], np.array([1]))
    assert none.shape == (0, 3) and one.tolist() == [[0, 0]]


# 6. the CLI
def test_cli_arguments_and_header(tmp_path):
    from scripts import measure_tumours as cli

    args = cli.build_parser().parse_args(["-s", "P", "-o", "R.csv"])
    assert (args.json, args.connectivity, args.min_lesion_voxels, args.regions) == (None, 26, 1, ["WT", "CT", "ET"])
    args = cli.build_parser().parse_args(["-s", "P", "-o", "R.csv", "--json", "R.json", "--connectivity", "6",
                                          "--min_lesion_voxels", "10", "--regions", "ET", "WT"])
    assert (args.json, args.connectivity, args.min_lesion_voxels, args.regions) == ("R.json", 6, 10, ["ET", "WT"])
    for bad in (["--connectivity", "18"], ["--regions", "TC"], []):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args((["-s", "P", "-o", "R.csv"] if bad else ["-s", "P"]) + bad)
    assert cli.HEADER[:7] == ["id", "region", "lesion", "n_lesions", "root", "voxels", "volume_ml"]
    assert len(cli.HEADER) == 22 == len(set(cli.HEADER))
    vol = ref.embed(ref.box_block(), (8, 7, 5), (1, 2, 1))
    vol[7, 6, 4] = 1
    report = ref.tumour_report(vol, (0.9375, 0.9375, 5))
    rows = cli.rows_of("scan", report, ("WT", "ET"))
    assert all(len(row) == len(cli.HEADER) for row in rows)
    assert [row[:6] for row in rows] == [["scan", "WT", "1", "", "47", "30"], ["scan", "WT", "2", "", "280", "1"],
                                        ["scan", "WT", "total", "2", "", "31"], ["scan", "ET", "1", "", "47", "30"],
                                        ["scan", "ET", "total", "1", "", "30"]]
    assert float(rows[0][6]) == report["WT"]["lesions"][0]["volume_ml"] and rows[2][10:] == [""] * 12
    assert [float(v) for v in rows[2][7:10]] == report["WT"]["class_ml"]
    cli.write_csv(str(tmp_path / "out" / "r.csv"), rows)
    lines = (tmp_path / "out" / "r.csv").read_text().splitlines()
    assert lines[0] == ",".join(cli.HEADER) and len(lines) == 6 and lines[3].split(",")[2] == "total"
    (tmp_path / "a.nii.gz").write_bytes(b"")
    (tmp_path / "b.nii").write_bytes(b"")
    assert list(cli.find_predictions(str(tmp_path))) == ["a"]
