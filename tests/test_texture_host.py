"""gts.texture without a GPU: the reference on cases computed by hand, `derive` against the exact reference, the
entry points' refusals and their order, the byte cap, the work-unit plan, the CLI's arguments and row layout, and
the reference's cost on the GPU cases."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

from tests import measure_ref
from tests import texture_ref as ref

EPS = 2.0 ** -52


# 1. the reference on cases computed by hand
def test_constant_box_by_hand():
    a, b, c = ref.BOX
    for name, (labels, image) in ref.box_cases().items():
        t = ref.lesion_texture(labels, image, "WT")
        assert t["levels"].tolist() == [1] and t["lo"].tolist() == t["hi"].tolist(), name
        assert t["hist"].tolist() == [[int((labels != 0).sum())]], name
        if name.startswith("box"):
            want = [2 * (a - abs(dx)) * (b - abs(dy)) * (c - abs(dz)) for dx, dy, dz in ref.DIRECTIONS]
            assert t["glcm"][0, :, 0, 0].tolist() == want, name
    unit = ref.lesion_texture(*ref.box_cases()["unit-axis"], "ET")
    assert unit["glcm"][0, :, 0, 0].tolist() == [2 * (3 - abs(dx)) * (3 - abs(dy)) * (1 - abs(dz))
                                                 for dx, dy, dz in ref.DIRECTIONS]
    assert len(ref.DIRECTIONS) == 13 and ref.DIRECTIONS[0] == (0, 0, 1) and ref.DIRECTIONS[-1] == (1, 1, 1)


def test_ramp_and_checkerboard_by_hand():
    labels, image, (a, b, c) = ref.ramp_case()
    t = ref.lesion_texture(labels, image, "WT", bins=a)
    assert t["levels"].tolist() == [a] and t["hist"].tolist() == [[b * c] * a]      # hi lands in a - 1, not a
    for d, (dx, dy, dz) in enumerate(ref.DIRECTIONS):
        m = t["glcm"][0, d]
        per_step = (b - abs(dy)) * (c - abs(dz))
        if dx:
            assert np.array_equal(m, per_step * (np.eye(a, k=1, dtype=np.int64) + np.eye(a, k=-1, dtype=np.int64)))
        else:
            assert np.array_equal(m, 2 * per_step * np.eye(a, dtype=np.int64))
    labels, image, (a, b, c) = ref.checkerboard_case()
    t = ref.lesion_texture(labels, image, "CT", bins=2)
    for d, delta in enumerate(ref.DIRECTIONS):
        pairs = (a - abs(delta[0])) * (b - abs(delta[1])) * (c - abs(delta[2]))
        m = t["glcm"][0, d]
        if sum(abs(s) for s in delta) % 2:                   # an odd step changes the colour: purely off-diagonal
            assert m[0, 0] == m[1, 1] == 0 and m[0, 1] == m[1, 0] == pairs
        else:
            assert m[0, 1] == m[1, 0] == 0 and m[0, 0] + m[1, 1] == 2 * pairs


def test_same_root_not_same_mask_by_hand():
    labels, image = ref.touching_case()
    six = ref.lesion_texture(labels, image, "WT", 6)
    assert six["n"].tolist() == [12, 12, 12] and six["levels"].tolist() == [32, 32, 32]
    whole = ref.lesion_texture(labels, image, "WT", 26)
    assert whole["n"].tolist() == [36]
    alone = [ref.lesion_texture(np.where(np.isin(image, values), labels, 0), image, "WT", 6)
             for values in ((10, 12), (20, 27), (35, 31))]
    for k, t in enumerate(alone):                            # no pair crosses the edge or the corner
        assert np.array_equal(six["glcm"][k], t["glcm"][0])
    assert whole["glcm"].sum() > six["glcm"].sum()           # one lesion: the pairs across appear


def test_level_edges_by_hand():
    values = np.array([-2.5, -2.0, -0.5, 0.0, 0.5, 1.99, 2.0], dtype=np.float32)
    g, n_levels = ref.grey_levels(values, values.min(), values.max(), bin_width=0.5)
    assert g.tolist() == [0, 1, 4, 5, 6, 8, 9] and n_levels == 10          # floor, not truncation
    g, n_levels = ref.grey_levels(values, values.min(), values.max(), bins=3)
    assert g.tolist() == [0, 0, 1, 1, 2, 2, 2] and n_levels == 3            # -2.5 + 4.5 / 3 k: 0.5 lies on a boundary
    g, n_levels = ref.grey_levels(np.int16([5, 5]), 5, 5, bins=32)
    assert g.tolist() == [0, 0] and n_levels == 1
    assert ref.grey_levels(np.int16([0, 127]), 0, 127, bin_width=1.0)[1] == 128
    line = np.full((1, 1, 130), 1, dtype=np.int16)
    with pytest.raises(ref.Refused):
        ref.lesion_texture(line, np.arange(130, dtype=np.int16).reshape(1, 1, 130), "WT", bin_width=1.0)


# 2. derive against the exact reference
def _tables():
    labels, image = ref.touching_case()
    yield "touching-26", ref.lesion_texture(labels, image, "WT", 26, bins=8)
    yield "touching-6-width", ref.lesion_texture(labels, image, "WT", 6, bin_width=2.5)
    labels, image, (a, _, _) = ref.ramp_case()
    yield "ramp", ref.lesion_texture(labels, image, "WT", bins=a)
    yield "box", ref.lesion_texture(*ref.box_cases()["box-interior"], "WT")
    name, labels, image = ref.cached_selection()[1]
    yield name, ref.lesion_texture(labels, image, "WT", 6, bins=16, min_lesion_voxels=1)     # many lone voxels
    name, labels, image = ref.cached_selection()[2]
    yield name, ref.lesion_texture(labels, image, "WT", 6, bin_width=100.0, min_lesion_voxels=3)


def test_derive_equals_the_exact_reference():
    from gts import texture

    assert texture.HIST_KEYS == ref.HIST_KEYS and texture.GLCM_KEYS == ref.GLCM_KEYS
    assert list(texture.DIRECTIONS) == ref.DIRECTIONS
    worst, lone = {}, 0
    for name, table in _tables():
        for k in range(len(table["root"])):
            got = texture.derive(table, k)
            assert got["root"] == table["root"][k] and got["n"] == table["n"][k]
            want = dict(ref.histogram_features(table, k))
            pairs = ref.glcm_features(table, k)
            if pairs is None:
                assert all(got[key] is None for key in ref.GLCM_KEYS), name
                lone += 1
            else:
                want.update(pairs)
            bound = (int(table["levels"][k]) ** 2 + 8) * EPS
            for key, (exact, terms) in want.items():
                err = abs(float(got[key]) - float(exact)) if not isinstance(exact, float) else abs(got[key] - exact)
                if isinstance(exact, (int, np.integer)) or key in ("min", "max"):
                    assert got[key] == exact, (name, k, key)
                assert err <= bound * float(terms), (name, k, key, got[key], float(exact), err)
                if float(terms):
                    worst[key] = max(worst.get(key, 0.0), err / float(terms) / EPS)
    print({key: round(v, 2) for key, v in worst.items()})
    assert lone > 0 and max(worst.values()) <= 8.0            # a handful of roundings, far inside (G^2 + 8)


def test_degenerate_features():
    from gts import texture

    box = ref.lesion_texture(*ref.box_cases()["box-interior"], "WT")
    got = texture.derive(box, 0)
    assert (got["levels"], got["variance"], got["skewness"], got["kurtosis"], got["entropy"]) == (1, 0.0, 0.0, 0.0, 0.0)
    assert (got["correlation"], got["information_correlation_1"], got["information_correlation_2"]) == (1.0, 0.0, 0.0)
    assert got["joint_maximum"] == 1.0 == got["angular_second_moment"] and got["mean_intensity_approx"] == 7.0
    speck = np.zeros((3, 3, 3), dtype=np.int16)
    speck[1, 1, 1] = 2
    lone = texture.derive(ref.lesion_texture(speck, np.ones(speck.shape, np.float32), "WT"), 0)
    assert all(lone[key] is None for key in texture.GLCM_KEYS) and lone["median_level"] == 1


# 3. the reference stays cheap on every case of the GPU tests
def test_reference_cost_of_the_gpu_cases():
    start = time.perf_counter()
    lesions = 0
    for index in range(len(ref.cached_selection())):
        for connectivity in (6, 26):
            for least in (1, 5):
                lesions += len(ref.cached_selection_table(index, connectivity, least)["root"])
    for labels, image, bins in ref.contention_cases().values():
        ref.lesion_texture(labels, image, "WT", bins=bins)
    for voxels in (2047, 2048, 2049, 4097):
        labels, image = ref.chunk_case(voxels, 2048)
        assert ref.lesion_texture(labels, image, "WT")["n"].tolist() == [voxels]
    assert lesions > 1000
    assert time.perf_counter() - start < 5.0, "every reference call of the GPU cases together"


# 4. argument checks, nothing launched
P = ctypes.c_void_p(16)         # never dereferenced: every call below is refused before a launch


def test_entry_points_refuse_in_order(hip_lib):
    lib = hip_lib
    from gts import _lib

    assert (_lib.const("GTS_TEXTURE_MAX_LEVELS"), _lib.const("GTS_TEXTURE_DIRECTIONS")) == (128, 13)
    assert _lib.const("GTS_TEXTURE_CHUNK") % 256 == 0
    ws, ints = lib.gts_texture_workspace(8, 8, 8), lib.gts_texture_count_i64s(8, 8, 8, 26)
    assert ws > 0 and ints == 8 + 2 * 64 and lib.gts_texture_count_i64s(8, 8, 8, 6) == 8 + 2 * 256
    assert lib.gts_texture_workspace(0, 8, 8) == 0 == lib.gts_texture_workspace(4098, 1, 1)
    assert lib.gts_texture_workspace(4097, 4097, 127) > 0 and lib.gts_texture_workspace(4097, 4097, 128) == 0
    assert lib.gts_texture_count_i64s(8, 8, 8, 18) == 0 == lib.gts_texture_count_i64s(8, 0, 8, 26)
    words = lib.gts_texture_table_words(2, 32)
    assert words == 2 * (32 + 13 * 528)
    # X1 counts: roots, X, Y, Z, connectivity, counts, counts_i64s, workspace, workspace_bytes, grid_blocks, stream
    x0 = lib.gts_texture_counts
    assert x0(None, 0, 8, 8, 18, P, 0, P, 0, -1, None) == -1 == x0(P, 8, 8, 8, 26, None, ints, P, ws, 0, None)
    assert x0(P, 8, 8, 8, 26, P, ints, None, ws, 0, None) == -1
    assert x0(P, 0, 8, 8, 18, P, 0, P, 0, -1, None) == -2                   # the shape before the kinds
    assert x0(P, 8, 8, 8, 18, P, 0, P, 0, -1, None) == -3                   # the kinds before the grid and the sizes
    assert x0(P, 8, 8, 8, 26, P, ints, P, ws, -1, None) == -2 == x0(P, 8, 8, 8, 26, P, ints, P, ws, 1 << 31, None)
    assert x0(P, 8, 8, 8, 26, P, ints, P, ws - 1, 0, None) == -2 == x0(P, 8, 8, 8, 26, P, ints - 1, P, ws, 0, None)
    assert x0(P, 8, 8, 8, 6, P, ints, P, ws, 0, None) == -2                 # a table sized for 26 is too short for 6
    # X1 ranges: roots, image, dtype, X, Y, Z, select, n_rows, segments, lesions, ranges, ranges_i64s, list, n_listed,
    #            workspace, workspace_bytes, grid_blocks, stream
    good = [P, P, 4, 8, 8, 8, P, 3, P, 2, P, 8 + 4 * 2, P, 100, P, ws, 0, None]

    def ranges(**change):
        args = list(good)
        for at, value in change.items():
            args[int(at[1:])] = value
        return lib.gts_texture_ranges(*args)
    for at in (0, 1, 6, 8, 10, 12, 14):
        assert ranges(**{f"a{at}": None, "a2": 8, "a3": 0}) == -1
    assert ranges(a2=8, a3=0) == -2 == ranges(a2=8, a5=4098)                 # the shape before the dtype
    assert ranges(a7=0) == -2 == ranges(a9=4) == ranges(a9=0) == ranges(a13=0) == ranges(a13=513)
    assert ranges(a2=8, a16=-1, a15=0) == -3                                # the dtype before the grid and the sizes
    assert ranges(a16=-1, a15=0) == -2 == ranges(a15=ws - 1) == ranges(a11=8 + 4 * 2 - 1)
    assert ranges(a2=16, a16=1 << 31) == -2
    # X2: image, dtype, X, Y, Z, bins, bin_width, segments, plan, lesions, list, n_listed, levels, table, table_words,
    #     max_levels, workspace, workspace_bytes, grid_blocks, stream
    good2 = [P, 16, 8, 8, 8, 32, 0.0, P, P, 2, P, 100, P, P, words, 32, P, ws, 0, None]

    def levels(**change):
        args = list(good2)
        for at, value in change.items():
            args[int(at[1:])] = value
        return lib.gts_texture_levels(*args)
    for at in (0, 7, 8, 10, 12, 13, 16):
        assert levels(**{f"a{at}": None, "a1": 8, "a2": 0}) == -1
    assert levels(a1=8, a2=0) == -2 == levels(a9=0) == levels(a11=0) == levels(a11=513)
    assert levels(a1=8, a5=0) == -3                                          # the dtype, then the bins
    for bins, width in ((0, 0.0), (129, 0.0), (-1, 0.0), (32, -1.0), (32, math.nan), (32, math.inf)):
        assert levels(a5=bins, a6=width, a18=-1) == -3                       # the bins before the grid
    assert levels(a5=0, a6=0.5, a18=-1) == -2                                # a width: the bin number is not looked at
    assert levels(a18=-1, a17=0) == -2 == levels(a17=ws - 1) == levels(a14=words - 1)
    assert levels(a15=0) == -2 == levels(a15=129)
    # X3: roots, X, Y, Z, work, n_work, segments, plan, lesions, list, levels, n_listed, table, table_words,
    #     max_levels, workspace, workspace_bytes, grid_blocks, stream
    good3 = [P, 8, 8, 8, P, 26, P, P, 2, P, P, 100, P, words, 32, P, ws, 0, None]

    def glcm(**change):
        args = list(good3)
        for at, value in change.items():
            args[int(at[1:])] = value
        return lib.gts_texture_glcm(*args)
    for at in (0, 4, 6, 7, 9, 10, 12, 15):
        assert glcm(**{f"a{at}": None, "a1": 0}) == -1
    assert glcm(a1=0, a17=-1) == -2 == glcm(a5=-1) == glcm(a5=1 << 31) == glcm(a8=0) == glcm(a11=0)
    assert glcm(a17=-1) == -2 == glcm(a16=ws - 1) == glcm(a13=words - 1) == glcm(a14=129)
    assert glcm(a4=None, a5=0) == 0                                          # no unit: nothing to launch


def test_the_byte_cap_refuses_instead_of_allocating(hip_lib):
    from gts import GtsError, _lib, texture

    cap = _lib.const("GTS_TEXTURE_MAX_TABLE_BYTES")
    per_lesion = 128 + 13 * 8256
    most = cap // (4 * per_lesion)
    assert hip_lib.gts_texture_table_words(most, 128) == most * per_lesion
    assert hip_lib.gts_texture_table_words(most + 1, 128) == 0
    assert hip_lib.gts_texture_table_words(most + 1, 127) > 0              # the cap scales with lesions x 13 x levels^2
    assert hip_lib.gts_texture_table_words(1, 0) == 0 == hip_lib.gts_texture_table_words(1, 129)
    assert hip_lib.gts_texture_table_words(-1, 32) == 0 and hip_lib.gts_texture_table_words(0, 32) == 0
    assert texture.table_words(most, 128) == most * per_lesion
    with pytest.raises(GtsError, match="exceed 1073741824 bytes.*widen the bins"):
        texture.table_words(most + 1, 128)


def test_wrappers_refuse_with_their_own_messages(hip_lib):
    from gts import GtsError, measure, texture

    vol = torch.zeros((4, 5, 6), dtype=torch.int16)
    img = torch.zeros((4, 5, 6), dtype=torch.float32)
    for bad, match in ((dict(bins=0), "bins 0"), (dict(bins=129), "bins 129"), (dict(bins=2.0), "bins 2.0"),
                       (dict(bin_width=0), "bin_width 0"), (dict(bin_width=-1.0), "bin_width -1.0"),
                       (dict(bin_width=math.inf), "bin_width inf"), (dict(min_lesion_voxels=0), "min_lesion_voxels 0"),
                       (dict(grid_blocks=-1), "grid_blocks"), (dict(connectivity=18), "connectivity 18")):
        with pytest.raises(GtsError, match=match):
            texture.lesion_texture(vol, img, "WT", **bad)
    with pytest.raises(GtsError, match="region 'TC'"):
        texture.lesion_texture(vol, img, "TC")
    with pytest.raises(GtsError, match="MI355X only"):
        texture.texture_features(vol, img, "WT")
    with pytest.raises(GtsError, match="bins 0"):
        measure.tumour_report(vol, texture={"t1": img}, texture_bins=0)
    assert texture.binning_args(32, None, "x") == (32, 0.0) and texture.binning_args(32, 2, "x") == (0, 2.0)
    lo, hi = np.float64([0.0, -0.25, 3.0]), np.float64([127.0, 63.75, 3.0])
    assert texture.level_counts(lo, hi, 0, 1.0).tolist() == [128, 65, 1]
    assert texture.level_counts(lo, hi, 0, 0.5).tolist() == [255, 129, 1]
    assert texture.level_counts(lo, hi, 32, 0.0).tolist() == [32, 32, 1]


# 5. the plan and the host ends of the device layout
def test_work_units_cover_every_lesion_direction_and_chunk_once():
    from gts import texture

    n = [1, texture.CHUNK - 1, texture.CHUNK, texture.CHUNK + 1, 2 * texture.CHUNK + 1]
    units = texture.work_units(n)
    assert units.dtype == np.int32 and units.shape == (13 * (1 + 1 + 1 + 2 + 3), 3)
    want = {(k, d, c) for k, count in enumerate(n) for d in range(13) for c in range(-(-count // texture.CHUNK))}
    assert {tuple(u) for u in units.tolist()} == want and len(want) == len(units)
    assert texture.work_units([]).shape == (0, 3)


def test_range_words_and_folded_triangles_decode():
    from gts import texture

    values = np.float32([-np.inf, -3.5, -1e-30, 0.0, 1e-30, 2.0, 7.25e8, np.inf])
    bits = values.view(np.uint32).astype(np.int64)
    words = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    assert np.all(np.diff(words) > 0)                                        # the encoding keeps the order
    assert np.array_equal(texture.decode_range(words, torch.float32), values)
    assert texture.decode_range(np.int64([0, 32768, 65535]), torch.int16).tolist() == [-32768, 0, 32767]
    G = 5
    rng = np.random.default_rng(0)
    folded = rng.integers(0, 9, (2, 13, G * (G + 1) // 2))
    dense = texture.unfold(folded, G)
    assert np.array_equal(dense, dense.transpose(0, 1, 3, 2))
    for i in range(G):
        for j in range(i, G):
            assert np.array_equal(dense[..., i, j], folded[..., j * (j + 1) // 2 + i] * (2 if i == j else 1))


# 6. the CLI
def test_cli_arguments_header_and_rows(tmp_path):
    from gts import texture
    from scripts import measure_tumours as cli

    base = ["-s", "P", "-o", "R.csv"]
    args = cli.build_parser().parse_args(base)
    assert (args.texture, args.texture_bins, args.texture_bin_width) == (None, None, None)
    assert args.texture_modalities == ["_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"]
    args = cli.build_parser().parse_args(base + ["--texture", "S", "--texture_modalities", "_t1ce.nii.gz", "_x.nii",
                                                 "--texture_bin_width", "25"])
    assert (args.texture, args.texture_modalities, args.texture_bin_width) == ("S", ["_t1ce.nii.gz", "_x.nii"], 25.0)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--texture", "S", "--texture_bins", "8", "--texture_bin_width", "2"])
    with pytest.raises(SystemExit):
        cli.main(["-s", str(tmp_path), "-o", str(tmp_path / "R.csv"), "--texture_bins", "8"])
    assert tuple(cli.TEXTURE_FEATURES) == texture.FEATURE_KEYS and len(cli.TEXTURE_FEATURES) == 37
    assert [cli.modality_name(e) for e in ("_flair.nii.gz", "_x.nii", "t2.nii.gz")] == ["flair", "x", "t2"]
    header = cli.texture_header(["_t1.nii.gz", "_t2.nii.gz"])
    assert header[0] == "tex_t1_min" and header[37] == "tex_t2_min" and len(header) == 74 == len(set(header))
    vol = measure_ref.embed(measure_ref.box_block(), (8, 7, 5), (1, 2, 1))
    vol[7, 6, 4] = 1
    report = measure_ref.tumour_report(vol, (1, 1, 1))
    plain = cli.rows_of("scan", report, ("WT",))
    image = np.arange(vol.size, dtype=np.int16).reshape(vol.shape)
    table = ref.lesion_texture(vol, image, "WT")
    by_root = {int(table["root"][k]): texture.derive(table, k) for k in range(2)}
    for m in report["WT"]["lesions"]:
        m["texture"] = {"t1": by_root[m["root"]]}
    rows = cli.rows_of("scan", report, ("WT",), False, ["t1"])
    assert [row[:len(cli.HEADER)] for row in rows] == plain
    assert all(len(row) == len(cli.HEADER) + 37 for row in rows) and rows[2][len(cli.HEADER):] == [""] * 37
    big, lone = rows[0][len(cli.HEADER):], rows[1][len(cli.HEADER):]
    assert float(big[4]) == by_root[47]["mean_level"] and big[3] == "32" and lone[3] == "1"
    assert lone[15:] == [""] * 22 and "" not in big                          # a lone voxel has no GLCM features
    cli.write_csv(str(tmp_path / "r.csv"), rows, False, ["_t1.nii.gz"])
    lines = (tmp_path / "r.csv").read_text().splitlines()
    assert lines[0] == ",".join(cli.HEADER + cli.texture_header(["_t1.nii.gz"])) and len(lines) == 4
