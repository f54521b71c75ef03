"""gts.texture's GLRLM, GLSZM, GLDM and NGTDM families without a GPU: the reference on the closed
forms, the identities on every shared case, `derive` against the exact reference, the degenerate cases, the argument
refusals of the wrappers, the CLI and the C entry points, the byte cap of a run table and the CSV layout."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import measure_ref
from tests import texture_matrices_ref as mref
from tests import texture_ref as ref

EPS = 2.0 ** -52
D = ref.DIRECTIONS


def _columns(row):
    """{column (from 0): count} of the entries of a table row that are not zero."""
    return {int(c): int(row[c]) for c in np.flatnonzero(row)}


# 1. the reference on the closed forms
def test_constant_box_by_hand():
    for name, (labels, image) in ref.box_cases().items():
        t = mref.lesion_matrices(labels, image, "WT")
        assert mref.identities_hold(t), name
        assert t["zones"].tolist() == [[0, 0, int((labels != 0).sum()), 1]] and t["ngtdm_s"].sum() == 0, name
        if not name.startswith("box"):
            continue
        runs = {d: _columns(t["glrlm"][0, D.index(d), 0]) for d in D}
        assert runs[(0, 0, 1)] == {4: 6} and runs[(0, 1, 0)] == {2: 10} and runs[(1, 0, 0)] == {1: 15}, name
        assert runs[(0, 1, 1)] == {0: 4, 1: 4, 2: 6} and runs[(1, 1, 1)] == {0: 14, 1: 8}, name
        assert _columns(t["gldm"][0, 0]) == {7: 8, 11: 16, 17: 6}, name      # k = 8, 12, 18
        assert _columns(t["ngtdm_n"][0, 0]) == {7: 8, 11: 16, 17: 6}, name
        assert t["glrlm"].shape == (1, 13, 1, 5) and t["gldm"].shape == (1, 1, 27), name


def test_checkerboard_by_hand():
    labels, image, _ = ref.checkerboard_case()
    t = mref.lesion_matrices(labels, image, "CT", bins=2)
    assert mref.identities_hold(t)
    assert t["zones"].tolist() == [[0, 0, 30, 1], [0, 1, 30, 1]]           # 6-connected zones would be 60 singletons
    assert t["glrlm"][0, D.index((0, 0, 1))].tolist() == [[30, 0, 0, 0], [30, 0, 0, 0]]
    assert t["glrlm"][0, D.index((1, 1, 0))].tolist() == [[3, 3, 3, 3], [3, 3, 3, 3]]
    for g in (0, 1):
        assert _columns(t["gldm"][0, g]) == {3: 4, 5: 12, 8: 11, 12: 3}      # k = 4, 6, 9, 13
        assert _columns(t["ngtdm_n"][0, g]) == {7: 4, 11: 12, 17: 11, 26: 3}
        assert _columns(t["ngtdm_s"][0, g]) == {7: 16, 11: 72, 17: 99, 26: 42}
    wide = mref.lesion_matrices(labels, image, "CT", bins=2, dependence_alpha=1)
    assert np.array_equal(wide["gldm"], wide["ngtdm_n"])    # every neighbour is dependent: column k - 1 is column m


def test_touching_lesions_share_nothing_by_hand():
    labels, image = ref.touching_case()
    six = mref.lesion_matrices(labels, image, "WT", 6, bins=1)            # one level everywhere: only the root separates
    whole = mref.lesion_matrices(labels, image, "WT", 26, bins=1)
    assert mref.identities_hold(six) and mref.identities_hold(whole)
    assert six["zones"].tolist() == [[k, 0, 12, 1] for k in range(3)] and whole["zones"].tolist() == [[0, 0, 36, 1]]
    assert six["ngtdm_n"][:, 0, [7, 11]].tolist() == [[8, 4]] * 3          # a 2 x 2 x 3 box alone: 7 at its ends, 11 between
    assert whole["ngtdm_n"][0, 0, 12:].sum() > 0
    d = D.index((1, 1, 0))
    assert six["glrlm"][:, d, 0, :2].tolist() == [[6, 3]] * 3 and whole["glrlm"][0, d, 0, 3] > 0


def test_line_and_serpentine_by_hand():
    t = mref.lesion_matrices(*mref.line_case(), "WT")
    assert t["glrlm"].shape == (1, 13, 1, 300) and t["zones"].tolist() == [[0, 0, 300, 1]]
    assert _columns(t["glrlm"][0, 0, 0]) == {299: 1} and all(_columns(m[0]) == {0: 300} for m in t["glrlm"][0, 1:])
    t = mref.lesion_matrices(*mref.serpentine_case(), "WT")
    assert mref.identities_hold(t) and t["zones"].tolist() == [[0, 0, 275, 1], [0, 31, 157, 1]]


# 2. the identities on every shared case, and what the reference costs
def test_identities_on_the_gpu_cases_and_their_cost():
    start = time.perf_counter()
    lesions = 0
    for index in range(len(ref.cached_selection())):
        for connectivity in (6, 26):
            for least in (1, 5):
                t = mref.cached_selection_matrices(index, connectivity, least)
                lesions += len(t["root"])
                assert mref.identities_hold(t), (index, connectivity, least)
                base = ref.cached_selection_table(index, connectivity, least)
                assert all(np.array_equal(t[key], base[key]) for key in ("root", "n", "levels", "hist", "glcm"))
    for labels, image, bins in ref.contention_cases().values():
        assert mref.identities_hold(mref.lesion_matrices(labels, image, "WT", bins=bins))
    for voxels in (2047, 2048, 2049, 4097):
        assert mref.identities_hold(mref.lesion_matrices(*ref.chunk_case(voxels, 2048), "WT"))
    assert lesions > 1000
    assert time.perf_counter() - start < 20.0, "every reference call of the GPU cases together"


# 3. derive against the exact reference
def _tables():
    labels, image = ref.touching_case()
    yield "touching-26", mref.lesion_matrices(labels, image, "WT", 26, bins=8)
    yield "touching-6-width", mref.lesion_matrices(labels, image, "WT", 6, bin_width=2.5, dependence_alpha=1)
    labels, image, (a, _, _) = ref.ramp_case()
    yield "ramp", mref.lesion_matrices(labels, image, "WT", bins=a)
    yield "box", mref.lesion_matrices(*ref.box_cases()["box-interior"], "WT")
    yield "checkerboard", mref.lesion_matrices(*ref.checkerboard_case()[:2], "CT", bins=2)
    yield "serpentine", mref.lesion_matrices(*mref.serpentine_case(), "WT")
    name, labels, image = ref.cached_selection()[1]
    yield name, mref.lesion_matrices(labels, image, "WT", 6, bins=16)                  # many lone voxels
    name, labels, image = ref.cached_selection()[2]
    yield name, mref.lesion_matrices(labels, image, "WT", 6, bin_width=100.0, min_lesion_voxels=3)
    name, labels, image = ref.cached_selection()[9]
    yield name, mref.lesion_matrices(labels, image, "WT", 26, bins=128, min_lesion_voxels=50)


def test_derive_equals_the_exact_reference():
    """The bound, by counting roundings: a rational feature is an exact Fraction rounded once by `derive` and once by
    this test's float(exact), 2 x 2^-53 = EPS of its value; an entropy is the math.fsum of the same rounded terms as
    the reference's, so it is equal, except the GLRLM's mean over 13 directions, 2 roundings in `derive` and 13 in
    the reference's running sum and division, 15 x 2^-53 < 8 EPS."""
    from gts import texture

    assert (texture.GLRLM_KEYS, texture.GLSZM_KEYS, texture.GLDM_KEYS, texture.NGTDM_KEYS) == \
        (mref.GLRLM_KEYS, mref.GLSZM_KEYS, mref.GLDM_KEYS, mref.NGTDM_KEYS)
    assert tuple(texture.MATRICES) == mref.MATRICES and len(texture.FEATURE_KEYS) == 37
    assert (len(mref.GLRLM_KEYS), len(mref.GLSZM_KEYS), len(mref.GLDM_KEYS)) == (16, 16, 16)
    worst, lone, lesions = {}, 0, 0
    for name, table in _tables():
        for k in range(len(table["root"])):
            got = texture.derive(table, k)
            lesions += 1
            want = dict(mref.glrlm_features(table, k), **mref.glszm_features(table, k), **mref.gldm_features(table, k))
            ngtdm = mref.ngtdm_features(table, k)
            if ngtdm is None:
                assert all(got[key] is None for key in mref.NGTDM_KEYS) and table["n"][k] == 1, name
                lone += 1
            else:
                want.update(ngtdm)
            assert set(got) == {"root", "n"} | set(texture.FEATURE_KEYS) | set(want) | set(mref.NGTDM_KEYS)
            for key, (exact, terms) in want.items():
                bound = (8.0 if key == "glrlm_run_entropy" else 1.0) * EPS
                err = abs(got[key] - float(exact))
                assert isinstance(got[key], float) and err <= bound * float(terms), (name, k, key, got[key], err)
                if float(terms):
                    worst[key] = max(worst.get(key, 0.0), err / float(terms) / EPS)
    print(lesions, {key: round(v, 3) for key, v in worst.items() if v})
    assert lone > 0 and lesions > 100


def test_degenerate_cases():
    from gts import texture

    speck = np.zeros((3, 3, 3), dtype=np.int16)
    speck[1, 1, 1] = 2
    lone = texture.derive(mref.lesion_matrices(speck, np.ones(speck.shape, np.float32), "WT"), 0)
    assert all(lone[key] is None for key in texture.NGTDM_KEYS)            # N_v = 0
    assert lone["glszm_zone_percentage"] == 1.0 == lone["glrlm_run_percentage"] == lone["gldm_low_dependence_emphasis"]
    box = texture.derive(mref.lesion_matrices(*ref.box_cases()["box-interior"], "WT"), 0)
    assert box["ngtdm_coarseness"] == 1e6                                  # sum p s = 0
    assert (box["ngtdm_contrast"], box["ngtdm_busyness"], box["ngtdm_strength"]) == (0.0, 0.0, 0.0)   # N_gp = 1
    assert box["ngtdm_complexity"] == 0.0 and box["glszm_zone_percentage"] == 1 / 30
    assert box["glszm_large_zone_emphasis"] == 900.0 and box["glrlm_run_entropy"] > 0.0
    # two levels of equal weight whose voxels all see the average of their neighbourhood: no difference at all
    n, s = np.zeros((2, 27), np.int64), np.zeros((2, 27), np.int64)
    n[0, 2] = n[1, 2] = 4
    flat = texture._ngtdm_features(n, s)
    assert flat["ngtdm_coarseness"] == 1e6 and flat["ngtdm_strength"] == 0.0 and flat["ngtdm_contrast"] == 0.0
    n[1, 2] = 2                                                            # 1 x 4/6 = 2 x 2/6: busyness' denominator is 0
    s[0, 2] = 3
    assert texture._ngtdm_features(n, s)["ngtdm_busyness"] == 0.0
    board = texture.derive(mref.lesion_matrices(*ref.checkerboard_case()[:2], "CT", bins=2), 0)
    assert board["ngtdm_busyness"] > 0.0 and board["ngtdm_contrast"] > 0.0 and board["ngtdm_strength"] > 0.0


def test_derive_without_the_new_tables_is_unchanged():
    from gts import texture

    table = mref.lesion_matrices(*ref.touching_case(), "WT", 26, bins=8)
    bare = {key: table[key] for key in ("root", "n", "lo", "hi", "levels", "hist", "glcm", "bins", "bin_width")}
    got = texture.derive(bare, 0)
    assert list(got) == ["root", "n"] + list(texture.FEATURE_KEYS) and len(got) == 37 + 2
    full = texture.derive(table, 0)
    assert all(full[key] == got[key] for key in got)
    only = texture.derive(dict(bare, zones=table["zones"]), 0)
    assert list(only) == list(got) + list(texture.GLSZM_KEYS)


# 4. refusals
def test_wrappers_refuse_with_their_own_messages(hip_lib):
    from gts import GtsError, measure, texture

    vol = torch.zeros((4, 5, 6), dtype=torch.int16)
    img = torch.zeros((4, 5, 6), dtype=torch.float32)
    for bad, match in ((dict(matrices=("glrlm", "glcm")), r"matrices \['glcm'\]"), (dict(matrices="zones"), "zones"),
                       (dict(matrices=("gldm",), dependence_alpha=-1), "dependence_alpha -1"),
                       (dict(matrices=("gldm",), dependence_alpha=1.0), "dependence_alpha 1.0"),
                       (dict(dependence_alpha=True), "dependence_alpha True")):
        with pytest.raises(GtsError, match=match):
            texture.lesion_texture(vol, img, "WT", **bad)
    with pytest.raises(GtsError, match="MI355X only"):
        texture.lesion_texture(vol, img, "WT", matrices=("glrlm",))        # the arguments pass: refused for the device
    with pytest.raises(GtsError, match="texture_matrices needs texture"):
        measure.tumour_report(vol, texture_matrices=("glrlm",))
    with pytest.raises(GtsError, match="matrices"):
        measure.tumour_report(vol, texture={"t1": img}, texture_matrices=("glxx",))
    with pytest.raises(GtsError, match="dependence_alpha"):
        measure.tumour_report(vol, texture={"t1": img}, texture_matrices=("gldm",), texture_dependence_alpha=-2)
    assert texture.matrices_arg(("ngtdm", "glrlm"), 3, "x") == (("glrlm", "ngtdm"), 3)
    assert texture.matrices_arg("gldm", 500, "x") == (("gldm",), 128) and texture.matrices_arg((), 0, "x") == ((), 0)
    empty = texture.empty_matrices(texture.MATRICES)
    assert {key: value.shape for key, value in empty.items()} == dict(
        glrlm=(0, 13, 1, 1), zones=(0, 4), gldm=(0, 1, 27), ngtdm_n=(0, 1, 27), ngtdm_s=(0, 1, 27))
    assert all(value.dtype == np.int64 for value in empty.values()) and texture.empty_matrices(()) == {}


def test_the_byte_cap_refuses_a_run_table(hip_lib):
    from gts import GtsError, _lib, texture

    cap = _lib.const("GTS_TEXTURE_MAX_TABLE_BYTES")
    per_lesion = 13 * 128 * 240
    most = cap // (4 * per_lesion)
    assert hip_lib.gts_texture_run_words(most, 128, 240) == most * per_lesion
    assert hip_lib.gts_texture_run_words(most + 1, 128, 240) == 0 < hip_lib.gts_texture_run_words(most + 1, 128, 239)
    assert hip_lib.gts_texture_run_words(1, 129, 1) == 0 == hip_lib.gts_texture_run_words(1, 0, 1)
    assert hip_lib.gts_texture_run_words(0, 1, 1) == 0 == hip_lib.gts_texture_run_words(1, 1, 0)
    assert hip_lib.gts_texture_run_words(1, 1, 4097) == 13 * 4097 and hip_lib.gts_texture_run_words(1, 1, 4098) == 0
    assert texture.run_table_words(most, 128, 240) == most * per_lesion
    with pytest.raises(GtsError, match="run-length tables of .* exceed 1073741824 bytes.*widen the bins"):
        texture.run_table_words(most + 1, 128, 240)
    assert hip_lib.gts_texture_neighbourhood_i64s(2, 32) == 3 * 2 * 32 * 27
    assert hip_lib.gts_texture_neighbourhood_i64s(2, 129) == 0 == hip_lib.gts_texture_neighbourhood_i64s(0, 32)
    assert hip_lib.gts_texture_neighbourhood_i64s(cap // (8 * 3 * 27 * 128) + 1, 128) == 0


P = ctypes.c_void_p(16)         # never dereferenced: every call below is refused before a launch


def _caller(fn, good):
    def call(**change):
        args = list(good)
        for at, value in change.items():
            args[int(at[1:])] = value
        return fn(*args)
    return call


def test_entry_points_refuse_in_order(hip_lib):
    lib = hip_lib
    from gts import _lib

    assert (_lib.const("GTS_TEXTURE_NEIGHBOURS"), _lib.const("GTS_TEXTURE_DEPENDENCES")) == (26, 27)
    assert (_lib.const("GTS_TEXTURE_MAX_RUN"), _lib.const("GTS_TEXTURE_ZONE_RECORD_I32")) == (4097, 3)
    ws = lib.gts_texture_workspace(8, 8, 8)
    # X4 lengths: roots, X, Y, Z, work, n_work, segments, plan, lesions, list, levels, n_listed, run_length,
    #             run_length_words, head, workspace, workspace_bytes, grid_blocks, stream
    lengths = _caller(lib.gts_texture_run_lengths, [P, 8, 8, 8, P, 26, P, P, 2, P, P, 100, P, 1300, P, P, ws, 0, None])
    for at in (0, 4, 6, 7, 9, 10, 12, 14, 15):
        assert lengths(**{f"a{at}": None, "a1": 0}) == -1                    # NULL before the shape
    assert lengths(a1=0, a17=-1) == -2 == lengths(a3=4098) == lengths(a5=0) == lengths(a5=1 << 31)
    assert lengths(a8=0) == -2 == lengths(a8=513) == lengths(a11=0) == lengths(a11=513)
    assert lengths(a17=-1) == -2 == lengths(a17=1 << 31) == lengths(a16=ws - 1) == lengths(a13=1299)
    # X4 counts: work, n_work, segments, plan, lesions, levels, run_length, n_listed, table, table_words, max_levels,
    #            longest, grid_blocks, stream
    words = lib.gts_texture_run_words(2, 32, 9)
    assert words == 2 * 13 * 32 * 9
    runs = _caller(lib.gts_texture_runs, [P, 26, P, P, 2, P, P, 100, P, words, 32, 9, 0, None])
    for at in (0, 2, 3, 5, 6, 8):
        assert runs(**{f"a{at}": None, "a4": 0}) == -1
    assert runs(a4=0, a12=-1) == -2 == runs(a1=0) == runs(a7=0) == runs(a10=0) == runs(a10=129)
    assert runs(a11=0) == -2 == runs(a11=4098) == runs(a12=-1) == runs(a9=words - 1)
    # X5: roots, X, Y, Z, segments, plan, lesions, list, levels, n_listed, scratch, scratch_words, records,
    #     records_words, head, workspace, workspace_bytes, grid_blocks, stream
    zones = _caller(lib.gts_texture_zones, [P, 8, 8, 8, P, P, 2, P, P, 100, P, 1024, P, 300, P, P, ws, 0, None])
    for at in (0, 4, 5, 7, 8, 10, 12, 14, 15):
        assert zones(**{f"a{at}": None, "a1": 0}) == -1
    assert zones(a1=0, a17=-1) == -2 == zones(a6=0) == zones(a9=0) == zones(a9=513)
    assert zones(a17=-1) == -2 == zones(a16=ws - 1) == zones(a11=1023) == zones(a13=299)
    # X6: roots, X, Y, Z, work, n_work, segments, plan, lesions, list, levels, n_listed, alpha, table, table_i64s,
    #     max_levels, workspace, workspace_bytes, grid_blocks, stream
    entries = lib.gts_texture_neighbourhood_i64s(2, 32)
    near = _caller(lib.gts_texture_neighbourhood,
                   [P, 8, 8, 8, P, 2, P, P, 2, P, P, 100, 0, P, entries, 32, P, ws, 0, None])
    for at in (0, 4, 6, 7, 9, 10, 13, 16):
        assert near(**{f"a{at}": None, "a1": 0}) == -1
    assert near(a1=0, a12=-1) == -2 == near(a5=0) == near(a8=0) == near(a11=513)     # the shape before alpha
    assert near(a12=-1, a18=-1) == -3                                       # alpha before the grid and the sizes
    assert near(a18=-1, a17=0) == -2 == near(a17=ws - 1) == near(a14=entries - 1) == near(a15=129) == near(a15=0)


# 5. the plan and the host ends of the device layout
def test_chunk_units_and_zone_counting():
    from gts import texture

    n = [1, texture.CHUNK - 1, texture.CHUNK, texture.CHUNK + 1, 2 * texture.CHUNK + 1]
    units = texture.chunk_units(n)
    assert units.dtype == np.int32 and units.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [4, 0], [4, 1], [4, 2]]
    assert texture.chunk_units([]).shape == (0, 2)
    records = np.int32([[1, 0, 5], [0, 3, 1], [1, 0, 5], [0, 3, 2], [0, 0, 7], [1, 0, 5]])
    want = [[0, 0, 7, 1], [0, 3, 1, 1], [0, 3, 2, 1], [1, 0, 5, 3]]
    assert texture.count_zones(records).tolist() == want == texture.count_zones(records[::-1].ravel()).tolist()
    assert texture.count_zones(records).dtype == np.int64 and texture.count_zones(np.zeros(0)).shape == (0, 4)


# 6. the CLI
def test_cli_arguments_header_and_rows(tmp_path):
    from gts import texture
    from scripts import measure_tumours as cli

    base = ["-s", "P", "-o", "R.csv"]
    args = cli.build_parser().parse_args(base)
    assert (args.texture_matrices, args.texture_dependence_alpha) == (None, None)
    args = cli.build_parser().parse_args(base + ["--texture", "S", "--texture_matrices", "ngtdm", "glrlm",
                                                 "--texture_dependence_alpha", "2"])
    assert (args.texture_matrices, args.texture_dependence_alpha) == (["ngtdm", "glrlm"], 2)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--texture", "S", "--texture_matrices", "glcm"])
    for flags in (["--texture_matrices", "all"], ["--texture_dependence_alpha", "1"]):
        with pytest.raises(SystemExit, match="need --texture"):
            cli.main(["-s", str(tmp_path), "-o", str(tmp_path / "R.csv")] + flags)
    assert tuple(cli.TEXTURE_MATRICES) == texture.MATRICES
    exts = ["_t1.nii.gz", "_t2.nii.gz"]
    plain = cli.texture_header(exts)
    assert len(plain) == 74 and cli.texture_header(exts, ()) == plain      # unchanged without the flag
    header = cli.texture_header(exts, ["ngtdm", "glszm"])
    assert header[:74] == plain and len(header) == 74 + 2 * (16 + 5) == len(set(header))
    assert header[74] == "tex_t1_glszm_small_zone_emphasis" and header[74 + 16] == "tex_t1_ngtdm_coarseness"
    assert header[74 + 21] == "tex_t2_glszm_small_zone_emphasis" and header[-1] == "tex_t2_ngtdm_strength"
    assert len(cli.texture_header(exts, cli.TEXTURE_MATRICES)) == 74 + 2 * (16 + 16 + 16 + 5)
    vol = measure_ref.embed(measure_ref.box_block(), (8, 7, 5), (1, 2, 1))
    vol[7, 6, 4] = 1
    report = measure_ref.tumour_report(vol, (1, 1, 1))
    image = np.arange(vol.size, dtype=np.int16).reshape(vol.shape)
    table = mref.lesion_matrices(vol, image, "WT")
    by_root = {int(table["root"][k]): texture.derive(table, k) for k in range(2)}
    for m in report["WT"]["lesions"]:
        m["texture"] = {"t1": by_root[m["root"]]}
    before = cli.rows_of("scan", report, ("WT",), False, ["t1"])
    rows = cli.rows_of("scan", report, ("WT",), False, ["t1"], ["glrlm", "ngtdm"])
    width = len(cli.HEADER) + 37
    assert [row[:width] for row in rows] == before and all(len(row) == width + 21 for row in rows)
    big, lone = rows[0][width:], rows[1][width:]
    assert float(big[0]) == by_root[47]["glrlm_short_runs_emphasis"] and "" not in big
    assert lone[16:] == [""] * 5 and "" not in lone[:16] and rows[2][width:] == [""] * 21
    cli.write_csv(str(tmp_path / "r.csv"), rows, False, ["_t1.nii.gz"], ["glrlm", "ngtdm"])
    lines = (tmp_path / "r.csv").read_text().splitlines()
    assert lines[0] == ",".join(cli.HEADER + cli.texture_header(["_t1.nii.gz"], ["glrlm", "ngtdm"])) and len(lines) == 4
