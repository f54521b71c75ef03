"""The C-ABI library builds for gfx950, loads without a GPU and exports every symbol that
include/gts_hip.h declares (no compute calls here)."""
import ctypes
import os
import subprocess

from gts import _lib, build


def test_library_builds_and_exports_declared_symbols(hip_lib):
    declared = _lib.declared_symbols()
    assert len(declared) >= 105
    table = _lib.signatures()
    assert all(name in table for name in declared), "a declared symbol has no derived signature"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in gts_hip.h but not exported"
    assert hip_lib.gts_abi_version() == _lib.ABI_VERSION


_P, _I32, _I64, _U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
_F32, _F64 = ctypes.c_float, ctypes.c_double
# one entry point of every kind of declaration, as the hand-written table held them before the header was parsed
PINNED = {
    "gts_abi_version": (_I32, []),                                                       # (void)
    "gts_error_string": (ctypes.c_char_p, [_I32]),                                       # const char* return
    "gts_gat_reduce_workspace": (_I64, [_I64, _I64]),                                    # int64_t return
    "gts_gat_fwd_f32": (_I32, [_P, _P, _P, _P, _P, _F32, _P, _P, _I32, _P, _P, _I64, _I64, _I64, _P]),     # float by value
    "gts_augment_features_f32": (_I32, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _F64, _U64, _U64, _P]),  # double, uint64_t
    "gts_spmm_max_fwd_cluster_f32": (_I32, [_P, _I64, _I32, _I32, _I32, _P, _P, _P, _I32, _I32, _I64, _I64, _P, _P]),  # uint32_t*
    "gts_pack_weights_f32": (_I32, [_P, _P, _P, _I32, _I64, _I64, _I32, _P]),            # const float* const*
    "gts_collate_plan": (_I32, [_P, _I32, _I64, _P, _I32, _P]),                          # struct pointers
}


def test_signatures_are_derived_from_the_header():
    table = _lib.signatures()
    assert table is _lib.signatures(), "the header is parsed once per process"
    for name, want in PINNED.items():
        assert table[name] == want, name
    for name, (restype, argtypes) in table.items():
        assert restype in (_I32, _I64, ctypes.c_char_p), name
        assert all(a in (_P, _I32, _I64, ctypes.c_uint32, _U64, _F32, _F64) for a in argtypes), name


def test_header_parser_refuses_what_it_cannot_bind():
    import pytest

    sigs, consts = _lib.parse_header("""
        /* int32_t gts_in_a_block_comment(int32_t a);  prose (with parentheses) */
        // int32_t gts_in_a_line_comment(int32_t a);
        #define GTS_THREE 3
        #define GTS_MINUS (-7)   /* why */
        #define GTS_NOT_A_NUMBER "x"
        typedef struct { int64_t n; void* p; } gts_pair_t;
        int32_t gts_one(const gts_pair_t* pair, uint32_t* words, const float* const* tables, double x, void* stream);
        int64_t gts_none(void);
        const char* gts_name(int32_t code);
        void gts_quiet(float a,
                       uint64_t b);
    """)
    assert sigs == {"gts_one": (_I32, [_P, _P, _P, _F64, _P]), "gts_none": (_I64, []),
                    "gts_name": (ctypes.c_char_p, [_I32]), "gts_quiet": (None, [_F32, _U64])}
    assert consts == {"GTS_THREE": 3, "GTS_MINUS": -7}
    for bad in ("int32_t gts_bad(int16_t small);",                 # a scalar outside the six
                "int32_t gts_bad(unsigned int n);",
                "int32_t gts_bad(gts_pair_t by_value);",           # a struct by value
                "gts_pair_t gts_bad(int32_t n);",
                "int32_t gts_bad(const char* fmt, ...);",          # variadic
                "int32_t gts_bad(int32_t box[6]);",
                "int32_t gts_bad(int32_t (*callback)(int32_t));",  # cannot be split
                "int32_t gts_bad(int32_t n) { return n; }"):
        with pytest.raises(_lib.GtsError, match="gts_bad"):
            _lib.parse_header(bad)


def test_constants_are_read_from_the_header():
    import pytest

    from gts import dense, graphgen, ops

    assert (ops.DICE_MAX_GROUPS, ops.DICE_STATS_FLOATS) == (8, 40)
    assert (ops._DICE_LOSS, ops._DICE_CE, ops._DICE_LDICE, ops._DICE_DICE) == (0, 1, 2, 8)
    assert _lib.COLLATE_MAX_SCHEDULES == 6
    assert (graphgen.MAX_SV, graphgen.MAX_K, graphgen.MAX_RADIUS) == (32767, 32, 16)
    assert _lib.const("GTS_CLUSTER_COUNTER_WORDS") == 256 and ops._COUNTER_BYTES == 4 * 256
    assert _lib.const("GTS_OPT_GEMM_TILE") == 1 and dense._OPT_GEMM_TILE == 1
    assert _lib.const("GTS_ERR_SHAPE") == -2
    assert _lib.const("GTS_DICE_CE_STATS_FLOATS") == 40
    with pytest.raises(_lib.GtsError, match="GTS_NO_SUCH"):
        _lib.const("GTS_NO_SUCH")


def test_crop_concat_and_crop_concat_rows_refuse_the_same_operands():
    """K16 and J1 share their operand checks: the same GtsError for the same bad operand, on the host, before any launch."""
    import numpy as np
    import pytest
    import torch

    from gts import ops

    shape = (3, 2, 4)
    box = ops.CropBox([0, 2], [1], [0, 1, 3], shape, "cpu")
    good = dict(img=torch.zeros(shape + (2,)), svs=torch.zeros(shape, dtype=torch.int16), table=torch.zeros(5, 4),
                bg_row=torch.zeros(4))
    bad = {"partitioning dtype": dict(svs=torch.zeros(shape, dtype=torch.int32)),
           "image over another volume": dict(img=torch.zeros((3, 2, 5, 2))),
           "background row width": dict(bg_row=torch.zeros(3)),
           "1-D table": dict(table=torch.zeros(20)),
           "3-D table": dict(table=torch.zeros(5, 2, 2))}
    for what, change in bad.items():
        texts = []
        for fn in (ops.crop_concat, ops.crop_concat_rows):
            a = dict(good, **change)
            with pytest.raises(ops._lib.GtsError) as err:
                fn(a["img"], a["svs"], a["table"], a["bg_row"], box)
            texts.append(str(err.value).replace(fn.__name__, "<fn>"))
        assert texts[0] == texts[1], what
        assert "MI355X only" not in texts[0], f"{what}: refused for its shape or dtype, not for lying on the CPU"
    assert np.prod(box.shape) == 6


def test_library_is_gfx950_code(hip_lib):
    out = subprocess.run(["strings", "-n", "6", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_argument_errors_do_not_need_a_gpu(hip_lib):
    """Argument validation happens before any launch: checkable on the CPU box."""
    assert hip_lib.gts_spmm_max_fwd_f32(None, None, None, None, None, 0, 0, 4, 4, None) == -1
    one = ctypes.c_void_p(16)
    assert hip_lib.gts_spmm_max_fwd_f32(one, one, one, one, one, 3, 0, 4, 4, None) == -3
    assert hip_lib.gts_spmm_sum_f32(one, one, one, one, None, None, None, 0, -1, 4, None) == -2
    assert hip_lib.gts_project_rows_i16(one, one, one, one, 10, 10, 5, None) == -3
    assert hip_lib.gts_gat_fwd_f32(one, one, one, one, one, 0.2, None, None, 0, one, one, 4, 0, 4, None) == -2
    assert hip_lib.gts_gat_fwd_f32(one, one, one, one, one, 0.2, None, None, 7, one, one, 4, 4, 4, None) == -3
    assert b"NULL" in hip_lib.gts_error_string(-1)
    # tuning knobs take the kernel forms the library carries and nothing else (the rejected ones are built from tools/diag/)
    assert hip_lib.gts_set_option(2, 7) == -3 and hip_lib.gts_set_option(1, 9) == -3 and hip_lib.gts_set_option(9, 1) == -3
    assert hip_lib.gts_set_option(2, 6) == 0 and hip_lib.gts_set_option(2, -1) == 0
    # zero-sized problems are accepted without touching memory or the device
    assert hip_lib.gts_spmm_max_fwd_f32(one, one, one, one, None, 0, 1, 0, 4, None) == 0


def _scan_refusals():
    """(label, entry point, arguments, expected code) of calls that the scan-volume entry points (conform,
    co-registration, bias correction, brain extraction) refuse before they touch memory or the device.  Per entry
    point: arguments that pass every check (the pointers are never followed), where its dtype code, its extents,
    its grid_blocks and its float64 scalars stand, and the code each kind of refusal gives (recorded from the
    library as it was when each entry point still spelt its own guards, not from csrc/gts_scan.h's)."""
    one, nan, big = ctypes.c_void_p(16), float("nan"), 1 << 40
    eye = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    nans = (ctypes.c_double * 12)(*[nan] * 12)
    rows = [one, 5, 6, 7, one, one, one, 2, 1]            # u, X, Y, Z, weights, cells, lattice, spans0, levels
    # name: (arguments, dtype at, extents at, every extent below 65536 on its own, grid_blocks at, {NaN at: value},
    #        codes for dtype 8, extent 0, extent 65536, grid_blocks -1, NaN)
    entries = {
        "gts_conform_gather": ([one, 4, 1, 5, 6, 7, 0, 1, 2, 5, 6, 7, one, one, one, 1, one, None],
                               1, (3, 4, 5, 9, 10, 11), True, None, {}, (-3, -2, -2, None, None)),
        "gts_affine_resample": ([one, 4, 5, 6, 7, eye, 5, 6, 7, one, 0, None],
                                1, (2, 3, 4, 6, 7, 8), True, None, {5: nans}, (-3, -2, -2, None, -3)),
        "gts_joint_histogram": ([one, 5, 6, 7, one, 4, 5, 6, 7, eye, 1, 1, 16, 0.0, 1.0, 0.0, 1.0, one, 0, None],
                                5, (1, 2, 3, 6, 7, 8), True, 18, {9: nans, 13: nan, 14: nan, 15: nan, 16: nan},
                                (-3, -2, -2, -2, -3)),
        "gts_bias_workspace": ([5, 6, 7, 2], None, (0, 1, 2), True, None, {}, (None, -2, -2, None, None)),
        "gts_bias_log": ([one, 4, 5, 6, 7, 0.0, one, one, None], 1, (2, 3, 4), True, None, {5: nan},
                         (-3, -2, -2, None, -3)),
        "gts_bias_range": (rows + [one, one, big, 0, None], None, (1, 2, 3), True, 12, {}, (None, -2, -2, -2, None)),
        "gts_bias_histogram": (rows + [0.0, 1.0, one, 0, None], None, (1, 2, 3), True, 12, {9: nan, 10: nan},
                               (None, -2, -2, -2, -3)),
        "gts_bias_fit": (rows + [0, one, 0.0, 1.0, one, one, one, big, 0, None], None, (1, 2, 3), True, 17,
                         {11: nan, 12: nan}, (None, -2, -2, -2, -3)),
        "gts_bias_mean": (rows + [one, one, big, 0, None], None, (1, 2, 3), True, 12, {}, (None, -2, -2, -2, None)),
        "gts_bias_apply": ([one, 4] + rows[1:] + [0.0, one, None, 0, None], 1, (2, 3, 4), True, 13, {10: nan},
                           (-3, -2, -2, -2, -3)),
        "gts_brain_range": ([one, 4, 5, 6, 7, one, 0, None], 1, (2, 3, 4), False, 6, {}, (-3, -2, -2, -2, None)),
        "gts_brain_histogram": ([one, 4, 5, 6, 7, 1.0, one, 0, None], 1, (2, 3, 4), False, 7, {5: nan},
                                (-3, -2, -2, -2, -3)),
        "gts_brain_threshold": ([one, 4, 5, 6, 7, 1.0, one, one, 0, None], 1, (2, 3, 4), False, 8, {5: nan},
                                (-3, -2, -2, -2, -3)),
        "gts_ball_morph_i16": ([one, 5, 6, 7, 4, 1, 0, one, one, big, 0, 0, None], None, (1, 2, 3), False, 11, {},
                               (None, -2, -2, -2, None)),
        "gts_largest_component_i16": ([one, 5, 6, 7, 6, one, one, one, big, 0, None], None, (1, 2, 3), False, 9, {},
                                      (None, -2, -2, -2, None)),
        "gts_fill_holes_i16": ([one, 5, 6, 7, one, one, one, big, 0, None], None, (1, 2, 3), False, 8, {},
                               (None, -2, -2, -2, None)),
        "gts_apply_mask": ([one, 4, 2, 5, 6, 7, one, one, one, 0, None], 1, (3, 4, 5), False, 9, {},
                           (-3, -2, -2, -2, None)),
    }

    def changed(args, changes):
        return [changes.get(at, value) for at, value in enumerate(args)]

    for name, (good, dtype_at, extents_at, each, grid_at, nan_at, codes) in entries.items():
        if dtype_at is not None:
            yield f"{name} dtype 8", name, changed(good, {dtype_at: 8}), codes[0]
        for at in extents_at:
            yield f"{name} extent 0 at {at}", name, changed(good, {at: 0}), codes[1]
            if each:
                yield f"{name} extent 65536 at {at}", name, changed(good, {at: 65536}), codes[2]
        if not each:   # brain extraction has no limit per extent: 65536 along every axis is past its 2^31 voxels
            yield f"{name} every extent 65536", name, changed(good, {at: 65536 for at in extents_at}), codes[2]
        if grid_at is not None:
            yield f"{name} grid_blocks -1", name, changed(good, {grid_at: -1}), codes[3]
        for at, value in nan_at.items():
            yield f"{name} NaN at {at}", name, changed(good, {at: value}), codes[4]


def test_scan_entry_points_refuse_bad_arguments_with_their_own_codes(hip_lib):
    """A bad dtype code, extent, grid_blocks or NaN scalar gives its own code, and of two bad arguments the one an
    entry point checks first answers: the order of its checks is part of an entry point's contract, and the guards
    that csrc/gts_scan.h shares must not change it."""
    cases = list(_scan_refusals())
    assert len(cases) == 142
    for label, name, args, want in cases:
        assert want in (-2, -3), label
        assert getattr(hip_lib, name)(*args) == want, label
    # two things wrong at once: the check that comes first in an entry point still answers
    one, top = ctypes.c_void_p(16), 65535

    def conform(c, x, axes):
        return hip_lib.gts_conform_gather(one, 4, c, x, x, x, *axes, 5, 6, 7, one, one, one, 1, one, None)
    assert conform(1, top, (0, 0, 2)) == -3             # the axes are looked at before the number of voxels
    assert conform(1, 0, (0, 0, 2)) == -2               # and after the extents
    assert conform(1, top, (0, 1, 2)) == -2
    assert conform(0, top, (0, 1, 2)) == 0              # no channel: nothing to index, nothing launched
    assert conform(-1, 5, (0, 1, 2)) == -2
    assert hip_lib.gts_brain_range(None, 8, 5, 6, 7, one, 0, None) == -1                     # NULL, then the dtype
    assert hip_lib.gts_brain_range(one, 8, 0, 6, 7, one, 0, None) == -3                      # the dtype, then the shape
    assert hip_lib.gts_bias_apply(one, 8, 0, 6, 7, one, one, one, 2, 1, 0.0, one, None, 0, None) == -3
    assert hip_lib.gts_intake_occupancy(one, 8, 0, 6, 7, one, one, one, one, None) == -2     # the shape, then the dtype
    assert hip_lib.gts_intake_occupancy(one, 8, 5, 6, 7, one, one, one, one, None) == -3
    assert hip_lib.gts_dataset_stats_mask(one, 8, one, 5, 6, 7, one, one, 0, None) == -2     # the workspace's size first
    assert hip_lib.gts_dataset_stats_mask(one, 8, one, 5, 6, 7, one, one, 1 << 40, None) == -3


def test_cluster_schedule_rejects_a_malformed_csr(hip_lib):
    """gts_cluster_schedule is a HOST entry point of the C ABI: ids outside [0, n), extents that go down or that do not
    match the transpose must come back as GTS_ERR_SHAPE, not index the builder's tables."""
    import numpy as np

    def run(indptr, indices, t_indptr, t_indices):
        arrs = [np.asarray(a, dtype=np.int32) for a in (indptr, indices, t_indptr, t_indices)]
        out = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        return hip_lib.gts_cluster_schedule(*[a.ctypes.data_as(ctypes.c_void_p) for a in arrs], None, 3, 8, 16, 64, None, 0,
                                            ctypes.byref(out[0]), ctypes.byref(out[1]), ctypes.byref(out[2]))
    good = ([0, 1, 2, 3], [1, 2, 0], [0, 1, 2, 3], [2, 0, 1])
    assert run(*good) == 0
    assert run([0, 1, 2, 3], [1, 7, 0], good[2], good[3]) == -2            # neighbour id past the last row
    assert run([0, 1, 2, 3], [1, -1, 0], good[2], good[3]) == -2
    assert run(good[0], good[1], [0, 1, 2, 3], [2, 0, 3]) == -2            # ... in the transpose
    assert run([0, 2, 1, 3], good[1], good[2], good[3]) == -2              # extents go down
    assert run([0, 1, 2, 3], good[1], [0, 1, 2, 2], good[3]) == -2         # transpose holds another number of edges
    assert run([1, 1, 2, 3], good[1], good[2], good[3]) == -2              # extents do not start at 0


def test_product_refuses_cpu_tensors(hip_lib):
    import numpy as np
    import pytest
    import torch

    import gts
    from gts import ops

    g = gts.Graph(np.array([0]), np.array([1]), 2)
    with pytest.raises(gts.GtsError, match="MI355X only"):
        ops.spmm_max_fwd(g, torch.zeros(2, 4))


def test_header_cites_reference_lines():
    text = open(_lib.HEADER_PATH).read()
    for cite in ("model/networks.py:25", "data_processing/graph_io.py:21-24",
                 "scripts/generate_gnn_predictions.py:55-61"):
        assert cite in text
    assert os.path.exists(build.LIB_PATH)
