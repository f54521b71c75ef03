"""Argument handling of the dense-GEMM entry points and of the option registry, pinned on the CPU: every case below
returns before anything is launched, so a fake non-null pointer stands in for device memory (as in test_abi.py).
Codes: -1 GTS_ERR_NULL, -2 GTS_ERR_SHAPE, -3 GTS_ERR_ARGKIND."""
import ctypes
import os
import re

import pytest

from gts import _lib

P = ctypes.c_void_p(16)   # non-null, never dereferenced
BIG_M = 1 << 31
BIG_W = 1 << 20
INT32_MIN = -(1 << 31)


def fwd(a0=P, w0=P, a1=None, w1=None, bias=None, out=P, m=8, n=8, k0=8, k1=0, relu=0, relu_bits=None):
    return "gts_linear_fwd_f32", (a0, w0, a1, w1, bias, out, m, n, k0, k1, relu, relu_bits, None, None)


def fwd_chain(a0=P, w0=P, a1=None, w1=None, bias=None, out=P, w2=P, bias2=None, out2=P, m=8, n=8, k0=8, k1=0, relu=0,
              n2=8, relu2=0, relu_bits=None):
    return "gts_linear_fwd_chain_f32", (a0, w0, a1, w1, bias, out, w2, bias2, out2, m, n, k0, k1, relu, n2, relu2,
                                        relu_bits, None, None)


def bwd_input(g0=P, w0=P, g1=None, w1=None, relu_mask=None, gin=P, m=8, k=8, n0=8, n1=0):
    return "gts_linear_bwd_input_f32", (g0, w0, g1, w1, relu_mask, gin, m, k, n0, n1, None)


def bwd_input_t(g0=P, w0=P, g1=None, w1=None, relu_mask=None, relu_bits=None, gin=P, m=8, k=8, n0=8, n1=0):
    return "gts_linear_bwd_input_t_f32", (g0, w0, g1, w1, relu_mask, relu_bits, gin, m, k, n0, n1, None, None)


def bwd_input_chain_t(g0=P, w0=P, g1=None, w1=None, relu_mask=None, relu_bits=None, gin=P, w2=P, gin2=P, m=8, k=8,
                      n0=8, n1=0, k2=8):
    return "gts_linear_bwd_input_chain_t_f32", (g0, w0, g1, w1, relu_mask, relu_bits, gin, w2, gin2, m, k, n0, n1, k2,
                                                None, None)


def bwd_input_t_act(g0=P, w0=P, g1=None, w1=None, act_out=P, activation=1, gin=P, g_bias=None, workspace=None,
                    workspace_bytes=0, m=8, k=8, n0=8, n1=0):
    return "gts_linear_bwd_input_t_act_f32", (g0, w0, g1, w1, act_out, activation, gin, g_bias, workspace,
                                              workspace_bytes, m, k, n0, n1, None, None)


def gat_fc_scores(h=P, w_fc=P, attn_l=P, attn_r=P, ft=P, el=P, er=P, m=8, heads=2, dim=4, k=8):
    return "gts_gat_fc_scores_f32", (h, w_fc, attn_l, attn_r, ft, el, er, None, 0, m, heads, dim, k, None, None)


# per entry point: the name of its first operand, of the two halves of its second pair with that pair's length, of a
# reduction width that must be a multiple of 4, and of a width bounded by 2^20
LINEAR = [
    (fwd, "a0", ("a1", "w1", "k1"), "k0", "n"),
    (fwd_chain, "a0", ("a1", "w1", "k1"), "k0", "n"),
    (bwd_input, "g0", ("g1", "w1", "n1"), "n0", "k"),
    (bwd_input_t, "g0", ("g1", "w1", "n1"), "n0", "k"),
    (bwd_input_chain_t, "g0", ("g1", "w1", "n1"), "n0", "k"),
    (bwd_input_t_act, "g0", ("g1", "w1", "n1"), "n0", "k"),
]


def _linear_cases():
    cases = []
    for make, first, (a1, w1, k1), width4, width in LINEAR:
        cases += [
            (make(**{first: None}), -1),
            (make(**{a1: P, k1: 8}), -1),                 # second pair half-given
            (make(**{w1: P, k1: 8}), -1),
            (make(**{width4: 6}), -2),
            (make(**{k1: 6, a1: P, w1: P}), -2),
            (make(**{width: BIG_W}), -2),
            (make(**{width4: BIG_W}), -2),
            (make(m=BIG_M), -2),
            (make(m=-1), -2),
            (make(**{a1: P, w1: P, k1: 0}), -2),          # second pair given with length 0
            (make(m=0), 0),
            (make(m=0, **{a1: P, w1: P, k1: 8}), 0),
            (make(**{first: None, "m": 0}), -1),          # nulls are seen before the sizes
        ]
    return cases


CASES = _linear_cases() + [
    # ReLU mask bits need whole 64-column blocks
    (fwd(relu_bits=P, n=96), -2),
    (fwd(relu_bits=P, n=64, m=0), 0),
    (fwd_chain(relu_bits=P, n=96), -2),
    (fwd_chain(relu_bits=P, n=64, m=0), 0),
    (fwd(out=None), -1),
    # the chained second stage
    (fwd_chain(w2=None), -1),
    (fwd_chain(out2=None), -1),
    (fwd_chain(n=6), -2),
    (fwd_chain(n2=0), -2),
    (fwd_chain(n2=BIG_W), -2),
    (fwd(n=6, m=0), 0),                                   # the single forward takes any output width
    (bwd_input_chain_t(w2=None), -1),
    (bwd_input_chain_t(gin2=None), -1),
    (bwd_input_chain_t(k2=0), -2),
    (bwd_input_chain_t(k2=BIG_W), -2),
    # input gradients: output width a multiple of 4, the bits only beside the float mask
    (bwd_input(k=6), -2),
    (bwd_input_t(k=6), -2),
    (bwd_input_chain_t(k=6), -2),
    (bwd_input_t_act(k=6), -2),
    (bwd_input_t(relu_bits=P), -1),
    (bwd_input_chain_t(relu_bits=P), -1),
    (bwd_input_t(relu_bits=P, relu_mask=P, k=96), -2),
    (bwd_input_chain_t(relu_bits=P, relu_mask=P, k=96), -2),
    (bwd_input_t(relu_bits=P, relu_mask=P, k=64, m=0), 0),
    (bwd_input_chain_t(relu_bits=P, relu_mask=P, k=64, m=0), 0),
    # the activation fold: nulls, then the activation, then the shapes, then the workspace
    (bwd_input_t_act(activation=0), -3),
    (bwd_input_t_act(activation=3), -3),
    (bwd_input_t_act(activation=2, m=0), 0),
    (bwd_input_t_act(activation=0, n0=6), -3),            # bad activation and bad shape: the activation is reported
    (bwd_input_t_act(activation=3, m=BIG_M), -3),
    (bwd_input_t_act(activation=0, act_out=None), -1),    # null and bad activation: the null is reported
    (bwd_input_t_act(act_out=None), -1),
    (bwd_input_t_act(g_bias=P), -1),                      # g_bias without workspace
    (bwd_input_t_act(g_bias=P, activation=3), -1),
    (bwd_input_t_act(g_bias=P, workspace=P, n0=6), -2),
    # GATConv's fc with scores
    (gat_fc_scores(attn_l=None), -1),
    (gat_fc_scores(attn_r=None), -1),
    (gat_fc_scores(h=None), -1),
    (gat_fc_scores(el=None), -1),
    (gat_fc_scores(k=6), -2),
    (gat_fc_scores(heads=0), -2),
    (gat_fc_scores(heads=1 << 10, dim=1 << 10), -2),
    (gat_fc_scores(m=BIG_M), -2),
    (gat_fc_scores(m=0), 0),
]


@pytest.mark.parametrize("call,expected", CASES, ids=[f"{i}-{c[0][0]}" for i, c in enumerate(CASES)])
def test_plain_entry_points(hip_lib, call, expected):
    name, args = call
    assert getattr(hip_lib, name)(*args) == expected


def test_act_fold_workspace_is_checked_after_the_shapes(hip_lib):
    need = hip_lib.gts_linear_bwd_input_t_act_workspace(8, 8)
    assert need > 0
    name, args = bwd_input_t_act(g_bias=P, workspace=P, workspace_bytes=need - 1)
    assert getattr(hip_lib, name)(*args) == -2
    # m = 0 asks for no workspace at all
    assert hip_lib.gts_linear_bwd_input_t_act_workspace(0, 8) == 0
    name, args = bwd_input_t_act(g_bias=P, workspace=P, workspace_bytes=0, m=0)
    assert getattr(hip_lib, name)(*args) == 0


def _ptr_array(n, hole=None):
    arr = (ctypes.c_void_p * n)(*[16] * n)
    if hole is not None:
        arr[hole] = None
    return arr


def test_weight_gradient_entry_point(hip_lib):
    f = hip_lib.gts_linear_bwd_weight_f32
    m, n, k = 64, 8, 8
    for q in (1, 3, 32):
        need = hip_lib.gts_linear_bwd_weight_workspace(m, n, k, q)
        assert need > 0
        arr = _ptr_array(q)
        assert f(None, arr, arr, None, q, P, need, m, n, k, None) == -1
        assert f(arr, None, arr, None, q, P, need, m, n, k, None) == -1
        assert f(arr, arr, None, None, q, P, need, m, n, k, None) == -1
        assert f(arr, arr, arr, None, q, None, need, m, n, k, None) == -1
        assert f(arr, arr, arr, None, q, P, need - 1, m, n, k, None) == -2
        assert f(arr, arr, arr, None, q, P, need, m, 6, k, None) == -2
        assert f(arr, arr, arr, None, q, P, need, m, n, 6, None) == -2
        assert f(arr, arr, arr, None, q, P, need, 0, n, k, None) == -2
        assert f(arr, arr, arr, None, q, P, need, BIG_M, n, k, None) == -2
        assert f(arr, arr, arr, None, q, P, need, m, BIG_W, k, None) == -2
        assert f(arr, arr, arr, None, q, P, need, m, n, BIG_W, None) == -2
        # a null inside the pointer arrays is found after the sizes and before any launch
        holed = _ptr_array(q, hole=q - 1)
        assert f(holed, arr, arr, None, q, P, need, m, n, k, None) == -1
        assert f(arr, holed, arr, None, q, P, need, m, n, k, None) == -1
        assert f(arr, arr, holed, None, q, P, need, m, n, k, None) == -1
        assert f(holed, arr, arr, None, q, P, need - 1, m, n, k, None) == -2
    arr = _ptr_array(33)
    for q in (0, 33, -1):
        assert f(arr, arr, arr, None, q, P, 1 << 40, m, n, k, None) == -3
        assert f(arr, arr, arr, None, q, P, 1 << 40, m, 6, k, None) == -3   # the count is checked before the shapes
        assert f(None, arr, arr, None, q, P, 1 << 40, m, n, k, None) == -1  # ... and after the nulls


def test_size_queries_return_zero_for_non_positive_sizes(hip_lib):
    for m, n, k, q in ((0, 8, 8, 1), (-1, 8, 8, 1), (64, 0, 8, 1), (64, 8, 0, 1), (64, 8, -4, 1), (64, 8, 8, 0),
                       (64, 8, 8, 33), (64, 8, 8, -1)):
        assert hip_lib.gts_linear_bwd_weight_workspace(m, n, k, q) == 0
    assert hip_lib.gts_linear_bwd_weight_workspace(64, 8, 8, 32) > 0
    for m, k in ((0, 8), (-1, 8), (8, 0), (8, -4)):
        assert hip_lib.gts_linear_bwd_input_t_act_workspace(m, k) == 0
    for m, heads, dim in ((0, 2, 64), (-1, 2, 64), (8, 0, 64), (8, 2, 0), (8, 2, -64), (8, 2, 96)):
        assert hip_lib.gts_gat_fc_scores_workspace(m, heads, dim) == 0
    assert hip_lib.gts_gat_fc_scores_workspace(8, 2, 128) == 2 * 8 * 2 * 2 * 4
    for m, n in ((0, 64), (-1, 64), (8, 0), (8, -64), (8, 96)):
        assert hip_lib.gts_relu_bits_bytes(m, n) == 0
    assert hip_lib.gts_relu_bits_bytes(5, 128) == 2 * 2 * 4 * 8
    for m, n in ((0, 64), (-1, 64), (8, 0), (8, -64), (8, 96), (BIG_M, 64), (8, BIG_W)):
        assert hip_lib.gts_relu_bits_pay(m, n) == 0


def _option_ids():
    text = open(_lib.HEADER_PATH).read()
    ids = {name: int(value) for name, value in re.findall(r"#define\s+(GTS_OPT_[A-Z0-9_]+)\s+(-?\d+)", text)}
    assert len(ids) == 17
    return ids


# the options whose values are a closed list: every legal value, and some illegal ones around them
LEGAL = {
    "GTS_OPT_GEMM_TILE": ((-1, -2, 1, 3, 5, 8, 10), (-3, 0, 2, 4, 6, 7, 9, 11, 12)),
    "GTS_OPT_IGRAD_TILE": ((-1, 1, 3, 5, 8, 10), (-2, 0, 2, 4, 6, 7, 9, 11, 12)),
    "GTS_OPT_WGRAD_TILE": ((-1, 1, 2, 4, 6), (-2, 0, 3, 5, 7, 8, 9)),
    "GTS_OPT_CLUSTER_DEALING": ((0, 1, 2), (-1, 3)),
    "GTS_OPT_GAT_CLUSTER_DEALING": ((0, 1), (-1, 2)),
}
DEFAULTS = {
    "GTS_OPT_GEMM_TILE": -1, "GTS_OPT_WGRAD_TILE": -1, "GTS_OPT_IGRAD_TILE": 1, "GTS_OPT_SPMM_ROWS_PER_WAVE": 0,
    "GTS_OPT_SPMM_STREAMING": -1, "GTS_OPT_PROJECT_STREAMING": 1, "GTS_OPT_GEMM_SCHED": 1, "GTS_OPT_CLUSTER_STREAMING": -1,
    "GTS_OPT_CLUSTER_RING": 0, "GTS_OPT_CLUSTER_PER_CU": 0, "GTS_OPT_CLUSTER_CONSUMERS": 0, "GTS_OPT_PANEL_ROWS": 0,
    "GTS_OPT_GAT_WALK": 1, "GTS_OPT_GAT_CLUSTER_WAVES": 0, "GTS_OPT_GAT_CLUSTER_GROUP": 0, "GTS_OPT_GAT_CLUSTER_DEALING": 0,
    "GTS_OPT_CLUSTER_DEALING": 0,
}


def test_every_option_round_trips(hip_lib):
    ids = _option_ids()
    assert set(ids) == set(DEFAULTS) and set(LEGAL) <= set(ids)
    assert len(set(ids.values())) == len(ids)
    start = {name: hip_lib.gts_get_option(opt) for name, opt in ids.items()}
    if "GTS_OPTIONS" not in os.environ:   # no knob was set from the environment at load time: the defaults are in force
        assert start == DEFAULTS
    for name, opt in ids.items():
        legal, illegal = LEGAL.get(name, ((-1, 0, 1, 2, 7, 144, 100000), ()))
        try:
            for value in legal:
                assert hip_lib.gts_set_option(opt, value) == 0, (name, value)
                assert hip_lib.gts_get_option(opt) == value, (name, value)
                for bad in illegal:
                    assert hip_lib.gts_set_option(opt, bad) == -3, (name, bad)
                    assert hip_lib.gts_get_option(opt) == value, (name, bad)   # a refused value changes nothing
                for other, oid in ids.items():                                # no other option moved
                    assert other == name or hip_lib.gts_get_option(oid) == start[other], (name, value, other)
        finally:
            assert hip_lib.gts_set_option(opt, start[name]) == 0
        assert hip_lib.gts_get_option(opt) == start[name]


def test_unknown_options(hip_lib):
    known = set(_option_ids().values())
    for opt in (-1, 0, 9, 19, 20, 1000, INT32_MIN):
        assert opt not in known
        assert hip_lib.gts_set_option(opt, 0) == -3
        assert hip_lib.gts_get_option(opt) == INT32_MIN
