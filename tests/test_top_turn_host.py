"""Argument handling of the training step's top-layer entry points (gts_sage_top_layer_train_f32 and the stack calls built on
it), pinned on the CPU: every case below returns before anything is launched, so a fake non-null pointer stands in for
device memory (as in test_gemm_abi_host.py).  Codes: -1 GTS_ERR_NULL, -2 GTS_ERR_SHAPE."""
import ctypes

import pytest

from gts import _lib

P = ctypes.c_void_p(16)   # non-null, never dereferenced
HUGE = 1 << 40
TOP_ARGS = ("h", "mx", "w_self", "w_neigh", "bias", "labels", "class_w", "normalise", "logits", "g", "gw_self", "gw_neigh",
            "g_bias", "out3", "workspace", "workspace_bytes", "m", "k", "n_classes", "stream")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _top(lib, **changed):
    args = dict.fromkeys(TOP_ARGS, P)
    args.update(class_w=None, normalise=1, workspace_bytes=HUGE, m=1000, k=256, n_classes=4, stream=None)
    args.update(changed)
    return lib.gts_sage_top_layer_train_f32(*[args[name] for name in TOP_ARGS])


def test_top_layer_workspace_is_sized_by_its_partials_and_rows(lib):
    chunk_floats = 512 * (2 * 4 * 256 + 4)
    for m in (1, 3, 4, 1000, 1024, 1025, 60000):
        want = chunk_floats + (m + 3) // 4 * 4 + 2 * ((m + 1023) // 1024)
        assert lib.gts_sage_top_layer_train_workspace(m, 256, 4) == 4 * want
    for m, k, c in ((0, 256, 4), (-1, 256, 4), (1 << 31, 256, 4), (1000, 128, 4), (1000, 260, 4), (1000, 256, 8), (1000, 256, 3)):
        assert lib.gts_sage_top_layer_train_workspace(m, k, c) == 0


def test_top_layer_entry_point_checks_pointers_shape_and_workspace(lib):
    for name in TOP_ARGS:
        if name not in ("class_w", "normalise", "workspace_bytes", "m", "k", "n_classes", "stream"):
            assert _top(lib, **{name: None}) == -1, name
    for changed in (dict(m=0), dict(m=-5), dict(m=1 << 31), dict(k=128), dict(k=512), dict(n_classes=8), dict(n_classes=1)):
        assert _top(lib, **changed) == -2, changed
    need = lib.gts_sage_top_layer_train_workspace(1000, 256, 4)
    assert _top(lib, workspace_bytes=need - 1) == -2
    assert _top(lib, workspace_bytes=0) == -2
    assert _top(lib, h=None, m=0) == -1            # pointers are looked at first


def _stack_tables(widths, n_params):
    return (ctypes.c_int64 * len(widths))(*widths), (ctypes.c_void_p * n_params)(*([16] * n_params))


def test_stack_training_forward_takes_a_256_to_4_top_layer_only(lib):
    def call(widths, n_rows=1000, labels=P, g_top=P, out3=P, top_ws=P, top_bytes=HUGE, grads=None, arena_bytes=HUGE):
        c_widths, table = _stack_tables(widths, 5 * (len(widths) - 1))
        grads = table if grads is None else grads
        return lib.gts_sage_pool_stack_train_fwd_f32(P, P, None, 0, 0, 0, 0, P, table, n_rows, c_widths, len(widths) - 1, 1, 1,
                                                     P, arena_bytes, labels, None, 1, g_top, grads, out3, top_ws, top_bytes,
                                                     None)

    good = (20, 256, 256, 4)
    assert call(good, labels=None) == -1
    assert call(good, g_top=None) == -1
    assert call(good, out3=None) == -1
    assert call(good, top_ws=None) == -1
    holes = (ctypes.c_void_p * 15)(*([16] * 12 + [None, 16, 16]))
    assert call(good, grads=holes) == -1                       # a destination of the top layer's gradients is missing
    assert call(good, top_bytes=lib.gts_sage_top_layer_train_workspace(1000, 256, 4) - 1) == -2
    assert call(good, arena_bytes=64) == -2
    assert call(good, n_rows=0) == -2                          # no rows: the plain forward's case, not this call's
    for widths in ((20, 256, 256, 8), (20, 128, 4), (20, 256, 64, 4), (4, 4)):
        assert call(widths) == -2, widths


def test_stack_backward_with_the_top_done_takes_that_top_layer_only(lib):
    def call(widths, n_rows=1000, top_done=1, gout=P):
        c_widths, table = _stack_tables(widths, 5 * (len(widths) - 1))
        return lib.gts_sage_pool_stack_bwd_top_f32(P, P, P, None, 0, 0, 0, 0, gout, P, table, n_rows, c_widths,
                                                   len(widths) - 1, 1, 1, P, table, None, P, HUGE, top_done, None)

    assert call((20, 256, 256, 4), gout=None) == -1
    for widths in ((20, 256, 256, 8), (20, 128, 4), (4, 4)):
        assert call(widths) == -2, widths
    assert call((20, 256, 256, 4), n_rows=0) == -2
    assert call((20, 256, 256, 4), n_rows=1 << 31) == -2
    # top_done = 0 is gts_sage_pool_stack_bwd_f32: the same answers to the same bad arguments
    c_widths, table = _stack_tables((20, 256, 4), 10)
    for arg_bytes in (1, 2):
        old = lib.gts_sage_pool_stack_bwd_f32(P, P, P, None, 0, 0, 0, 0, P, P, table, 1000, c_widths, 2, arg_bytes, 1, P, table,
                                              None, P, 64, None)
        new = lib.gts_sage_pool_stack_bwd_top_f32(P, P, P, None, 0, 0, 0, 0, P, P, table, 1000, c_widths, 2, arg_bytes, 1, P,
                                                  table, None, P, 64, 0, None)
        assert old == new == (-2 if arg_bytes == 1 else -3)
