"""What tests/test_gpu_conv3d_edges.py covers, checked without a GPU: tests/conv3d_ref.plan against the
library's own workspace queries for every case of that file, each coverage claim of its docstring from plan()
over its case lists, and that its integer-valued operands keep every partial sum an exact float32."""
import pytest
import torch

from tests.conv3d_ref import BIAS_PARTIAL_FLOATS, conv, data_grad, data_plan, plan, weight_grad
from tests.test_gpu_conv3d_edges import LAYER_CASES, REPEAT_CASE, WGRAD_CASES, case_id, integer_operands

PAIRS = {(cc, t) for cc in (4, 8, 12, 16) for t in (1, 2)}
FAMILIES = {(4, 1): 512, (8, 1): 256, (12, 1): 171, (16, 1): 128, (16, 2): 64}     # (CC, chunks): whole-launch target
EXACT = float(1 << 24)


def _family(p):
    return p.cc, p.chunks


# ---- the restatement against the library --------------------------------------------------------------
def test_plan_matches_the_workspace_queries(hip_lib):
    assert REPEAT_CASE in WGRAD_CASES
    for dims, cin, cout in LAYER_CASES + WGRAD_CASES:
        p, dp = plan(dims, cin, cout), data_plan(dims, cin, cout)
        assert hip_lib.gts_conv3d_fwd_workspace(cin, cout) == 4 * p.packed
        padded = (dims[0] + 4) * (dims[1] + 4) * (dims[2] + 4)
        assert dp.packed % 64 == 0                              # the library rounds it up to 64 floats
        assert hip_lib.gts_conv3d_bwd_data_workspace(*dims, cin, cout) == 4 * (dp.packed + padded * cin)
        partials = p.nsplit * p.chunks * p.ntn * 16 * cout
        assert hip_lib.gts_conv3d_bwd_weight_workspace(*dims, cin, cout) == 4 * (partials + BIAS_PARTIAL_FLOATS)


def test_plan_arithmetic_on_known_layers():
    """Worked by hand from csrc/gts_conv3d.hip, so that plan() is not only compared with itself."""
    p = plan((48, 48, 48), 8, 16)
    assert (p.cc, p.chunks, p.last, p.nt, p.bricks) == (8, 1, 8, 1, 432)
    assert (p.ntn, p.groups, p.target, p.per_split, p.nsplit, p.last_split) == (63, 2, 256, 2, 216, 2)
    p = plan((20, 52, 16), 32, 17)
    assert (p.cc, p.chunks, p.last, p.nt, p.bricks) == (16, 2, 16, 2, 65)
    assert (p.ntn, p.groups, p.target, p.per_split, p.nsplit, p.last_split) == (125, 4, 64, 2, 33, 1)
    p = data_plan((5, 5, 17), 13, 1)
    assert (p.cc, p.chunks, p.last, p.nt, p.bricks) == (4, 1, 1, 1, 3 * 3 * 2)
    assert all(plan((4, 4, 16), c, 1).target == t for c, t in ((1, 512), (5, 256), (9, 171), (13, 128), (32, 64)))


# ---- coverage claims ----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [plan, data_plan], ids=["forward", "data-gradient"])
def test_every_conv_kernel_instantiation_is_reached(route):
    plans = [route(*c) for c in LAYER_CASES]
    assert {(p.cc, p.nt) for p in plans} == PAIRS
    assert {p.nt for p in plans if p.chunks == 2} == {1, 2}
    assert {1, 4, 16} <= {p.last for p in plans if p.chunks == 2}


def test_every_wgrad_kernel_instantiation_is_reached():
    plans = [plan(*c) for c in LAYER_CASES + WGRAD_CASES]
    assert {(p.cc, p.nt) for p in plans} == PAIRS
    assert {p.nt for p in plans if p.chunks == 2} == {1, 2}
    assert {1, 4, 16} <= {p.last for p in plans if p.chunks == 2}


@pytest.mark.parametrize("family", sorted(FAMILIES), ids=lambda f: f"CC{f[0]}x{f[1]}")
def test_split_plans_per_family(family):
    plans = [p for p in (plan(*c) for c in WGRAD_CASES) if _family(p) == family]
    assert all(p.target == FAMILIES[family] for p in plans)
    for mt in (1, 2):
        mine = [p for p in plans if p.nt == mt]
        assert any(p.bricks == p.target and p.per_split == 1 and p.nsplit == p.target for p in mine), \
            f"no case at the whole-launch target of {FAMILIES[family]} bricks (MT {mt})"
        assert any(p.per_split >= 2 and p.last_split < p.per_split for p in mine), f"no short last split (MT {mt})"
        # the first plan past the target: two bricks in every split but the last, which has one
        assert any(p.per_split == 2 and p.last_split == 1 for p in mine), f"no 2-brick splits ending on 1 (MT {mt})"


def test_a_split_of_three_bricks_and_the_repeat_case():
    assert any(p.per_split >= 3 and p.last_split < p.per_split for p in (plan(*c) for c in WGRAD_CASES))
    p = plan(*REPEAT_CASE)
    assert p.chunks == 2 and p.per_split >= 2 and p.last_split < p.per_split


def test_volume_edges_are_in_the_lists():
    volumes = {c[0] for c in LAYER_CASES}
    assert {(4, 4, 16), (5, 5, 17), (3, 4, 15)} <= volumes
    assert plan((5, 5, 17), 1, 1).bricks == 8 and plan((4, 4, 16), 1, 1).bricks == 1
    used = {n for _, ci, co in LAYER_CASES for n in (ci, co)}
    assert {1, 4, 12, 13, 29, 31} <= used


# ---- the integer-valued operands never round ----------------------------------------------------------
@pytest.mark.parametrize("case", LAYER_CASES, ids=case_id)
def test_integer_operands_stay_exact_in_every_launch(case):
    x, w, b, dy = (t.double().abs() for t in integer_operands(*case))
    for t in (x, w, b, dy):
        assert torch.equal(t, t.round())
    assert conv(x, w, b).max() < EXACT
    assert data_grad(dy, w, case[0]).max() < EXACT               # the fold's up to 125 positions included
    dw, db = weight_grad(x, dy, case[2])
    assert dw.max() < EXACT and db.max() < EXACT


@pytest.mark.parametrize("case", WGRAD_CASES, ids=case_id)
def test_integer_operands_stay_exact_in_the_split_plans(case):
    x, _, _, dy = (t.double().abs() for t in integer_operands(*case))
    dw, db = weight_grad(x, dy, case[2])
    assert dw.max() < EXACT and db.max() < EXACT
