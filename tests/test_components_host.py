"""gts.components without a GPU: the scipy reference's own properties, the argument checks of the C entry
points, the workspace limits, the CLI flags and the refusals of the Python wrappers."""
import ctypes

import numpy as np
import pytest
import torch

from tests import components_ref as ref


def _two_bars():
    """Two bars that touch across a voxel edge, and a lone voxel of another label."""
    vol = np.zeros((4, 5, 6), dtype=np.int16)
    vol[0, 0, 0:3] = 1
    vol[0, 1, 3:6] = 2
    vol[3, 4, 5] = 4
    return vol


def test_reference_on_two_bars():
    vol = _two_bars()
    assert ref.ref_labels(vol, 6)[1] == 3 and ref.ref_labels(vol, 26)[1] == 2
    roots = ref.ref_roots(vol, 6)
    assert roots.dtype == np.int32 and set(np.unique(roots)) == {0, 1, 1 + 6 + 3, 120}
    roots = ref.ref_roots(vol, 26)
    assert set(np.unique(roots)) == {0, 1, 120} and (roots == 1).sum() == 6
    ref.check_roots(roots, vol, 26)
    with pytest.raises(AssertionError):
        ref.check_roots(roots, vol, 6)
    out, stats = ref.ref_filter(vol, 2, 26)
    assert stats == [2, 1, 1, 0] and out[3, 4, 5] == 0 and np.array_equal(out[0], vol[0])
    out, stats = ref.ref_filter(vol, 4, 6)
    assert stats == [3, 3, 7, 0] and not out.any()
    for none in (0, 1):
        out, stats = ref.ref_filter(vol, none, 6)
        assert stats == [3, 0, 0, 0] and np.array_equal(out, vol)


def test_reference_enhancing_rule_and_lifted_shapes():
    vol = np.zeros((6, 6, 12), dtype=np.int16)
    vol[1:4, 1:4, 1:4] = 2
    vol[2, 2, 1:4] = 4                                    # 3 enhancing voxels inside the block
    vol[5, 5, 8:11] = 4                                   # an island of 3 more
    et = dict(et_label=4, et_min_voxels=5, et_replacement=1)
    out, stats = ref.ref_filter(vol, 0, 26, **et)         # 6 enhancing voxels in all: untouched
    assert stats == [2, 0, 0, 0] and np.array_equal(out, vol)
    out, stats = ref.ref_filter(vol, 4, 26, **et)         # the island goes first, 3 are left: relabelled
    assert stats == [2, 1, 3, 3] and (out == 1).sum() == 3 and not (out == 4).any() and (out == 2).sum() == 24
    out, stats = ref.ref_filter(vol, 4, 26, et_label=4, et_min_voxels=0, et_replacement=1)
    assert stats == [2, 1, 3, 0] and (out == 4).sum() == 3
    line = np.array([1, 1, 0, 2, 0, 0, 3, 3, 3], dtype=np.int16)
    for shape in [(9,), (1, 9), (9, 1, 1), (1, 1, 9, 1)]:
        roots = ref.ref_roots(line.reshape(shape), 6)
        assert roots.shape == shape and roots.ravel().tolist() == [1, 1, 0, 4, 0, 0, 7, 7, 7]


def test_argument_checks_run_before_any_launch(hip_lib):
    one = ctypes.c_void_p(16)
    big = 1 << 40
    roots, filt = hip_lib.gts_components_roots_i16, hip_lib.gts_components_filter_i16
    assert roots(None, 4, 4, 4, 26, one, one, big, None) == -1
    assert roots(one, 4, 4, 4, 26, None, one, big, None) == -1
    assert roots(one, 4, 4, 4, 26, one, None, big, None) == -1
    assert filt(None, 4, 4, 4, 26, 5, 4, 0, 1, one, one, one, big, None) == -1
    assert filt(one, 4, 4, 4, 26, 5, 4, 0, 1, None, one, one, big, None) == -1
    assert filt(one, 4, 4, 4, 26, 5, 4, 0, 1, one, None, one, big, None) == -1
    assert filt(one, 4, 4, 4, 26, 5, 4, 0, 1, one, one, None, big, None) == -1
    for bad_connectivity in (18, 0, 7):
        assert roots(one, 4, 4, 4, bad_connectivity, one, one, big, None) == -2
        assert filt(one, 4, 4, 4, bad_connectivity, 5, 4, 0, 1, one, one, one, big, None) == -2
    for extents in [(-1, 4, 4), (4, -1, 4), (4, 4, -1), (2048, 1024, 1024), (1 << 40, 1 << 40, 1 << 40)]:
        assert roots(one, *extents, 26, one, one, big, None) == -2
        assert filt(one, *extents, 6, 5, 4, 0, 1, one, one, one, big, None) == -2
    need = hip_lib.gts_components_workspace(4, 4, 4)
    assert need >= 3 * 4 * 64
    assert roots(one, 4, 4, 4, 26, one, one, need - 1, None) == -2
    assert filt(one, 4, 4, 4, 26, 5, 4, 0, 1, one, one, one, need - 1, None) == -2
    for extents in [(0, 4, 4), (4, 0, 4), (4, 4, 0)]:     # nothing to do: accepted without touching memory
        assert roots(one, *extents, 26, one, one, 0, None) == 0
        assert filt(one, *extents, 26, 5, 4, 0, 1, one, one, one, 0, None) == 0


def test_workspace_limits(hip_lib):
    ws = hip_lib.gts_components_workspace
    n = 240 * 240 * 155
    assert 3 * 4 * n <= ws(240, 240, 155) <= 3 * 4 * n + 4096
    assert ws(2047, 1024, 1024) > 0                       # just below 2^31 voxels
    assert ws(2048, 1024, 1024) <= 0 and ws(1 << 31, 1, 1) <= 0 and ws(1 << 21, 1 << 21, 1 << 21) <= 0
    assert ws(-1, 4, 4) <= 0 and ws(0, 4, 4) <= 0
    assert ws(1, 1, 1) > 0


def test_the_three_parsers_carry_the_flags():
    from scripts import generate_gnn_predictions, generate_joint_predictions, segment_scans
    from scripts import cleanup

    for module, base in ((segment_scans, ["-d", "in", "-o", "out", "-g", "gnn.pt"]),
                         (generate_gnn_predictions, []), (generate_joint_predictions, [])):
        args = module.build_parser().parse_args(base)
        assert (args.min_component_voxels, args.connectivity, args.min_enhancing_voxels) == (0, 26, 0)
        assert cleanup.from_args(args) is None
        args = module.build_parser().parse_args(base + ["--min_component_voxels", "30", "--connectivity", "6",
                                                        "--min_enhancing_voxels", "200"])
        assert (args.min_component_voxels, args.connectivity, args.min_enhancing_voxels) == (30, 6, 200)
        picked = cleanup.from_args(args)
        assert (picked.min_voxels, picked.connectivity, picked.et_min_voxels) == (30, 6, 200) and picked.drops_components
        only_et = cleanup.from_args(module.build_parser().parse_args(base + ["--min_enhancing_voxels", "9"]))
        assert only_et is not None and not only_et.drops_components
        with pytest.raises(SystemExit):
            module.build_parser().parse_args(base + ["--connectivity", "18"])


def test_wrappers_refuse_what_the_kernels_do_not_take(hip_lib):
    from gts import GtsError, components

    labels = torch.zeros((4, 4, 4), dtype=torch.int16)
    for call in (lambda t: components.remove_small_components(t, 5), components.component_roots):
        with pytest.raises(GtsError, match="MI355X only"):
            call(labels)
        with pytest.raises(GtsError, match="int16"):
            call(labels.to(torch.int32))
        with pytest.raises(GtsError, match="int16"):
            call(labels.float())
        with pytest.raises(GtsError, match="empty"):
            call(torch.zeros((0, 4, 4), dtype=torch.int16))
    with pytest.raises(GtsError, match="connectivity"):
        components.component_roots(labels, 18)
    with pytest.raises(GtsError, match="at most 3"):
        components.lift_shape((2, 2, 2, 2))
    assert components.lift_shape((1, 40, 33, 21)) == (40, 33, 21) and components.lift_shape((64, 80)) == (1, 64, 80)
