"""Soft Dice + cross-entropy without a GPU: the float64 definition of tests/dice_ref.py against autograd and
against the evaluation's hard Dice, the argument checks of the two C entry points, make_voxel_loss and the flags
of the two training scripts."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dice_ref

ERR_NULL, ERR_SHAPE, ERR_ARGKIND = -1, -2, -3


def _inputs(n, c, seed, ignored=0.1):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, generator=g) * 3).float()
    y = torch.randint(0, c, (n,), generator=g)
    y[torch.rand(n, generator=g) < ignored] = dice_ref.IGNORE
    return x, y


@pytest.mark.parametrize("regions", ["brats", "classes"])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.0, 2.0), (0.7, 0.0)])
def test_closed_form_gradient_equals_autograd(regions, weights):
    x, y = _inputs(517, 4, seed=11)
    w = torch.tensor([0.1, 1.0, 2.0, 2.0])
    for class_w in (w, None):
        ref = dice_ref.dice_ce_ref(x, y, class_w, regions, weights[0], weights[1], smooth=1.0)
        assert bool((ref.grad[y == dice_ref.IGNORE] == 0).all())
        assert float(ref.grad.abs().max()) > 0
        assert float((ref.grad - ref.grad_closed).abs().max()) <= 1e-12
        # every entry lies under the stated bound on |dL/dp| (|dL/dx_j| = |p_j (g_j - sum g p)| <= 2 max |g|)
        assert float(ref.grad.abs().max()) <= 2 * ref.s_bound


def test_saturated_soft_dice_is_the_evaluations_hard_dice():
    from model import evaluation

    rng = np.random.default_rng(5)
    n = 4000
    truth = rng.integers(0, 4, n)
    pred = np.where(rng.random(n) < 0.7, truth, rng.integers(0, 4, n))
    x = torch.zeros(n, 4)
    x[torch.arange(n), torch.from_numpy(pred)] = 40.0
    ref = dice_ref.dice_ce_ref(x, torch.from_numpy(truth), None, "brats", 0.0, 1.0, smooth=1e-6)
    confusion = np.zeros((5, 5), dtype=np.int64)
    np.add.at(confusion, (pred, truth), 1)
    hard = evaluation.dices_from_confusion(confusion)
    assert abs((1.0 - float(ref.l_dice)) - np.mean(hard)) <= 1e-5
    assert np.allclose(ref.dices.numpy(), hard, rtol=0, atol=1e-5)


def test_region_masks():
    from gts import _lib, ops

    assert ops.dice_region_masks("brats", 4) == (0b1110, 0b1100, 0b1000)
    assert ops.dice_region_masks("classes", 5) == (2, 4, 8, 16)
    assert ops.dice_region_masks([[0, 31], (3,)], 32) == ((1 << 31) | 1, 8)
    for regions, c in (("brats", 5), ("wt", 4), ([[]], 4), ([[4]], 4), ([[-1]], 4), ([], 4), ([[1]] * 9, 4),
                       ("classes", 1)):
        with pytest.raises(_lib.GtsError):
            ops.dice_region_masks(regions, c)


def _call(lib, which, **over):
    """One of the two entry points with arguments that are all acceptable (fake non-null device pointers: every
    refusal comes before a launch), except those in `over`."""
    masks = over.pop("masks", (0b1110, 0b1100, 0b1000))
    n_groups = 3 if masks is None else len(masks)
    a = dict(logits=8, labels=8, class_w=None,
             masks=None if masks is None else (ctypes.c_uint32 * max(1, n_groups))(*masks),
             n_groups=n_groups, ce_weight=1.0, dice_weight=1.0, smooth=1.0, stats=8, workspace=8,
             workspace_bytes=1 << 20, grad_scale=None, grad=8, n=1000, n_classes=4)
    a.update(over)
    head = (a["logits"], a["labels"], a["class_w"], a["masks"], a["n_groups"], a["ce_weight"], a["dice_weight"],
            a["smooth"], a["stats"])
    if which == "fwd":
        return lib.gts_dice_ce_fwd_f32(*head, a["workspace"], a["workspace_bytes"], a["n"], a["n_classes"], None)
    return lib.gts_dice_ce_bwd_f32(*head, a["grad_scale"], a["grad"], a["n"], a["n_classes"], None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_entry_points_refuse_bad_arguments_before_any_launch(hip_lib, which):
    lib = hip_lib
    pointers = ["logits", "labels", "masks", "stats"] + (["workspace"] if which == "fwd" else ["grad"])
    for name in pointers:
        assert _call(lib, which, **{name: None}) == ERR_NULL, name
    for over in (dict(n=0), dict(n=-5), dict(n_classes=0), dict(n_classes=33), dict(masks=()),
                 dict(masks=(2,) * 9)):
        assert _call(lib, which, **over) == ERR_SHAPE, over
    if which == "fwd":
        need = lib.gts_dice_ce_workspace(1000, 3)
        assert need == 1 * (2 + 3 * 3) * 4
        assert _call(lib, which, workspace_bytes=need - 1) == ERR_SHAPE
        assert lib.gts_dice_ce_workspace(1025, 8) == 2 * 26 * 4
        assert lib.gts_dice_ce_workspace(0, 3) == 0 and lib.gts_dice_ce_workspace(10, 9) == 0
    inf, nan = float("inf"), float("nan")
    for over in (dict(masks=(2, 0, 4)), dict(masks=(2, 16)), dict(masks=(1 << 31,)), dict(ce_weight=-1.0),
                 dict(dice_weight=-1e-3), dict(ce_weight=nan), dict(dice_weight=inf), dict(smooth=0.0),
                 dict(smooth=-1.0), dict(smooth=nan), dict(smooth=inf), dict(n_classes=2, masks=(4,))):
        assert _call(lib, which, **over) == ERR_ARGKIND, over


def test_ce_kind_is_the_weighted_cross_entropy_call(monkeypatch):
    from gts import ops
    from model import losses

    calls = []

    def forbidden(*args, **kwargs):
        raise AssertionError("kind 'ce' must not reach the Dice op")

    monkeypatch.setattr(ops, "weighted_cross_entropy", lambda *a, **k: calls.append((a, k)) or "the loss")
    monkeypatch.setattr(ops, "dice_ce_loss", forbidden)
    logits, labels, w = torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64), torch.ones(4)
    loss = losses.make_voxel_loss("ce", w, dice_weight=3.0, smooth=0.5, regions="classes")
    assert loss(logits, labels) == "the loss"
    assert len(calls) == 1 and calls[0][1] == {}
    assert all(got is want for got, want in zip(calls[0][0], (logits, labels, w))) and len(calls[0][0]) == 3
    with pytest.raises(ValueError):
        losses.make_voxel_loss("dice", w)
    with pytest.raises(ValueError):
        losses.make_voxel_loss("dice_ce", w, smooth=0.0)


def test_dice_ce_kind_passes_its_settings(monkeypatch):
    from gts import ops
    from model import losses

    calls = []
    monkeypatch.setattr(ops, "dice_ce_loss", lambda *a, **k: calls.append((a, k)) or "the loss")
    w = torch.ones(4)
    loss = losses.make_voxel_loss("dice_ce", w, dice_weight=0.5, smooth=2.0, regions="classes")
    assert loss("x", "y") == "the loss"
    assert calls == [(("x", "y", w), dict(regions="classes", ce_weight=1.0, dice_weight=0.5, smooth=2.0))]


@pytest.mark.parametrize("module,required", [("train_refinement_cnn", ["-r", "run"]), ("train_joint", ["-r", "run"])])
def test_parsers_take_the_loss_flags(module, required):
    import importlib

    cli = importlib.import_module(f"scripts.{module}")
    args = cli.build_cli_parser().parse_args(required)
    assert (args.loss, args.dice_weight, args.dice_smooth, args.dice_regions) == ("ce", 1.0, 1.0, "brats")
    assert cli.voxel_loss_from_args(args, [0.1, 1.0, 2.0, 2.0]) is None
    args = cli.build_cli_parser().parse_args(required + ["--loss", "dice_ce", "--dice_weight", "0.5", "--dice_smooth",
                                                     "1e-5", "--dice_regions", "classes"])
    assert (args.loss, args.dice_weight, args.dice_smooth, args.dice_regions) == ("dice_ce", 0.5, 1e-5, "classes")
    for bad in (["--loss", "dice"], ["--dice_regions", "wt"]):
        with pytest.raises(SystemExit):
            cli.build_cli_parser().parse_args(required + bad)
