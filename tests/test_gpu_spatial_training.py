"""Training under rotated / zoomed crops (gts/augment.py) on the GPU: the joint autograd node against
the hand composition of its calls, one short epoch of RefinementModel and of JointModel (reproducible, different
from the plain augmentation, which in turn is what it was before the spatial arguments existed) and the two
command lines that see geometry."""
import io
import os
from collections import namedtuple
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests import cnn_data, spatial_ref
from tests.dataset_util import write_dataset

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HP = namedtuple("HP", "n_epochs in_feats out_classes lr lr_decay w_decay class_weights layer_sizes")
CNN_HP = HP(1, 8, 4, 1e-3, 0.98, 1e-4, [0.1, 5.0, 15.0, 15.0], [16])
BG = [1.0, -1.0, -1.0, -1.0]


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _plan(matrix, flips=(True, False, True)):
    from gts.augment import AugmentPlan

    return AugmentPlan(flips, [1.08, 0.93, 1.0, 1.05], [-0.07, 0.04, 0.0, 0.09], [0.0, 0.25, 0.0, 0.0], 0.0, (42, 0), 5,
                       matrix)


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def _state(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


# ---------------------------------------------------------------- the autograd node
@pytest.mark.parametrize("spatial", [True, False], ids=["spatial", "mirror"])
def test_joint_node_equals_the_hand_composition(spatial):
    from gts import ops
    from gts.conv3d import conv3d_bwd_data, conv3d_fwd
    from gts.joint import joint_refinement_logits
    from model.networks import CnnRefinementNet

    torch.manual_seed(5)
    shape, n_rows = (14, 12, 10), 30
    rng = np.random.default_rng(9)
    svs_host = rng.integers(-1, n_rows, size=shape).astype(np.int16)
    idx = [np.flatnonzero(rng.random(n) < 0.7) for n in shape]
    assert all(len(i) > 1 for i in idx)
    box = ops.CropBox(*idx, shape, DEV)
    dims = box.shape
    net = CnnRefinementNet(8, 4, [16]).to(DEV)
    c1, c2 = net.conv_layers[0], net.conv_layers[1]
    img = torch.randn(*shape, 4).to(DEV)
    bg = torch.tensor(BG, device=DEV)
    lists = ops.SupervoxelLists(svs_host, n_rows, DEV)
    table = torch.randn(n_rows, 4).to(DEV).requires_grad_(True)
    dy = torch.randn(int(np.prod(dims)), 4).to(DEV)
    plan = _plan(spatial_ref.matrix_from((20.0, -15.0, 10.0), 1.1) if spatial else np.eye(3))
    assert plan.spatial == spatial

    logits = joint_refinement_logits(table, img, lists.svs, box, bg, net, lists, augment=plan)
    logits.backward(dy)

    with torch.no_grad():
        x = ops.crop_concat_rows(img, lists.svs, table.detach(), bg, box)
        x = ops.augment_crop(x, None, plan)[0]
        h1 = conv3d_fwd(x, c1.weight, c1.bias, relu=True)
        want = conv3d_fwd(h1.view(*dims, -1), c2.weight, c2.bias, relu=False)
        dz1 = conv3d_bwd_data(dy, c2.weight, dims, h=h1)
        dx_logits = conv3d_bwd_data(dz1, c1.weight[:, 4:].contiguous(), dims)
        if spatial:
            back = ops.spatial_crop_bwd(dx_logits, dims, plan)
            assert not torch.equal(back, ops.flip_crop(dx_logits, dims, plan.flips))
        else:       # today's path: the mirror alone
            back = ops.flip_crop(dx_logits, dims, plan.flips)
        d_table = ops.crop_concat_rows_bwd(back, lists, box, 0)
    assert torch.equal(logits.detach(), want)
    assert torch.equal(table.grad, d_table) and float(d_table.abs().max()) > 0


# ---------------------------------------------------------------- one short epoch of each voxel network
def _augmenter(kind, seed=4):
    from gts.augment import Augmenter

    if kind == "spatial":
        return Augmenter(seed, rotate=20, zoom=0.2, spatial_prob=1)
    if kind == "zero":
        return Augmenter(seed, rotate=0, zoom=0, spatial_prob=1)
    return Augmenter(seed)


def test_refinement_epochs(tmp_path):
    from data_processing.data_loader import ImageGraphDataset, PredLogitDataset
    from model.cnn_model import RefinementModel

    data, logits = str(tmp_path / "data") + os.sep, str(tmp_path / "logits")
    cnn_data.write(data, logits, ("BraTS_a", "BraTS_b"))
    image = ImageGraphDataset(data, "BraTS", read_image=True, read_graph=False, read_label=True)

    def run(kind, evaluate=False, epoch=True):
        torch.manual_seed(2)
        model = RefinementModel(CNN_HP, image, PredLogitDataset(logits), prefetch=False,
                                augmenter=_augmenter(kind) if kind else None)
        before = model.evaluate(image) if evaluate else None
        if epoch:
            assert np.isfinite(model.run_epoch())
        return _state(model.net), before

    first, metrics = run("spatial", evaluate=True)
    again, _ = run("spatial")
    zero, _ = run("zero")
    old, _ = run("old")
    _, plain_metrics = run(None, evaluate=True, epoch=False)
    assert _same(first, again)
    assert not _same(first, zero)
    assert _same(zero, old)
    assert np.array_equal(metrics, plain_metrics)
    assert all(bool(torch.isfinite(w).all()) for w in first.values())


def test_joint_epochs(tmp_path):
    from data_processing.data_loader import ImageGraphDataset
    from model.joint_model import JointModel
    from utils.hyperparam_helpers import FullParamSet

    data = str(tmp_path / "data") + "/"
    write_dataset(data, 2)
    with redirect_stdout(io.StringIO()):
        ds = ImageGraphDataset(data, "BraTS_", read_image=True, read_graph=True, read_label=True)
    gnn_hp = FullParamSet(1, 20, 4, 1e-3, 0.98, 1e-4, [0.1, 1.0, 2.0, 2.0], [64, 64], 0, None, None)
    cnn_hp = FullParamSet(1, 8, 4, 1e-3, 0.98, 1e-4, CNN_HP.class_weights, [16], 0, None, None)

    def run(kind, evaluate=False, epoch=True):
        torch.manual_seed(6)
        model = JointModel("GSpool", gnn_hp, cnn_hp, ds, gnn_loss_weight=0.5,
                           augmenter=_augmenter(kind) if kind else None)
        with redirect_stdout(io.StringIO()):
            before = model.evaluate(ds) if evaluate else None
            if epoch:
                assert np.isfinite(model.run_epoch())
        return _state(model.graph_net), _state(model.conv_net), before

    first, again, zero, old = run("spatial", evaluate=True), run("spatial"), run("zero"), run("old")
    plain = run(None, evaluate=True, epoch=False)
    assert _same(first[0], again[0]) and _same(first[1], again[1])
    assert not _same(first[0], zero[0]) and not _same(first[1], zero[1])
    assert _same(zero[0], old[0]) and _same(zero[1], old[1])
    assert np.array_equal(first[2], plain[2])


# ---------------------------------------------------------------- command lines
def test_refinement_cli_with_rotation_and_zoom(tmp_path, monkeypatch):
    from scripts import train_refinement_cnn as cli
    from utils import hyperparam_helpers as hp_mod

    cnn_data.write(str(tmp_path / "data") + os.sep, str(tmp_path / "logits"), ("BraTS_a", "BraTS_b"))
    real = hp_mod.populate_hardcoded_hyperparameters
    monkeypatch.setattr(cli, "populate_hardcoded_hyperparameters", lambda m: real(m)._replace(n_epochs=1))
    out = tmp_path / "out"
    out.mkdir()
    torch.manual_seed(9)
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["-d", str(tmp_path / "data") + os.sep, "-l", str(tmp_path / "logits"), "-o", str(out), "-r", "run",
                  "-k", "1", "--augment", "--aug_rotate", "15", "--aug_zoom", "0.1"])
    assert "rotation +- 15.0" in log.getvalue() and "zoom 1 +- 0.1" in log.getvalue()
    weights = torch.load(out / "run_f1.pt", map_location="cpu", weights_only=True)
    assert all(bool(torch.isfinite(w).all()) for w in weights.values())


def test_joint_cli_with_rotation_and_zoom(tmp_path, monkeypatch):
    from scripts import train_joint as cli
    from utils import hyperparam_helpers as hp_mod

    data = str(tmp_path / "data") + "/"
    write_dataset(data, 2)
    real = hp_mod.populate_hardcoded_hyperparameters
    monkeypatch.setattr(cli, "populate_hardcoded_hyperparameters", lambda m: real(m)._replace(n_epochs=1))
    out = tmp_path / "out"
    out.mkdir()
    torch.manual_seed(1)
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["-d", data, "-p", "BraTS_", "-o", str(out), "-r", "run", "-k", "1", "--augment", "--aug_rotate", "15",
                  "--aug_zoom", "0.1"])
    assert "rotation +- 15.0" in log.getvalue()
    for name in ("run_f1_gnn.pt", "run_f1_cnn.pt"):
        weights = torch.load(out / name, map_location="cpu", weights_only=True)
        assert all(bool(torch.isfinite(w).all()) for w in weights.values())
