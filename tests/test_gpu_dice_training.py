"""Training on soft Dice + cross-entropy (model/losses.py) on the GPU: one step of RefinementModel and of
JointModel against the same networks in torch CPU float64 with the loss of tests/dice_ref.py, under the bounds
tests/test_gpu_refinement.py holds the composed cross-entropy step to (loss 1e-5 relative, each gradient tensor
within 1e-4 of its largest entry), and scripts/train_refinement_cnn.py with and without --loss."""
import io
import os
from collections import namedtuple
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from oracle import graph_ref, torch_ref
from tests import cnn_data, dice_ref
from tests.conv3d_ref import d64
from tests.dataset_util import write_dataset

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HP = namedtuple("HP", "n_epochs in_feats out_classes lr lr_decay w_decay class_weights layer_sizes")
CNN_HP = HP(1, 8, 4, 1e-3, 0.98, 1e-4, [0.1, 5.0, 15.0, 15.0], [16])
BG = [1.0, -1.0, -1.0, -1.0]
DICE = dict(dice_weight=0.8, smooth=1.0, regions="brats")


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _dice_ce(class_weights):
    from model.losses import make_voxel_loss

    return make_voxel_loss("dice_ce", torch.tensor(class_weights, dtype=torch.float32, device=DEV), **DICE)


def _ref_loss(out, y, class_weights):
    m = dice_ref.membership(dice_ref.region_sets(DICE["regions"], 4), 4)
    w = torch.tensor(class_weights, dtype=torch.float64)
    return dice_ref.loss_terms(out, y, w, m, 1.0, DICE["dice_weight"], DICE["smooth"])[0]


def _ref_cnn(net):
    from model.networks import CnnRefinementNet

    ref = CnnRefinementNet(net.conv_layers[0].in_channels, net.conv_layers[1].out_channels,
                           [net.conv_layers[0].out_channels]).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    return ref


def _assert_grads(net, ref):
    for (name, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        err = (d64(p.grad) - q.grad).abs()
        print(f"  {name}: max err {err.max():.3e} of {q.grad.abs().max():.3e}")
        assert err.max() <= 1e-4 * q.grad.abs().max() + 1e-30, f"{name}: max err {err.max():.3e}"


def test_refinement_step_against_fp64(tmp_path):
    from data_processing.data_loader import ImageGraphDataset, PredLogitDataset
    from model.cnn_model import RefinementModel

    data, logits = str(tmp_path / "data") + os.sep, str(tmp_path / "logits")
    cnn_data.write(data, logits, ("BraTS_a",))
    image = ImageGraphDataset(data, "BraTS", read_image=True, read_graph=False, read_label=True)
    torch.manual_seed(2)
    model = RefinementModel(CNN_HP, image, PredLogitDataset(logits), prefetch=False,
                            voxel_loss=_dice_ce(CNN_HP.class_weights))
    x, y = model._cropped(*image[0])
    ref = _ref_cnn(model.net)
    loss = model.train_step(x.to(DEV), y.to(DEV))
    out = ref(x.double().movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, 4)
    loss_ref = _ref_loss(out, y, CNN_HP.class_weights)
    loss_ref.backward()
    # not the cross-entropy: the Dice term is a sizeable part of what was trained on
    ce_only = float(dice_ref.dice_ce_ref(out, y, torch.tensor(CNN_HP.class_weights), "brats", 1.0, 0.0).loss)
    assert float(loss_ref.detach()) - ce_only > 0.05
    print(f"loss {float(loss):.8f} fp64 {float(loss_ref.detach()):.8f} (cross-entropy alone {ce_only:.8f})")
    assert abs(float(loss) - float(loss_ref.detach())) <= 1e-5 * float(loss_ref.detach())
    _assert_grads(model.net, ref)


def test_joint_step_node_logit_gradient_against_fp64(tmp_path):
    from data_processing.data_loader import ImageGraphDataset
    from model.joint_model import JointModel
    from utils.hyperparam_helpers import FullParamSet

    data = str(tmp_path / "data") + "/"
    write_dataset(data, 1)
    with redirect_stdout(io.StringIO()):
        ds = ImageGraphDataset(data, "BraTS_", read_image=True, read_graph=True, read_label=True)
    gnn_hp = FullParamSet(3, 20, 4, 1e-3, 0.98, 1e-4, [0.1, 1.0, 2.0, 2.0], [64, 64], 0, None, None)
    cnn_hp = FullParamSet(3, 8, 4, 1e-3, 0.98, 1e-4, CNN_HP.class_weights, [16], 0, None, None)
    torch.manual_seed(6)
    # the voxel loss alone: what reaches the node logits is the Dice + CE gradient through both convolutions
    model = JointModel("GSpool", gnn_hp, cnn_hp, ds, gnn_loss_weight=0.0, voxel_loss=_dice_ce(cnn_hp.class_weights))
    sample = model._to_device(ds, ds[0])
    ref_gnn = torch_ref.ref_init_graph_net("GSpool", gnn_hp).double()
    ref_gnn.load_state_dict({k: v.detach().cpu().double() for k, v in model.graph_net.state_dict().items()})
    ref_cnn = _ref_cnn(model.conv_net)
    seen = {}
    hook = model.graph_net.register_forward_hook(
        lambda _m, _i, out: out.register_hook(lambda g: seen.__setitem__("grad", g.detach().clone())) and None)
    with redirect_stdout(io.StringIO()):
        loss = model.train_step(*sample)
    hook.remove()
    box = model.last_box
    mri, graph, feats, _, img, voxel_labels = ds[0]
    svs = np.ascontiguousarray(ds.get_supervoxel_partitioning(mri))
    tg = torch_ref.TGraph(graph_ref.RefGraph(graph.src, graph.dst, graph.n))
    node_logits = ref_gnn(tg, torch.as_tensor(np.asarray(feats)).float().double())
    node_logits.retain_grad()
    ids = svs.astype(np.int64)                      # the row of cat(node_logits, bg) every voxel reads
    rows = np.where(ids < 0, ids + graph.n + 1, ids)
    rows = torch.from_numpy(np.where((rows < 0) | (rows >= graph.n), graph.n, rows))
    voxel = torch.cat([node_logits, torch.tensor(BG, dtype=torch.float64).reshape(1, -1)], dim=0)[rows]
    x = torch.cat([torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).double(), voxel], dim=-1)[box.as_ix()]
    out = ref_cnn(x.movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, 4)
    y = torch.from_numpy(np.ascontiguousarray(voxel_labels).astype(np.int64))[box.as_ix()].reshape(-1)
    loss_ref = _ref_loss(out, y, cnn_hp.class_weights)
    loss_ref.backward()
    print(f"loss {float(loss):.8f} fp64 {float(loss_ref.detach()):.8f} box {box.shape}")
    assert abs(float(loss) - float(loss_ref.detach())) <= 1e-5 * float(loss_ref.detach())
    want = node_logits.grad
    err = (d64(seen["grad"]) - want).abs()
    print(f"d node_logits: max err {err.max():.3e} of {want.abs().max():.3e}")
    assert float(want.abs().max()) > 0 and err.max() <= 1e-4 * want.abs().max()
    _assert_grads(model.conv_net, ref_cnn)


def _train_cli(tmp_path, monkeypatch, run, extra, seed=9, out_dir="out"):
    from scripts import train_refinement_cnn as cli
    from utils import hyperparam_helpers as hp_mod

    real = hp_mod.populate_hardcoded_hyperparameters
    monkeypatch.setattr(cli, "populate_hardcoded_hyperparameters", lambda m: real(m)._replace(n_epochs=1))
    out = tmp_path / out_dir
    out.mkdir(exist_ok=True)
    torch.manual_seed(seed)
    with redirect_stdout(io.StringIO()):
        cli.main(["-d", str(tmp_path / "data") + os.sep, "-l", str(tmp_path / "logits"), "-o", str(out), "-r", run,
                  "-k", "1"] + extra)
    return out


def test_cli_trains_on_dice_ce(tmp_path, monkeypatch):
    cnn_data.write(str(tmp_path / "data") + os.sep, str(tmp_path / "logits"), ("BraTS_a", "BraTS_b"))
    out = _train_cli(tmp_path, monkeypatch, "dice", ["--loss", "dice_ce"])
    assert (out / "dice_f1.pt").exists()
    last = (out / "dice.txt").read_text().splitlines()[-1].split("\t")
    assert last[0] == "dice_full" and np.isfinite(float(last[1])) and float(last[1]) > 0
    # the progress file's loss is the configured one: above the cross-entropy of the same weights by the Dice
    # term, which is no smaller than 0.1 on a network trained for two steps
    from data_processing.data_loader import ImageGraphDataset, PredLogitDataset
    from model.cnn_model import RefinementModel
    from utils.hyperparam_helpers import populate_hardcoded_hyperparameters

    image = ImageGraphDataset(str(tmp_path / "data") + os.sep, "BraTS", read_image=True, read_graph=False,
                              read_label=True)
    model = RefinementModel(populate_hardcoded_hyperparameters("CNN"), None, PredLogitDataset(str(tmp_path / "logits")))
    model.net.load_state_dict(torch.load(out / "dice_f1.pt", map_location=DEV, weights_only=True))
    ce_same_weights = model.evaluate(image)[0]
    print(f"dice_ce {float(last[1]):.4f}, cross-entropy of the same weights {ce_same_weights:.4f}")
    assert float(last[1]) > ce_same_weights + 0.1


def test_cli_default_is_the_cross_entropy_run(tmp_path, monkeypatch):
    cnn_data.write(str(tmp_path / "data") + os.sep, str(tmp_path / "logits"), ("BraTS_a", "BraTS_b"))
    # one run name in two folders: torch.save stores the file's name inside the archive
    flag = _train_cli(tmp_path, monkeypatch, "run", ["--loss", "ce"], out_dir="flag")
    plain = _train_cli(tmp_path, monkeypatch, "run", [], out_dir="plain")
    assert (flag / "run_f1.pt").read_bytes() == (plain / "run_f1.pt").read_bytes()
    assert (flag / "run.txt").read_text() == (plain / "run.txt").read_text()
