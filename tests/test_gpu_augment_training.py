"""Training under augmentation (gts/augment.py) on the GPU: one step of RefinementModel and of
JointModel on an augmented sample against the same networks in torch CPU float64 on the tests/augment_ref.py
version of that sample, under the bounds tests/test_gpu_refinement.py and tests/test_gpu_dice_training.py hold the
plain step to (loss 1e-5 relative, each gradient tensor within 1e-4 of its largest entry), and the three training
command lines with --augment."""
import io
import os
from collections import namedtuple
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from oracle import graph_ref, torch_ref
from tests import augment_ref, cnn_data
from tests.conv3d_ref import d64
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


def _plan(flips, sigma):
    from gts.augment import AugmentPlan

    return AugmentPlan(flips, [1.08, 0.93, 1.0, 1.05], [-0.07, 0.04, 0.0, 0.09], sigma, 0.0, (42, 0), 5)


def _ce(out, y, class_weights):
    return torch.nn.functional.cross_entropy(out, y, weight=torch.tensor(class_weights, dtype=torch.float64))


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


def test_refinement_step_on_an_augmented_sample_against_fp64(tmp_path):
    from data_processing.data_loader import ImageGraphDataset, PredLogitDataset
    from gts import ops
    from model.cnn_model import RefinementModel

    data, logits = str(tmp_path / "data") + os.sep, str(tmp_path / "logits")
    cnn_data.write(data, logits, ("BraTS_a",))
    image = ImageGraphDataset(data, "BraTS", read_image=True, read_graph=False, read_label=True)
    torch.manual_seed(2)
    model = RefinementModel(CNN_HP, image, PredLogitDataset(logits), prefetch=False)
    x, y = model._cropped(*image[0])
    dims = tuple(x.shape[:3])
    plan = _plan((True, False, True), [0.3, 0.0, 0.0, 0.2])
    ref = _ref_cnn(model.net)
    xa, ya = ops.augment_crop(x.to(DEV), y.to(DEV), plan)
    loss = model.train_step(xa, ya)
    x_ref, y_ref = augment_ref.crop(x.numpy(), y.numpy().reshape(dims), plan)
    assert np.array_equal(ya.cpu().numpy(), y_ref.reshape(-1))
    out = ref(torch.from_numpy(x_ref).movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, 4)
    loss_ref = _ce(out, torch.from_numpy(y_ref.reshape(-1)), CNN_HP.class_weights)
    loss_ref.backward()
    with torch.no_grad():       # the plain sample through the same weights: another loss, so the plan was not dropped
        plain = _ce(ref(x.double().movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, 4), y, CNN_HP.class_weights)
    print(f"loss {float(loss):.8f} fp64 {float(loss_ref.detach()):.8f} (plain sample {float(plain):.8f})")
    assert abs(float(plain) - float(loss_ref.detach())) > 1e-3 * float(loss_ref.detach())
    assert abs(float(loss) - float(loss_ref.detach())) <= 1e-5 * float(loss_ref.detach())
    _assert_grads(model.net, ref)


def test_joint_step_node_logit_gradient_under_a_mirror_against_fp64(tmp_path):
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
    model = JointModel("GSpool", gnn_hp, cnn_hp, ds, gnn_loss_weight=0.0)
    sample = model._to_device(ds, ds[0])
    plan = _plan((True, False, True), [0.0, 0.25, 0.0, 0.0])
    ref_gnn = torch_ref.ref_init_graph_net("GSpool", gnn_hp).double()
    ref_gnn.load_state_dict({k: v.detach().cpu().double() for k, v in model.graph_net.state_dict().items()})
    ref_cnn = _ref_cnn(model.conv_net)
    seen = {}
    hook = model.graph_net.register_forward_hook(
        lambda _m, _i, out: out.register_hook(lambda g: seen.__setitem__("grad", g.detach().clone())) and None)
    with redirect_stdout(io.StringIO()):
        loss = model.train_step(*sample, plan=plan)
    hook.remove()
    box = model.last_box
    mri, graph, feats, _, img, voxel_labels = ds[0]
    svs = np.ascontiguousarray(ds.get_supervoxel_partitioning(mri))
    tg = torch_ref.TGraph(graph_ref.RefGraph(graph.src, graph.dst, graph.n))
    # the float64 pipeline: features mapped per modality, then the input and the labels of the crop mirrored, the
    # image channels mapped and noised
    feats = np.asarray(feats, dtype=np.float32)
    mapped = augment_ref.features_no_noise(feats, [feats.shape[0]], [plan])
    assert not np.array_equal(mapped, feats)
    node_logits = ref_gnn(tg, torch.from_numpy(mapped).double())
    node_logits.retain_grad()
    ids = svs.astype(np.int64)
    rows = np.where(ids < 0, ids + graph.n + 1, ids)
    rows = torch.from_numpy(np.where((rows < 0) | (rows >= graph.n), graph.n, rows))
    voxel = torch.cat([node_logits, torch.tensor(BG, dtype=torch.float64).reshape(1, -1)], dim=0)[rows]
    x = torch.cat([torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).double(), voxel], dim=-1)[box.as_ix()]
    x = torch.flip(x, dims=[ax for ax in range(3) if plan.flips[ax]])
    a = torch.cat([torch.from_numpy(plan.scale).double(), torch.ones(4, dtype=torch.float64)])
    b = torch.cat([torch.from_numpy(plan.shift).double(), torch.zeros(4, dtype=torch.float64)])
    x = x * a + b + torch.from_numpy(augment_ref.crop_noise(box.shape, 8, plan))
    out = ref_cnn(x.movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, 4)
    y = np.ascontiguousarray(voxel_labels).astype(np.int64)[box.as_ix()]
    y = torch.from_numpy(np.ascontiguousarray(augment_ref.flip(y, plan.flips))).reshape(-1)
    loss_ref = _ce(out, y, cnn_hp.class_weights)
    loss_ref.backward()
    print(f"loss {float(loss):.8f} fp64 {float(loss_ref.detach()):.8f} box {box.shape}")
    assert abs(float(loss) - float(loss_ref.detach())) <= 1e-5 * float(loss_ref.detach())
    want = node_logits.grad
    err = (d64(seen["grad"]) - want).abs()
    print(f"d node_logits: max err {err.max():.3e} of {want.abs().max():.3e}")
    assert float(want.abs().max()) > 0 and err.max() <= 1e-4 * want.abs().max()
    _assert_grads(model.conv_net, ref_cnn)


def _train_cnn(tmp_path, monkeypatch, extra, out_dir, seed=9):
    from scripts import train_refinement_cnn as cli
    from utils import hyperparam_helpers as hp_mod

    real = hp_mod.populate_hardcoded_hyperparameters
    monkeypatch.setattr(cli, "populate_hardcoded_hyperparameters", lambda m: real(m)._replace(n_epochs=1))
    out = tmp_path / out_dir
    out.mkdir(exist_ok=True)
    torch.manual_seed(seed)
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["-d", str(tmp_path / "data") + os.sep, "-l", str(tmp_path / "logits"), "-o", str(out), "-r", "run",
                  "-k", "1"] + extra)
    return out, log.getvalue()


def test_refinement_cli_with_augment(tmp_path, monkeypatch):
    cnn_data.write(str(tmp_path / "data") + os.sep, str(tmp_path / "logits"), ("BraTS_a", "BraTS_b"))
    # one run name in several folders: torch.save stores the file's name inside the archive
    plain, plain_log = _train_cnn(tmp_path, monkeypatch, [], "plain")
    off = ["--augment", "--aug_flip_prob", "0", "--aug_scale", "0", "--aug_shift", "0", "--aug_noise", "0"]
    identity, identity_log = _train_cnn(tmp_path, monkeypatch, off, "identity")
    assert "augmentation:" in identity_log and "augmentation:" not in plain_log
    assert (identity / "run_f1.pt").read_bytes() == (plain / "run_f1.pt").read_bytes()
    assert (identity / "run.txt").read_text() == (plain / "run.txt").read_text()
    first, log = _train_cnn(tmp_path, monkeypatch, ["--augment", "--aug_seed", "4"], "first")
    assert log.count("augmentation:") == 1 and "seed 4" in log
    again, _ = _train_cnn(tmp_path, monkeypatch, ["--augment", "--aug_seed", "4"], "again")
    other, _ = _train_cnn(tmp_path, monkeypatch, ["--augment", "--aug_seed", "5"], "other")
    assert (first / "run_f1.pt").read_bytes() == (again / "run_f1.pt").read_bytes()
    assert (first / "run.txt").read_text() == (again / "run.txt").read_text()
    assert (first / "run_f1.pt").read_bytes() != (plain / "run_f1.pt").read_bytes()
    assert (first / "run_f1.pt").read_bytes() != (other / "run_f1.pt").read_bytes()
    weights = torch.load(first / "run_f1.pt", map_location="cpu", weights_only=True)
    assert all(bool(torch.isfinite(w).all()) for w in weights.values())


def _epoch_losses(log):
    lines = log.splitlines()
    return [float(lines[i + 1]) for i, line in enumerate(lines) if line.startswith("____Epoch")]


def test_gnn_cli_with_augment(tmp_path, monkeypatch):
    from scripts import train_gnn as cli
    from utils import hyperparam_helpers as hp_mod

    data = str(tmp_path / "data") + "/"
    write_dataset(data, 4)
    real = hp_mod.populate_hardcoded_hyperparameters
    monkeypatch.setattr(cli, "populate_hardcoded_hyperparameters",
                        lambda m: real(m)._replace(n_epochs=1, layer_sizes=[64, 64]))
    files = {}
    for run, extra in (("a", ["--augment", "--aug_seed", "3"]), ("b", ["--augment", "--aug_seed", "3"]), ("plain", [])):
        out = tmp_path / run
        out.mkdir()
        torch.manual_seed(1)
        log = io.StringIO()
        with redirect_stdout(log):
            cli.main(["-d", data, "-o", str(out), "-r", "run", "-m", "GSpool", "-k", "1", "-p", "BraTS_"] + extra)
        losses = _epoch_losses(log.getvalue())
        assert len(losses) == 1 and np.isfinite(losses[0])
        assert ("augmentation:" in log.getvalue()) == bool(extra)
        files[run] = (out / "run_f1.pt").read_bytes()
    assert files["a"] == files["b"] and files["a"] != files["plain"]


def test_joint_cli_with_augment(tmp_path, monkeypatch):
    from scripts import train_joint as cli
    from utils import hyperparam_helpers as hp_mod

    data = str(tmp_path / "data") + "/"
    write_dataset(data, 2)
    real = hp_mod.populate_hardcoded_hyperparameters
    monkeypatch.setattr(cli, "populate_hardcoded_hyperparameters", lambda m: real(m)._replace(n_epochs=1))
    files = {}
    for run, extra in (("a", ["--augment", "--aug_seed", "3"]), ("b", ["--augment", "--aug_seed", "3"]), ("plain", [])):
        out = tmp_path / run
        out.mkdir()
        torch.manual_seed(1)
        log = io.StringIO()
        with redirect_stdout(log):
            cli.main(["-d", data, "-p", "BraTS_", "-o", str(out), "-r", "run", "-k", "1"] + extra)
        losses = _epoch_losses(log.getvalue())
        assert len(losses) == 1 and np.isfinite(losses[0])
        files[run] = (out / "run_f1_gnn.pt").read_bytes(), (out / "run_f1_cnn.pt").read_bytes()
    assert files["a"] == files["b"]
    assert files["a"][0] != files["plain"][0] and files["a"][1] != files["plain"][1]
