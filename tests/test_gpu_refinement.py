"""RefinementModel and scripts/train_refinement_cnn.py on the GPU: HIP logits against MIOpen, step-1
gradients and three epochs of training against torch CPU fp64, evaluate rows against the host metrics,
and the CLI end to end into generate_joint_predictions."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cnn_data
from tests.conv3d_ref import conv, d64, weight_grad

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HP = namedtuple("HP", "n_epochs in_feats out_classes lr lr_decay w_decay class_weights layer_sizes")


def _hp(n_epochs=3):
    return HP(n_epochs, 8, 4, 1e-3, 0.98, 1e-4, [0.1, 5.0, 15.0, 15.0], [16])


def _datasets(tmp_path, ids=("BraTS_a", "BraTS_b", "BraTS_c"), missing=()):
    from data_processing.data_loader import ImageGraphDataset, PredLogitDataset

    data, logits = str(tmp_path / "data") + os.sep, str(tmp_path / "logits")
    cnn_data.write(data, logits, ids, missing_logits=missing)
    image = ImageGraphDataset(data, "BraTS", read_image=True, read_graph=False, read_label=True)
    return image, PredLogitDataset(logits)


def _ref_net(model):
    from model.networks import CnnRefinementNet

    ref = CnnRefinementNet(8, 4, [16]).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in model.net.state_dict().items()})
    return ref


def test_hip_logits_match_miopen_forward(hip_lib):
    from gts.conv3d import refinement_logits
    from model.networks import CnnRefinementNet

    torch.manual_seed(1)
    for cin, cout, dims in ((8, 4, (37, 41, 29)), (9, 5, (64, 64, 64))):
        net = CnnRefinementNet(cin, cout, [16]).to(DEV)
        x = torch.randn(*dims, cin, device=DEV)
        with torch.no_grad():
            mine = refinement_logits(x, net)
            theirs = net(x.movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, cout)
        assert torch.allclose(mine, theirs, rtol=1e-4, atol=1e-4)


def test_step_one_gradients_against_fp64(hip_lib, tmp_path):
    from gts import ops
    from gts.conv3d import refinement_logits
    from model.cnn_model import RefinementModel

    image, logit_ds = _datasets(tmp_path, ids=("BraTS_a",))
    torch.manual_seed(2)
    model = RefinementModel(_hp(), image, logit_ds, prefetch=False)
    mri, img, lab = image[0]
    x, y = model._cropped(mri, img, lab)
    ref = _ref_net(model)
    xd, yd = x.to(DEV), y.to(DEV)
    loss = ops.weighted_cross_entropy(refinement_logits(xd, model.net), yd, model.class_weights)
    model.optimizer.zero_grad()
    loss.backward()
    out = ref(x.double().movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, 4)
    loss_ref = F.cross_entropy(out, y, weight=torch.tensor(_hp().class_weights, dtype=torch.float64))
    loss_ref.backward()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-5 * float(loss_ref.detach())
    # parameter gradients within 1e-4 of each tensor's largest entry: the loss gradient feeding C3-C5 is itself
    # an fp32 softmax (relative rounding ~1e-7 per entry), so the pure-convolution bound of test_gpu_conv3d.py,
    # which checks C3-C5 on exact operands, does not apply to the composed step
    for (name, p), (_, q) in zip(model.net.named_parameters(), ref.named_parameters()):
        err = (d64(p.grad) - q.grad).abs()
        assert err.max() <= 1e-4 * q.grad.abs().max() + 1e-30, f"{name}: max err {err.max():.3e}"


def test_three_epochs_against_fp64_adamw(hip_lib, tmp_path):
    """Three epochs over three samples (in loader order) against the same model in fp64 with torch.optim.AdamW
    and ExponentialLR.  Tolerance 1e-4 relative per epoch loss: the fp32 step differs from fp64 by rounding
    (~1e-6 relative per gradient); Adam divides by sqrt(v), so a parameter whose gradient is near zero can take
    a step of a different size, which nine steps at lr 1e-3 turn into loss changes far below 1e-4."""
    from data_processing.data_loader import collate_refinement_net
    from model.cnn_model import RefinementModel

    image, logit_ds = _datasets(tmp_path)
    torch.manual_seed(3)
    hp = _hp()
    model = RefinementModel(hp, image, logit_ds)
    model.train_loader = torch.utils.data.DataLoader(image, batch_size=1, shuffle=False,
                                                     collate_fn=collate_refinement_net)
    ref = _ref_net(model)
    opt = torch.optim.AdamW(ref.parameters(), lr=hp.lr, weight_decay=hp.w_decay)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, hp.lr_decay)
    w = torch.tensor(hp.class_weights, dtype=torch.float64)
    samples = [model._cropped(*image[i]) for i in range(len(image))]
    for _ in range(hp.n_epochs):
        got = model.run_epoch()
        losses = []
        for x, y in samples:
            out = ref(x.double().movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, 4)
            loss = F.cross_entropy(out, y, weight=w)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        sched.step()
        assert abs(got - np.mean(losses)) <= 1e-4 * np.mean(losses), (got, np.mean(losses))


def test_evaluate_rows_against_host_metrics(hip_lib, tmp_path):
    """Rows against the reference's arithmetic on the host (MIOpen forward, CrossEntropyLoss,
    calculate_brats_metrics on the [1, cx, cy, cz] arrays); a sample without logits is a zero row."""
    from model import evaluation
    from model.cnn_model import RefinementModel

    image, logit_ds = _datasets(tmp_path, missing=("BraTS_c",))
    torch.manual_seed(4)
    model = RefinementModel(_hp(), None, logit_ds)
    got = model.evaluate(image)
    rows = np.zeros((len(image), 7))
    w = model.class_weights.cpu().double()
    ref = _ref_net(model)
    r = 0
    for mri, img, lab in image:
        sample = model._cropped(mri, img, lab)
        if sample is None:
            continue
        x, y = sample
        with torch.no_grad():
            out = ref(x.double().movedim(-1, 0)[None])
        rows[r][0] = float(F.cross_entropy(out[0].movedim(0, -1).reshape(-1, 4), y, weight=w))
        pred = out.argmax(1).numpy()
        rows[r][1:] = evaluation.calculate_brats_metrics(pred, y.numpy().reshape(pred.shape))
        r += 1
    want = rows.mean(axis=0)
    assert r == 2
    assert abs(got[0] - want[0]) <= 1e-5 * want[0]
    assert np.allclose(got[1:], want[1:], rtol=1e-6, atol=0)


def test_cli_end_to_end(hip_lib, tmp_path):
    from gts import graph as ggraph  # noqa: F401  (the package imports)
    from scripts import generate_joint_predictions as gjp
    from scripts import train_refinement_cnn as cli

    image, _ = _datasets(tmp_path, ids=("BraTS_a", "BraTS_b", "BraTS_c", "BraTS_d"))
    out = tmp_path / "out"
    out.mkdir()
    base = ["-d", str(tmp_path / "data") + os.sep, "-l", str(tmp_path / "logits"), "-o", str(out)]
    cli.main(base + ["-r", "full", "-k", "1"])
    cli.main(base + ["-r", "kf", "-k", "2"])
    full = (out / "full.txt").read_text().splitlines()
    assert full[1] == "Model\tCNN" and full[-1].startswith("full_full\t")
    kf = (out / "kf.txt").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in kf[-4:]] == ["kf_f1_train", "kf_f1_val", "kf_f2_train", "kf_f2_val"]
    for name in ("full_f1.pt", "kf_f1.pt", "kf_f2.pt"):
        assert (out / name).exists()
    # the checkpoint drives joint prediction (the GNN side: a freshly initialised network)
    from model.networks import init_graph_net
    from utils.hyperparam_helpers import EvalParamSet

    gnn_hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[64] * 2, gat_heads=None, gat_residuals=None)
    torch.save(init_graph_net("GSpool", gnn_hp).state_dict(), tmp_path / "gnn.pt")
    graph_net, conv_net = gjp.load_nets("GSpool", str(tmp_path / "gnn.pt"), str(out / "full_f1.pt"), gnn_hp=gnn_hp)
    from gts import synth

    import gts

    g = gts.batch([synth.random_graph(n=50, n_pairs=150, seed=5)])
    feats = synth.node_features(g.n, 20, 5)
    svs = np.random.default_rng(5).integers(-1, 50, size=(20, 18, 14)).astype(np.int16)
    img = cnn_data.make(9)[0]
    pred = gjp.predict_one_sample(graph_net, conv_net, g, feats, img, svs)
    assert pred.shape == svs.shape
