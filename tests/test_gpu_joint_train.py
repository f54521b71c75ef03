"""Joint GNN + CNN training on the GPU: J1 / J2 (csrc/gts_joint.hip), conv1's data gradient on the logit
channels, the autograd function, JointModel's step and epochs against torch CPU fp64, and the CLI."""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import graph_ref, joint_ref, torch_ref
from tests.conv3d_ref import d64, data_grad
from tests.dataset_util import write_dataset

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BG = [1.0, -1.0, -1.0, -1.0]
U = 2.0 ** -24                   # unit roundoff of fp32


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _mask_box(shape, seed, p=0.6):
    from gts import ops

    rng = np.random.default_rng(seed)
    idx = [np.flatnonzero(rng.random(n) < p) for n in shape]
    idx = [i if len(i) else np.array([0]) for i in idx]
    return ops.CropBox(*idx, shape, DEV)


def _whole_box(shape):
    from gts import ops

    return ops.CropBox(*[np.arange(n) for n in shape], shape, DEV)


def _one_voxel_box(shape):
    from gts import ops

    return ops.CropBox([shape[0] - 1], [shape[1] // 2], [0], shape, DEV)


def _partitioning(shape, n_rows, seed):
    """Random ids: below -1 (numpy wraps them), -1 (background), past the table, and every row in between."""
    rng = np.random.default_rng(seed)
    svs = rng.integers(-n_rows - 3, n_rows + 3, size=shape).astype(np.int16)
    svs[rng.random(shape) < 0.3] = -1
    return svs


def _resolved_rows(svs, n_rows):
    """Row of cat(table, bg) every voxel reads: n_rows is the background row."""
    ids = svs.astype(np.int64)
    rows = np.where(ids < 0, ids + n_rows + 1, ids)
    return np.where((rows < 0) | (rows >= n_rows), n_rows, rows)


# ------------------------------------------------------------------------------------------- 1. J1
@pytest.mark.parametrize("ci,ct", [(4, 4), (5, 3)])
def test_j1_equals_k16_transposed(ci, ct):
    from gts import ops

    shape, n_rows = (19, 14, 23), 41
    rng = np.random.default_rng(ci * 10 + ct)
    svs = torch.from_numpy(_partitioning(shape, n_rows, ci)).to(DEV)
    table = torch.from_numpy(rng.standard_normal((n_rows, ct)).astype(np.float32)).to(DEV)
    bg = torch.from_numpy(rng.standard_normal(ct).astype(np.float32)).to(DEV)
    img = torch.from_numpy(rng.standard_normal(shape + (ci,)).astype(np.float32)).to(DEV)
    for box in (_mask_box(shape, 3), _mask_box(shape, 4, p=0.3), _whole_box(shape), _one_voxel_box(shape)):
        got = ops.crop_concat_rows(img, svs, table, bg, box)
        want = ops.crop_concat(img, svs, table, bg, box)[0].movedim(0, -1)
        assert got.shape == (*box.shape, ci + ct) and got.is_contiguous()
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------- 2. J2
def _check_j2(svs, n_rows, box, ci, ct, seed):
    """J2 against index_add_ in fp64.  A fixed-order fp32 sum of k terms lies within (k - 1) u sum|x_i| of the
    exact sum (u = 2^-24); twice that is allowed, for a tree whose partial sums are themselves rounded."""
    from gts import ops

    torch.manual_seed(seed)
    v = int(np.prod(box.shape))
    lists = ops.SupervoxelLists(svs, n_rows, DEV)
    dx = torch.randn(v, ci + ct, device=DEV)
    got = ops.crop_concat_rows_bwd(dx, lists, box, ci)
    assert got.shape == (n_rows, ct)
    rows = torch.from_numpy(_resolved_rows(svs, n_rows)[box.as_ix()].reshape(-1))
    g64 = d64(dx)[:, ci:]
    want = torch.zeros(n_rows + 1, ct, dtype=torch.float64).index_add_(0, rows, g64)[:n_rows]
    sum_abs = torch.zeros(n_rows + 1, ct, dtype=torch.float64).index_add_(0, rows, g64.abs())[:n_rows]
    k = torch.bincount(rows, minlength=n_rows + 1)[:n_rows].double()
    bound = 2.0 * (k - 1).clamp(min=0)[:, None] * U * sum_abs
    err = (d64(got) - want).abs()
    print(f"J2 {tuple(box.shape)} n={n_rows}: max err {err.max():.3e}, max bound {bound.max():.3e}, "
          f"largest list in the box {int(k.max())}, empty nodes {int((k == 0).sum())}")
    assert torch.all(err <= bound), f"max excess {(err - bound).max():.3e}"
    empty = (k == 0).to(DEV)
    assert torch.all(got[empty] == 0.0) and not torch.any(torch.signbit(got[empty]))
    # two runs: identical bits
    assert torch.equal(got, ops.crop_concat_rows_bwd(dx, lists, box, ci))
    # background voxels and the image columns change nothing
    other = dx.clone()
    other[(rows == n_rows).to(DEV)] += 3.0
    other[:, :ci] -= 5.0
    assert torch.equal(got, ops.crop_concat_rows_bwd(other, lists, box, ci))
    return lists, dx, got, bound


@pytest.mark.parametrize("ci,ct", [(0, 4), (4, 4), (5, 3), (0, 1)])
def test_j2_against_fp64_index_add(ci, ct):
    from gts import ops

    shape, n_rows = (13, 11, 17), 23
    svs = _partitioning(shape, n_rows, seed=ci + ct)
    svs[(svs == 5) | (svs == 5 - (n_rows + 1))] = -1              # row 5 has no voxel anywhere
    for i, box in enumerate((_mask_box(shape, 7), _mask_box(shape, 8, p=0.25), _whole_box(shape),
                             _one_voxel_box(shape))):
        lists, dx, got, bound = _check_j2(svs, n_rows, box, ci, ct, seed=i)
        assert not got[5].any()
        if ci == 0:
            continue
        # <J1(T) - J1(0), G> = <T, J2(G)>: J1 is affine in T (the background row is a constant)
        img = torch.randn(*shape, ci, device=DEV)
        table = torch.randn(n_rows, ct, device=DEV)
        bg = torch.randn(ct, device=DEV)
        svs_d = torch.from_numpy(svs).to(DEV)
        moved = d64(ops.crop_concat_rows(img, svs_d, table, bg, box)) \
            - d64(ops.crop_concat_rows(img, svs_d, torch.zeros_like(table), bg, box))
        lhs = (moved.reshape(-1, ci + ct) * d64(dx)).sum()
        rhs = (d64(table) * d64(got)).sum()
        assert abs(lhs - rhs) <= (d64(table).abs() * bound).sum() + 1e-12 * abs(lhs)


def test_j2_at_brats_proportions():
    """The whole-brain crop of a synthetic BraTS-size scan (gts.synth_mri: between 144 x 144 x 93 and
    180 x 180 x 116; 148 x 162 x 107 for this seed) with the graph generator's SLIC partition: 5 467 supervoxels are
    left of the 13 500 asked for once those outside the brain are dropped (the generator is deterministic; the
    range below leaves room for a change of its tie rules, not for another order of magnitude)."""
    from data_processing.image_processing import determine_brain_crop, normalize_img, standardize_img
    from gts import graphgen, synth_mri
    from scripts.preprocess_dataset import STANDARDIZATION_STATS

    img, _ = synth_mri.make_sample(11)
    crop = determine_brain_crop(img)
    data = standardize_img(normalize_img(img[crop]), np.float32(STANDARDIZATION_STATS[0]),
                           np.float32(STANDARDIZATION_STATS[1]))
    res = graphgen.build_graph(data, None, 13500, 0.5, 0)
    svs, n_rows = np.ascontiguousarray(res["partition"]), int(res["feats"].shape[0])
    print(f"volume {svs.shape}, {n_rows} nodes")
    assert svs.dtype == np.int16 and 5000 <= n_rows <= 6000 and svs.size > 2_500_000
    _check_j2(svs, n_rows, _whole_box(svs.shape), 0, 4, seed=1)
    _check_j2(svs, n_rows, _mask_box(svs.shape, 2, p=0.5), 4, 4, seed=2)


# ------------------------------------------------------------------------------------------- 3. conv1 data gradient
@pytest.mark.parametrize("ci,ct,dims", [(4, 4, (9, 7, 21)), (5, 3, (4, 18, 5)), (4, 4, (1, 1, 1))])
def test_conv1_data_gradient_on_the_logit_channels(ci, ct, dims):
    """C3 with the contiguous slice w1[:, Ci:]: against fp64 under the pure-kernel bound of test_gpu_conv3d.py, and
    the same bits as the [:, Ci:] columns of the full data gradient (both routes run the same kernel: a column
    of the implicit GEMM does not depend on its neighbours)."""
    from gts import conv3d

    torch.manual_seed(ci + ct + sum(dims))
    cmid, v = 16, dims[0] * dims[1] * dims[2]
    w1 = torch.randn(cmid, ci + ct, 5, 5, 5) * 0.1
    dz1 = torch.randn(v, cmid)
    sliced = w1[:, ci:].contiguous()
    got = conv3d.conv3d_bwd_data(dz1.to(DEV), sliced.to(DEV), dims)
    want = data_grad(dz1.double(), sliced.double(), dims)
    bound = data_grad(dz1.double().abs(), sliced.double().abs(), dims)
    err = (d64(got) - want).abs()
    print(f"conv1 logit-channel data gradient {dims}: max err {err.max():.3e}, bound {2e-6 * bound.max():.3e}")
    assert got.shape == (v, ct) and torch.all(err <= 2e-6 * bound + 1e-30)
    full = conv3d.conv3d_bwd_data(dz1.to(DEV), w1.to(DEV), dims)
    assert torch.equal(got, full[:, ci:])


# ------------------------------------------------------------------------------------------- 4. autograd function
def _ref_voxel_logits(table, bg, rows, img, box_ix, cnn):
    """cat(node_logits, bg)[svs][box] ++ image -> RefCnnRefinementNet -> [V, Cout], on torch CPU tensors."""
    voxel = torch.cat([table, bg.reshape(1, -1)], dim=0)[rows]
    x = joint_ref.combine_logits_and_image_ref(voxel, img, box_ix)
    return cnn(x)[0].movedim(0, -1).reshape(-1, cnn.conv_layers[1].out_channels)


def _ref_cnn(net, dtype):
    ref = joint_ref.RefCnnRefinementNet(net.conv_layers[0].in_channels, net.conv_layers[1].out_channels,
                                        [net.conv_layers[0].out_channels]).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()})
    return ref


def _assert_cnn_grads(net, ref):
    for (name, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        err = (d64(p.grad) - q.grad.double()).abs()
        print(f"  {name}: max err {err.max():.3e} of {q.grad.abs().max():.3e}")
        assert err.max() <= 1e-4 * q.grad.abs().max() + 1e-30, f"{name}: max err {err.max():.3e}"


def test_autograd_function_against_fp64():
    from gts import ops
    from gts.joint import joint_refinement_logits
    from model.networks import CnnRefinementNet

    torch.manual_seed(5)
    shape, n_rows, pad = (14, 12, 10), 30, 5
    svs = _partitioning(shape, n_rows, seed=9)
    box = _mask_box(shape, 5, p=0.7)
    net = CnnRefinementNet(8, 4, [16]).to(DEV)
    big = torch.randn(n_rows + 9, 4, requires_grad=True)
    img = torch.randn(*shape, 4)
    y = torch.randint(0, 4, (int(np.prod(box.shape)),))
    w = torch.tensor([0.1, 5.0, 15.0, 15.0])
    big_d = big.detach().to(DEV).requires_grad_(True)
    logits = joint_refinement_logits(big_d[pad:pad + n_rows], img.to(DEV), torch.from_numpy(svs).to(DEV), box,
                                     torch.tensor(BG, device=DEV), net)
    loss = ops.weighted_cross_entropy(logits, y.to(DEV), w.to(DEV))
    loss.backward()
    ref = _ref_cnn(net, torch.float64)
    big64 = big.detach().double().requires_grad_(True)
    rows = torch.from_numpy(_resolved_rows(svs, n_rows))
    out = _ref_voxel_logits(big64[pad:pad + n_rows], torch.tensor(BG, dtype=torch.float64), rows, img.double(),
                            box.as_ix(), ref)
    loss_ref = F.cross_entropy(out, y, weight=w.double())
    loss_ref.backward()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-5 * float(loss_ref.detach())
    err = (d64(big_d.grad) - big64.grad).abs()
    print(f"d node_logits: max err {err.max():.3e} of {big64.grad.abs().max():.3e}")
    assert err.max() <= 1e-4 * big64.grad.abs().max()
    outside = torch.ones(n_rows + 9, dtype=torch.bool)
    outside[pad:pad + n_rows] = False
    assert not big_d.grad[outside.to(DEV)].any() and big_d.grad[pad:pad + n_rows].abs().max() > 0
    _assert_cnn_grads(net, ref)


# ------------------------------------------------------------------------------------------- 5-7. JointModel
def _hps(gnn_layers=(64, 64)):
    from utils.hyperparam_helpers import FullParamSet

    gnn = FullParamSet(3, 20, 4, 1e-3, 0.98, 1e-4, [0.1, 1.0, 2.0, 2.0], list(gnn_layers), 0, None, None)
    cnn = FullParamSet(3, 8, 4, 1e-3, 0.98, 1e-4, [0.1, 5.0, 15.0, 15.0], [16], 0, None, None)
    return gnn, cnn


def _dataset(tmp_path, n):
    from data_processing.data_loader import ImageGraphDataset

    data = str(tmp_path / "data") + "/"
    write_dataset(data, n)
    with redirect_stdout(io.StringIO()):
        return ImageGraphDataset(data, "BraTS_", read_image=True, read_graph=True, read_label=True)


def _leave_k_tumour_nodes(model, samples, k=2):
    """Shift the class-0 bias of the graph network's last layer so that, on the first of `samples`, exactly the k
    nodes with the largest tumour margin stay tumour: the crop around them is then a proper sub-box (a freshly
    initialised network calls nearly every node tumour, and the crop would be the whole volume)."""
    with torch.no_grad():
        logits = model.graph_net(samples[0][0], samples[0][1])
        margin = torch.sort(logits[:, 1:].max(dim=1).values - logits[:, 0], descending=True).values
        model.graph_net.layers[-1].bias[0] += 0.5 * (margin[k - 1] + margin[k])


def _gnn_grads(model):
    """Gradients of the last step by parameter name: from the fused stack's flat buffer, or from .grad."""
    sink = model.grad_sink
    out = {}
    for name, p in model.graph_net.named_parameters():
        if sink.filled:
            at = sink.offsets[id(p)]
            out[name] = sink.flat[at:at + p.numel()].view_as(p).detach().cpu().double()
        else:
            out[name] = p.grad.detach().cpu().double()
    return out


class _RefPair:
    """The same two networks on the CPU in `dtype`, from the model's weights as they are now."""

    def __init__(self, model, gnn_type, gnn_hp, dtype):
        self.dtype = dtype
        self.gnn = torch_ref.ref_init_graph_net(gnn_type, gnn_hp).to(dtype)
        self.gnn.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in model.graph_net.state_dict().items()})
        self.cnn = _ref_cnn(model.conv_net, dtype)
        self.w_gnn = model.gnn_class_weights.cpu().to(dtype)
        self.w_cnn = model.cnn_class_weights.cpu().to(dtype)

    def loss(self, host, box, gnn_loss_weight):
        """Total loss of one sample for the crop `box` (the one the model reports)."""
        graph, feats, node_labels, img, svs, voxel_labels = host
        tg = torch_ref.TGraph(graph_ref.RefGraph(graph.src, graph.dst, graph.n))
        # the features as the model uploads them: rounded to fp32 once
        node_logits = self.gnn(tg, torch.as_tensor(np.asarray(feats)).float().to(self.dtype))
        rows = torch.from_numpy(_resolved_rows(svs, graph.n))
        out = _ref_voxel_logits(node_logits, torch.tensor(BG, dtype=self.dtype), rows,
                                torch.from_numpy(img).to(self.dtype), box.as_ix(), self.cnn)
        y = torch.from_numpy(voxel_labels.astype(np.int64))[box.as_ix()].reshape(-1)
        loss = F.cross_entropy(out, y, weight=self.w_cnn)
        if gnn_loss_weight:
            loss = loss + gnn_loss_weight * F.cross_entropy(
                node_logits, torch.from_numpy(np.asarray(node_labels).astype(np.int64)), weight=self.w_gnn)
        return loss


def _host_sample(ds, i):
    mri, graph, feats, node_labels, img, voxel_labels = ds[i]
    svs = np.ascontiguousarray(ds.get_supervoxel_partitioning(mri))
    return graph, feats, node_labels, np.ascontiguousarray(img, dtype=np.float32), svs, np.ascontiguousarray(voxel_labels)


@pytest.mark.parametrize("gnn_type", ["GSpool", "GSmean"])
@pytest.mark.parametrize("gnn_loss_weight", [1.0, 0.0])
def test_step_one_gradients_against_fp64(tmp_path, gnn_type, gnn_loss_weight):
    from model.joint_model import JointModel

    ds = _dataset(tmp_path, 1)
    gnn_hp, cnn_hp = _hps()
    torch.manual_seed(6)
    model = JointModel(gnn_type, gnn_hp, cnn_hp, ds, gnn_loss_weight=gnn_loss_weight)
    dev_sample = model._to_device(ds, ds[0])
    _leave_k_tumour_nodes(model, [dev_sample])
    ref64 = _RefPair(model, gnn_type, gnn_hp, torch.float64)
    ref32 = _RefPair(model, gnn_type, gnn_hp, torch.float32)
    with redirect_stdout(io.StringIO()):
        loss = model.train_step(*dev_sample)
    box, host = model.last_box, _host_sample(ds, 0)
    # the reported box is the reference's crop of the model's own node predictions, and a proper sub-box
    preds = graph_ref.project_nodes_to_img_ref(host[4], model.last_node_logits.argmax(1).cpu().numpy())
    with redirect_stdout(io.StringIO()):
        want_crop = joint_ref.determine_tumor_crop_ref(preds)
    assert all(np.array_equal(a.reshape(-1), b) for a, b in zip(want_crop, box.host))
    assert 0 < np.prod(box.shape) < host[4].size
    loss64 = ref64.loss(host, box, gnn_loss_weight)
    loss64.backward()
    ref32.loss(host, box, gnn_loss_weight).backward()
    assert abs(float(loss) - float(loss64.detach())) <= 1e-5 * float(loss64.detach())
    _assert_cnn_grads(model.conv_net, ref64.cnn)
    mine = _gnn_grads(model)
    for (name, q32), (_, q64) in zip(ref32.gnn.named_parameters(), ref64.gnn.named_parameters()):
        s = max(float(q64.grad.abs().max()), 1e-6)
        e_gpu = float((mine[name] - q64.grad).abs().max())
        e_cpu = float((q32.grad.double() - q64.grad).abs().max())
        print(f"  {name}: gpu {e_gpu:.3e} cpu32 {e_cpu:.3e} scale {s:.3e}")
        assert e_gpu < max(10 * e_cpu, 1e-3 * s), f"{name}: gpu {e_gpu:.3e} cpu {e_cpu:.3e} scale {s:.3e}"
        assert e_gpu < 1e-2 * s, f"{name}: {e_gpu:.3e} vs scale {s:.3e}"
        if not gnn_loss_weight:           # the voxel loss alone reaches the graph network through J2
            assert float(q64.grad.abs().max()) > 0 and float(mine[name].abs().max()) > 0


def test_three_epochs_against_fp64_adamw(tmp_path):
    """Three epochs over three samples in loader order against the same pair in fp64 with two torch.optim.AdamW and
    two ExponentialLR, the fp64 side taking the boxes the model reports; epoch loss within 1e-4 relative (the
    figure and the argument of test_gpu_refinement.py::test_three_epochs_against_fp64_adamw)."""
    from model.joint_model import JointModel, _first

    ds = _dataset(tmp_path, 3)
    gnn_hp, cnn_hp = _hps()
    torch.manual_seed(7)
    model = JointModel("GSpool", gnn_hp, cnn_hp, ds)
    model.train_loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, collate_fn=_first)
    _leave_k_tumour_nodes(model, [model._to_device(ds, ds[0])])
    ref = _RefPair(model, "GSpool", gnn_hp, torch.float64)
    opts = [torch.optim.AdamW(net.parameters(), lr=hp.lr, weight_decay=hp.w_decay)
            for net, hp in ((ref.gnn, gnn_hp), (ref.cnn, cnn_hp))]
    scheds = [torch.optim.lr_scheduler.ExponentialLR(o, hp.lr_decay) for o, hp in zip(opts, (gnn_hp, cnn_hp))]
    boxes, step = [], model.train_step

    def recording_step(*args):
        out = step(*args)
        boxes.append(model.last_box)
        return out

    model.train_step = recording_step
    hosts = [_host_sample(ds, i) for i in range(len(ds))]
    for epoch in range(gnn_hp.n_epochs):
        del boxes[:]
        with redirect_stdout(io.StringIO()):
            got = model.run_epoch()
        losses = []
        for host, box in zip(hosts, boxes):
            loss = ref.loss(host, box, 1.0)
            for o in opts:
                o.zero_grad()
            loss.backward()
            for o in opts:
                o.step()
            losses.append(float(loss))
        for s in scheds:
            s.step()
        print(f"epoch {epoch}: gpu {got:.8f} fp64 {np.mean(losses):.8f} boxes {[b.shape for b in boxes]}")
        assert abs(got - np.mean(losses)) <= 1e-4 * np.mean(losses), (got, np.mean(losses))


def test_no_predicted_tumour_trains_on_the_whole_volume(tmp_path):
    from model.joint_model import JointModel

    ds = _dataset(tmp_path, 1)
    torch.manual_seed(8)
    model = JointModel("GSpool", *_hps(), ds)
    with torch.no_grad():
        model.graph_net.layers[-1].bias[0] += 1e3
    log = io.StringIO()
    with redirect_stdout(log):
        loss = model.train_step(*model._to_device(ds, ds[0]))
    assert "No GNN predicted tumor" in log.getvalue()
    assert model.last_box.shape == model.last_box.volume_shape and np.isfinite(float(loss))


# ------------------------------------------------------------------------------------------- 8. CLI
def test_cli_end_to_end(tmp_path, monkeypatch):
    from data_processing.data_loader import ImageGraphDataset
    from model.joint_model import JointModel
    from scripts import generate_joint_predictions as gjp
    from scripts import train_joint as cli
    from torch.utils.data import Subset
    from utils import hyperparam_helpers as hp_mod

    data = str(tmp_path / "data") + "/"
    write_dataset(data, 4)
    out = tmp_path / "out"
    out.mkdir()
    real = hp_mod.populate_hardcoded_hyperparameters
    monkeypatch.setattr(cli, "populate_hardcoded_hyperparameters", lambda m: real(m)._replace(n_epochs=2))
    base = ["-d", data, "-p", "BraTS_", "-o", str(out)]
    with redirect_stdout(io.StringIO()):
        cli.main(base + ["-r", "full", "-k", "1"])
        cli.main(base + ["-r", "kf", "-k", "2", "-w", "0.5"])
    full = (out / "full.txt").read_text().splitlines()
    assert full[1] == "Model\tGSpool" and full[-1].startswith("full_full\t")
    kf = (out / "kf.txt").read_text().splitlines()
    rows = [ln.split("\t") for ln in kf[-4:]]
    assert [r[0] for r in rows] == ["kf_f1_train", "kf_f1_val", "kf_f2_train", "kf_f2_val"]
    assert all(len(r) == 5 and np.isfinite(float(r[1])) for r in rows)
    for name in ("full_f1", "kf_f1", "kf_f2"):
        assert (out / f"{name}_gnn.pt").exists() and (out / f"{name}_cnn.pt").exists()
    # the pair drives joint prediction unchanged
    graph_net, conv_net = gjp.load_nets("GSpool", str(out / "full_f1_gnn.pt"), str(out / "full_f1_cnn.pt"))
    with redirect_stdout(io.StringIO()):
        ds = ImageGraphDataset(data, "BraTS_", read_image=True, read_graph=True, read_label=False)
        mri, graph, feats, img = ds[0]
        svs = ds.get_supervoxel_partitioning(mri)
        pred = gjp.predict_one_sample(graph_net, conv_net, graph, feats, img, svs)
    assert pred.shape == svs.shape and pred.dtype == np.int16
    # started from that pair on one sample with -w 0, the first step's loss is the voxel cross-entropy that
    # evaluate reports on those weights before any update
    single = str(tmp_path / "single") + "/"
    write_dataset(single, 1)
    start = ["-g", str(out / "full_f1_gnn.pt"), "-c", str(out / "full_f1_cnn.pt")]
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["-d", single, "-p", "BraTS_", "-o", str(out), "-r", "tuned", "-k", "1", "-w", "0"] + start)
        one = ImageGraphDataset(single, "BraTS_", read_image=True, read_graph=True, read_label=True)
        model = JointModel("GSpool", real("GSpool"), real("CNN"), one, gnn_loss_weight=0.0,
                           gnn_weights=start[1], cnn_weights=start[3])
        before = model.evaluate(Subset(one, range(1)))[0]
    lines = log.getvalue().splitlines()
    first_epoch_loss = float(lines[lines.index("____Epoch 1_____") + 1])
    assert abs(first_epoch_loss - before) <= 1e-5 * before, (first_epoch_loss, before)
    assert (out / "tuned_f1_gnn.pt").exists() and (out / "tuned_f1_cnn.pt").exists()
