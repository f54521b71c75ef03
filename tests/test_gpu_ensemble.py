"""Ensemble prediction on the MI355X: E1 (softmax_accumulate) against float64 and against itself bit for bit, E2
(argmax_scatter_rows) bit-exact, the mirrored weights on the HIP convolutions against mirrored data, the whole
predictor against tests/ensemble_ref.py, and the command lines."""
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from gts import ops
from tests import ensemble_ref as R
from tests.dataset_util import write_dataset
from tests.test_gpu_joint import _box, _nets

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gnn-tumor-seg_amd")
ROWS = (1, 3, 63, 64, 65, 257, 4099)
SETS = (1, 2, 8, 9, 17)
MASKS = [tuple(bool(m >> a & 1) for a in range(3)) for m in range(8)]
# |mean probability - float64|: a few fp32 ulp per softmax value <= 1 plus half an ulp per add
E1_BOUND = 2e-6


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _logit_sets(rows, classes, n_sets, seed):
    """Random logits with planted rows: +-80 and +-100 (exp overflows fp32 without the max subtraction) and rows
    whose logits are all equal."""
    rng = np.random.default_rng(seed)
    sets = []
    for s in range(n_sets):
        x = (4.0 * rng.standard_normal((rows, classes))).astype(np.float32)
        big = np.arange(s % 3, rows, 3)
        x[big] = rng.choice(np.array([-80.0, 80.0], dtype=np.float32), size=(len(big), classes))
        x[big[1::2]] *= 1.25
        x[np.arange((s + 1) % 7, rows, 7)] = np.float32(rng.standard_normal())
        sets.append(x)
    return sets


def _dev(sets):
    return [torch.from_numpy(s).to(DEV) for s in sets]


# ------------------------------------------------------------------------------------------------ E1
@pytest.mark.parametrize("classes", [4, 1, 3, 5])
def test_softmax_accumulate_against_float64(classes):
    for rows in ROWS:
        for n_sets in SETS:
            sets = _logit_sets(rows, classes, n_sets, seed=rows * 100 + n_sets * 10 + classes)
            acc = ops.softmax_accumulate(_dev(sets))
            assert acc.shape == (rows, classes) and acc.dtype == torch.float32
            got = acc.cpu().numpy().astype(np.float64) / n_sets
            err = float(np.abs(got - R.mean_softmax(sets)).max())
            print(f"E1 rows {rows} classes {classes} sets {n_sets}: max |mean - float64| {err:.3e}")
            assert np.isfinite(got).all() and err <= E1_BOUND, (rows, classes, n_sets, err)


def test_softmax_accumulate_labels_of_24_random_softmaxes():
    """Arg-max of the accumulated sum against float64 wherever the float64 margin exceeds 1e-5; near-ties measured on
    the CPU for means of 24 random softmaxes are 0.0135 % of the rows, so at most 0.1 % may be left out."""
    rng = np.random.default_rng(24)
    sets = [(2.0 * rng.standard_normal((4099, 4))).astype(np.float32) for _ in range(24)]
    want = R.mean_softmax(sets)
    clear = R.top_two_margin(want) > 1e-5
    got = ops.softmax_accumulate(_dev(sets)).cpu().numpy()
    print(f"E1 labels: {int((~clear).sum())} of {len(clear)} rows below the margin")
    assert (~clear).mean() <= 1e-3
    assert np.array_equal(got.argmax(axis=1)[clear], want.argmax(axis=1)[clear])
    assert float(np.abs(got.astype(np.float64) / 24 - want).max()) <= E1_BOUND


@pytest.mark.parametrize("rows,classes", [(4099, 4), (257, 3), (65, 5), (1, 4)])
def test_softmax_accumulate_grouping_changes_no_bit(rows, classes):
    sets = _dev(_logit_sets(rows, classes, 17, seed=rows + classes))
    whole = ops.softmax_accumulate(sets)
    assert torch.equal(whole, ops.softmax_accumulate(sets))                            # two runs
    split = ops.softmax_accumulate(sets[:8])
    assert ops.softmax_accumulate(sets[8:16], split) is split
    ops.softmax_accumulate(sets[16:], split)
    assert torch.equal(whole, split)                                                   # 8 + 8 + 1
    single = ops.softmax_accumulate(sets[:1])
    for s in sets[1:]:
        ops.softmax_accumulate([s], single)
    assert torch.equal(whole, single)                                                  # one at a time
    uneven = ops.softmax_accumulate(sets[:3])
    ops.softmax_accumulate(sets[3:14], uneven)
    ops.softmax_accumulate(sets[14:], uneven)
    assert torch.equal(whole, uneven)                                                  # 3 + 11 + 3
    onto_zeros = ops.softmax_accumulate(sets, torch.zeros(rows, classes, device=DEV))
    assert torch.equal(whole, onto_zeros)                                              # overwrite == add onto zeros
    for s in sets:                                                                     # the inputs are only read
        assert torch.isfinite(s).all()


@pytest.mark.parametrize("rows", [1, 65, 4099])
def test_softmax_accumulate_wide_rows_equal_the_generic_loop(rows):
    """Four classes take 16-byte loads when every pointer is 16-byte aligned; a set that starts 4 bytes into its
    buffer sends the same call through the per-class loop.  Same bits."""
    sets = _dev(_logit_sets(rows, 4, 9, seed=rows))
    wide = ops.softmax_accumulate(sets)
    shifted = torch.empty(rows * 4 + 1, device=DEV)[1:].view(rows, 4)
    shifted.copy_(sets[0])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert torch.equal(wide, ops.softmax_accumulate([shifted] + sets[1:]))


def test_softmax_accumulate_tied_mean():
    """The hand-computed case of tests/test_ensemble_host.py on the kernels: both columns of the sum are the same two
    numbers added, so E2's first maximum is class 0."""
    a = torch.tensor([[np.log(3.0), 0.0]], dtype=torch.float32, device=DEV)
    b = torch.tensor([[0.0, np.log(3.0)]], dtype=torch.float32, device=DEV)
    total = ops.softmax_accumulate([a, b])
    assert float(total[0, 0]) == float(total[0, 1]) and abs(float(total[0, 0]) - 1.0) < 1e-6
    box = ops.CropBox([1], [0], [2], (2, 1, 3), DEV)
    relabel = torch.tensor([7, 9], dtype=torch.int16, device=DEV)
    out = ops.argmax_scatter_rows(total, box, relabel).cpu().numpy()
    assert out[1, 0, 2] == 7 and np.count_nonzero(out) == 1


# ------------------------------------------------------------------------------------------------ E2
@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("classes", [4, 3, 5])
@pytest.mark.parametrize("shape", [(18, 15, 13), (1, 1, 1), (5, 64, 3)])
def test_argmax_scatter_rows_bit_exact(shape, classes, relabel):
    box = _box(shape, seed=sum(shape))
    assert box.shape != shape or shape == (1, 1, 1)                                    # a non-contiguous box
    rng = np.random.default_rng(classes + sum(shape))
    scores = rng.integers(-2, 3, size=(*box.shape, classes)).astype(np.float32)        # duplicate maxima everywhere
    scores.reshape(-1, classes)[::5] = scores.reshape(-1, classes)[::5].max(axis=1, keepdims=True)   # all tied
    table = np.array([0, 2, 1, 4, 3], dtype=np.int16)[:classes]
    dev_table = torch.from_numpy(table).to(DEV) if relabel else None
    dev_scores = torch.from_numpy(scores).to(DEV)
    got = ops.argmax_scatter_rows(dev_scores.view(-1, classes), box, dev_table)
    labels = scores.argmax(axis=-1)                                                    # numpy: first maximum
    want = np.zeros(shape, dtype=np.int16)
    want[box.as_ix()] = table[labels] if relabel else labels
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, ops.argmax_scatter_rows(dev_scores, box, dev_table))       # [cx, cy, cz, C] as well
    k17 = ops.argmax_scatter(dev_scores.movedim(-1, 0).contiguous(), box, dev_table)
    assert torch.equal(got, k17)


def test_argmax_scatter_rows_unaligned_scores():
    shape = (9, 8, 7)
    box = _box(shape, seed=5)
    rows = box.shape[0] * box.shape[1] * box.shape[2]
    scores = torch.randn(rows, 4, device=DEV)
    shifted = torch.empty(rows * 4 + 1, device=DEV)[1:].view(rows, 4)
    shifted.copy_(scores)
    assert torch.equal(ops.argmax_scatter_rows(scores, box), ops.argmax_scatter_rows(shifted, box))


# ------------------------------------------------------------------------------------------------ mirrored weights
@pytest.mark.parametrize("dims", [(7, 5, 9), (12, 6, 5)])
def test_mirrored_weights_on_the_hip_convolutions(dims):
    from gts.conv3d import conv3d_fwd
    from gts.ensemble import mirrored_cnn_weights

    _, cnn = _nets(sum(dims))
    x = torch.randn(*dims, 8, device=DEV)

    def run(inp, w1, b1, w2, b2):
        h1 = conv3d_fwd(inp, w1, b1, relu=True)
        return conv3d_fwd(h1.view(*dims, -1), w2, b2, relu=False)

    plain = mirrored_cnn_weights(cnn, (False, False, False))
    for flips in MASKS[1:]:
        want = ops.flip_crop(run(ops.flip_crop(x, dims, flips), *plain), dims, flips)
        got = run(x, *mirrored_cnn_weights(cnn, flips))
        err = float((got - want).abs().max())
        print(f"mirrored weights {dims} {flips}: max |diff| {err:.3e}")
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-4), (flips, err)


# ------------------------------------------------------------------------------------------------ the predictor
@pytest.fixture(scope="module")
def members():
    return [_nets(0), _nets(1)]


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    from data_processing.data_loader import ImageGraphDataset

    data = str(tmp_path_factory.mktemp("ensemble") / "data") + "/"
    write_dataset(data, 2)
    with redirect_stdout(io.StringIO()):
        ds = ImageGraphDataset(data, "BraTS_", read_image=True, read_graph=True, read_label=False)
        return [(graph, np.asarray(feats), np.ascontiguousarray(img),
                 np.ascontiguousarray(ds.get_supervoxel_partitioning(mri))) for mri, graph, feats, img in ds]


def _node_logits(members, graph, feats):
    with torch.no_grad():
        return [gnn(graph.to(DEV), torch.FloatTensor(feats).to(DEV)).float().cpu().numpy() for gnn, _ in members]


def test_predict_joint_matches_the_float64_definition(members, samples):
    from gts.ensemble import EnsemblePredictor, mirror_views
    from utils.hyperparam_helpers import DEFAULT_BACKGROUND_NODE_LOGITS

    views = mirror_views("xyz")
    predictor = EnsemblePredictor([g for g, _ in members], [c for _, c in members], views)
    assert predictor.terms == 16
    for graph, feats, img, svs in samples:
        assert svs.shape == (24, 20, 16)
        labels, probs, box = predictor.predict_joint(graph, feats, img, svs, return_probabilities=True)
        ref = R.ensemble_ref(_node_logits(members, graph, feats), [c for _, c in members], views, img, svs,
                             DEFAULT_BACKGROUND_NODE_LOGITS)
        for mine, theirs in zip(box.host, ref["crop"]):
            assert np.array_equal(mine, theirs.reshape(-1))
        err = float(np.abs(probs.cpu().numpy().astype(np.float64) - ref["probs"]).max())
        clear_box = ref["margin"] > 1e-3
        print(f"predict_joint: box {box.shape}, max |mean probability - float64| {err:.3e}, "
              f"clear voxels {clear_box.mean():.3f} of the box")
        assert err <= 1e-4
        assert labels.dtype == np.int16 and labels.shape == svs.shape
        clear = np.zeros(svs.shape, dtype=bool)
        clear[ref["crop"]] = clear_box
        outside = np.ones(svs.shape, dtype=bool)
        outside[ref["crop"]] = False
        assert clear.mean() > 0.5 * (~outside).mean()
        assert np.array_equal(labels[clear], ref["labels"][clear]) and not labels[outside].any()
        assert np.array_equal(labels, predictor.predict_joint(graph, feats, img, svs))
        relabelled = predictor.predict_joint(graph, feats, img, svs,
                                             relabel=torch.tensor([0, 2, 1, 4], dtype=torch.int16, device=DEV))
        assert np.array_equal(relabelled, np.array([0, 2, 1, 4], dtype=np.int16)[labels])


def test_one_member_one_view_is_the_plain_softmax(members, samples):
    """M * V = 1: the mean probability is the softmax of the one net's logits on the HIP convolutions."""
    from gts.conv3d import refinement_logits
    from gts.ensemble import EnsemblePredictor

    gnn, cnn = members[0]
    graph, feats, img, svs = samples[0]
    labels, probs, box = EnsemblePredictor([gnn], [cnn]).predict_joint(graph, feats, img, svs,
                                                                       return_probabilities=True)
    with torch.no_grad():
        table = gnn(graph.to(DEV), torch.FloatTensor(feats).to(DEV)).float()
        x = ops.crop_concat_rows(torch.from_numpy(img).to(DEV), torch.from_numpy(svs).to(DEV), table,
                                 torch.tensor([1.0, -1.0, -1.0, -1.0], device=DEV), box)
        want = torch.softmax(refinement_logits(x, cnn).double(), dim=1).cpu().numpy()
    assert float(np.abs(probs.view(-1, 4).cpu().numpy() - want).max()) <= E1_BOUND
    assert labels[box.as_ix()].shape == box.shape


def test_predict_gnn_and_node_probabilities(members, samples):
    from gts.ensemble import EnsemblePredictor

    predictor = EnsemblePredictor([g for g, _ in members])
    for graph, feats, img, svs in samples:
        want_probs, want_labels, margin = R.node_prediction(_node_logits(members, graph, feats), svs)
        got_probs = predictor.node_probabilities(graph, feats).cpu().numpy()
        assert float(np.abs(got_probs.astype(np.float64) - want_probs).max()) <= E1_BOUND
        got = predictor.predict_gnn(graph, feats, svs)
        clear = margin > 1e-5
        assert got.dtype == np.int16 and got.shape == svs.shape and clear.mean() > 0.5
        assert np.array_equal(got[clear], want_labels[clear])
        assert not got[svs < 0].any()


# ------------------------------------------------------------------------------------------------ command lines
def _save_full_size_nets(folder, seeds):
    from model.networks import CnnRefinementNet, init_graph_net
    from utils.hyperparam_helpers import EvalParamSet

    paths = []
    for seed in seeds:
        torch.manual_seed(seed)
        gnn, cnn = os.path.join(folder, f"gnn_f{seed}.pt"), os.path.join(folder, f"cnn_f{seed}.pt")
        torch.save(init_graph_net("GSpool", EvalParamSet(20, 4, [256] * 4, None, None)).state_dict(), gnn)
        torch.save(CnnRefinementNet(8, 4, [16]).state_dict(), cnn)
        paths.append((gnn, cnn))
    return paths


def test_joint_cli_writes_the_predictors_volumes(tmp_path):
    from data_processing import nifti_io
    from data_processing.data_loader import ImageGraphDataset
    from data_processing.image_processing import uncrop_to_brats_size
    from data_processing.labels import INTERNAL_TO_BRATS
    from scripts import cleanup, ensemble_flags
    from scripts import generate_joint_predictions as joint

    data, out = str(tmp_path / "data") + "/", str(tmp_path / "out")
    write_dataset(data, 2)
    (g0, c0), (g1, c1) = _save_full_size_nets(str(tmp_path), (1, 2))
    with redirect_stdout(io.StringIO()) as log:
        rc = joint.main(["-d", data, "-p", "BraTS_", "-o", out, "-g", g0, "-c", c0, "--also_gnn_weights", g1,
                         "--also_cnn_weights", c1, "--tta_mirror", "xz", "--min_component_voxels", "5"])
        ds = ImageGraphDataset(data, "BraTS_", read_image=True, read_graph=True, read_label=False)
        predictor = ensemble_flags.Members([g0, g1], [c0, c1], "xz").predictor("GSpool")
    assert rc == 0 and predictor.terms == 8
    relabel = torch.from_numpy(INTERNAL_TO_BRATS).to(DEV)
    for mri, graph, feats, img in ds:
        saved = nifti_io.read_nifti(os.path.join(out, f"{mri}.nii.gz"), np.int16)
        pred = predictor.predict_joint(graph, feats, img, ds.get_supervoxel_partitioning(mri), relabel,
                                       cleanup=cleanup.Cleanup(min_component_voxels=5))
        assert saved.shape == (240, 240, 155) and set(np.unique(saved)) <= {0, 1, 2, 4}
        assert np.array_equal(saved, uncrop_to_brats_size(ds.get_crop(mri), pred))
        assert f"{mri}: components " in log.getvalue() and "components_removed" in log.getvalue()
    assert "ensemble of 2 member(s) x 4 view(s)" in log.getvalue()


def test_gnn_cli_averages_the_members(tmp_path):
    from data_processing import nifti_io
    from data_processing.data_loader import ImageGraphDataset
    from data_processing.image_processing import uncrop_to_brats_size
    from data_processing.labels import INTERNAL_TO_BRATS
    from scripts import ensemble_flags
    from scripts import generate_gnn_predictions as gen

    data, out = str(tmp_path / "data") + "/", str(tmp_path / "out")
    write_dataset(data, 2)
    (g0, _), (g1, _) = _save_full_size_nets(str(tmp_path), (3, 4))
    with redirect_stdout(io.StringIO()):
        assert gen.main(["-d", data, "-p", "BraTS_", "-o", out, "-w", g0, "-f", "preds", "--also_gnn_weights", g1]) == 0
        ds = ImageGraphDataset(data, "BraTS_", read_image=False, read_graph=True, read_label=False)
        predictor = ensemble_flags.Members([g0, g1], None, "").predictor()
    relabel = torch.from_numpy(INTERNAL_TO_BRATS).to(DEV)
    for mri, graph, feats in ds:
        saved = nifti_io.read_nifti(os.path.join(out, f"{mri}.nii.gz"), np.int16)
        pred = predictor.predict_gnn(graph, feats, ds.get_supervoxel_partitioning(mri), relabel)
        assert np.array_equal(saved, uncrop_to_brats_size(ds.get_crop(mri), pred))


# preprocess_dataset + generate_joint_predictions against segment_scans, both with the ensemble flags, on one
# synthetic scan (the kind tests/test_gpu_segment.py segments); one process, bounded by the subprocess timeout.
_E2E = r"""
import io, os, sys
from contextlib import redirect_stdout
import torch
from gts import synth_mri
from model.networks import CnnRefinementNet, init_graph_net
from utils.hyperparam_helpers import EvalParamSet
from scripts import generate_gnn_predictions, generate_joint_predictions, preprocess_dataset, segment_scans
tmp = sys.argv[1]
j = lambda *p: os.path.join(tmp, *p)
raw = j("raw")
synth_mri.write_sample(raw, "BraTS_000", 300)
hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
for fold in (0, 1):
    torch.manual_seed(fold)
    torch.save(init_graph_net("GSpool", hp).state_dict(), j(f"gnn{fold}.pt"))
    torch.save(CnnRefinementNet(8, 4, [16]).state_dict(), j(f"cnn{fold}.pt"))
flags = ["--also_gnn_weights", j("gnn1.pt"), "--also_cnn_weights", j("cnn1.pt"), "--tta_mirror", "xz",
         "--min_component_voxels", "20"]
gnn_flags = ["--also_gnn_weights", j("gnn1.pt")]
with redirect_stdout(io.StringIO()):
    assert preprocess_dataset.main(["-d", raw, "-o", j("ds"), "-n", "6000"]) == 0
    assert generate_joint_predictions.main(["-d", j("ds") + "/", "-o", j("joint"), "-g", j("gnn0.pt"),
                                            "-c", j("cnn0.pt")] + flags) == 0
    assert generate_gnn_predictions.main(["-d", j("ds") + "/", "-o", j("gnn"), "-w", j("gnn0.pt"), "-f", "preds"]
                                         + gnn_flags) == 0
rc1 = segment_scans.main(["-d", raw, "-o", j("seg_joint"), "-g", j("gnn0.pt"), "-c", j("cnn0.pt"), "-n", "6000"]
                         + flags)
rc2 = segment_scans.main(["-d", raw, "-o", j("seg_gnn"), "-g", j("gnn0.pt"), "-n", "6000", "--tta_mirror", "y"]
                         + gnn_flags)
print("RC", rc1, rc2, "ENSEMBLE" if "gts.ensemble" in sys.modules else "")
"""


@pytest.mark.timeout(600)
def test_segmenter_equals_two_step_pipeline_with_ensemble_flags(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-c", _E2E, str(tmp_path)], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=550)
    assert r.returncode == 0 and "RC 0 0 ENSEMBLE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "BraTS_000: done (components " in r.stdout                      # the clean-up still reports its counts
    assert r.stdout.count("mirrors do not change a GNN prediction") == 1   # --tta_mirror without -c: one line
    for want_dir, got_dir in (("joint", "seg_joint"), ("gnn", "seg_gnn")):
        want = open(tmp_path / want_dir / "BraTS_000.nii.gz", "rb").read()
        got = open(tmp_path / got_dir / "BraTS_000.nii.gz", "rb").read()
        assert len(got) > 0 and got == want, (got_dir, len(got), len(want))
