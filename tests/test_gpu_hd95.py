"""gts.metrics.hd95s on the GPU against the scipy route of model.evaluation.calculate_hd95s, compared
with == on float64, and both evaluate methods with scipy's distance transform made unreachable."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from tests.dataset_util import write_dataset

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _check(pred, truth):
    from gts.metrics import hd95s
    from model import evaluation

    want = evaluation.calculate_hd95s(np.asarray(pred), np.asarray(truth))
    got = hd95s(torch.from_numpy(np.ascontiguousarray(pred, dtype=np.int16)).to(DEV),
                torch.from_numpy(np.ascontiguousarray(truth, dtype=np.int16)).to(DEV))
    assert all(isinstance(g, float) for g in got)
    assert got == [float(w) for w in want], (pred.shape, got, want)
    return got


def _blobs(shape, rng, n_blobs=4, labels=(1, 2, 3)):
    """Nested tumour-like regions: spheres of label 1 holding smaller ones of 2 and 3."""
    grid = np.indices(shape).reshape(len(shape), -1).T.astype(np.float64)
    vol = np.zeros(int(np.prod(shape)), dtype=np.int16)
    for _ in range(n_blobs):
        centre = rng.uniform(0, shape)
        radius = rng.uniform(0.15, 0.35) * min(s for s in shape if s > 1) + 1
        dist = np.sqrt(((grid - centre) ** 2).sum(axis=1))
        for k, lab in enumerate(labels):
            vol[dist < radius * (1 - 0.3 * k)] = lab
    return vol.reshape(shape)


def test_reference_fixtures(golden_dir):
    import os

    d = np.load(os.path.join(golden_dir, "ref_evaluation.npz"))
    for i in range(3):
        got = _check(d[f"pred{i}"], d[f"true{i}"])
        assert got == [float(v) for v in d[f"brats{i}"][3:]]


@pytest.mark.parametrize("shape", [(37, 50, 61), (129, 3, 70), (16, 16, 16), (5, 90, 33)])
def test_random_blobs_on_odd_shapes(shape):
    rng = np.random.default_rng(sum(shape))
    for _ in range(2):
        _check(_blobs(shape, rng), _blobs(shape, rng))


@pytest.mark.parametrize("shape", [(37, 1, 50), (1, 40, 33, 21), (1, 17, 1, 23), (64, 80), (1, 1, 90), (90,),
                                   (41, 29, 1)])
def test_unit_axes_two_d_and_the_mask_mode(shape):
    rng = np.random.default_rng(len(shape) + sum(shape))
    for _ in range(2):
        _check(_blobs(shape, rng), _blobs(shape, rng))


def test_labels_outside_zero_to_three():
    rng = np.random.default_rng(7)
    pred = rng.choice(np.array([0, 1, 2, 3, 5, -2, 7], dtype=np.int16), size=(23, 31, 19), p=[.55, .1, .1, .1, .05, .05, .05])
    truth = rng.choice(np.array([0, 3, 4, -1], dtype=np.int16), size=(23, 31, 19), p=[.7, .1, .1, .1])
    _check(pred, truth)


def test_absent_regions_and_extremes():
    shape = (20, 24, 28)
    rng = np.random.default_rng(3)
    a = _blobs(shape, rng, labels=(1, 2))                 # no ET: absent from one side below, from both here
    b = _blobs(shape, rng, labels=(1, 2))
    assert _check(a, b)[2] == 0.0
    c = _blobs(shape, rng)
    c[c == 0] = 1                                         # ... ET present in truth only
    assert c[c == 3].size and _check(a, c)[2] == 300.0
    assert _check(np.zeros(shape, np.int16), np.zeros(shape, np.int16)) == [0.0, 0.0, 0.0]
    assert _check(np.zeros(shape, np.int16), c) == [300.0, 300.0, 300.0]
    one, other = np.zeros(shape, np.int16), np.zeros(shape, np.int16)
    one[3, 5, 7], other[19, 0, 27] = 3, 3                 # single voxels
    _check(one, other)
    _check(one, one)
    full = np.full(shape, 3, np.int16)                    # a region filling the volume
    _check(full, c)
    _check(full, full)
    _check(np.full((1, 1, 1), 2, np.int16), np.full((1, 1, 1), 3, np.int16))


def test_brats_size_pair_and_repeatability():
    from gts.metrics import hd95_order_stats

    shape = (240, 240, 155)
    rng = np.random.default_rng(11)
    pred, truth = np.zeros(shape, np.int16), np.zeros(shape, np.int16)
    sub = (slice(70, 170), slice(60, 180), slice(30, 125))
    sub_shape = tuple(s.stop - s.start for s in sub)
    pred[sub], truth[sub] = _blobs(sub_shape, rng, n_blobs=5), _blobs(sub_shape, rng, n_blobs=5)
    pred[200:204, 20:23, 140:150] = 1                     # a stray false positive far from the tumour
    _check(pred, truth)
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV)
    first = hd95_order_stats(p, t).cpu()
    assert torch.equal(first, hd95_order_stats(p, t).cpu())


def _host_hd95s(pred, truth):
    """The scipy route, standing in for gts.metrics.hd95s while the expected rows are computed."""
    from model import evaluation

    return evaluation.calculate_hd95s(pred.cpu().numpy(), truth.cpu().numpy())


def _forbid_scipy(monkeypatch):
    import scipy.ndimage

    from model import evaluation

    def refuse(*args, **kwargs):
        raise AssertionError("evaluate reached the host HD95 route")

    monkeypatch.setattr(evaluation, "calculate_hd95s", refuse)
    monkeypatch.setattr(evaluation, "distance_transform_edt", refuse)
    monkeypatch.setattr(scipy.ndimage, "distance_transform_edt", refuse)


def test_gnn_evaluate_does_not_use_scipy(tmp_path, monkeypatch):
    from data_processing.data_loader import ImageGraphDataset
    from model import gnn_model
    from utils.hyperparam_helpers import FullParamSet

    data = str(tmp_path / "data") + "/"
    write_dataset(data, 3)
    with redirect_stdout(io.StringIO()):
        ds = ImageGraphDataset(data, "BraTS_", read_image=False, read_graph=True, read_label=True)
        hp = FullParamSet(2, 20, 4, 5e-3, 0.98, 1e-4, [0.1, 1, 2, 2], [64, 64], 0, None, None)
        torch.manual_seed(0)
        model = gnn_model.GNN("GSpool", hp, ds, batch_size=2)
    model.run_epoch()
    subset = torch.utils.data.Subset(ds, [0, 1, 2])
    with monkeypatch.context() as m:
        m.setattr(gnn_model.gmetrics, "hd95s", _host_hd95s)
        want = model.evaluate(subset)
    _forbid_scipy(monkeypatch)
    got = model.evaluate(subset)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_refinement_evaluate_does_not_use_scipy(tmp_path, monkeypatch):
    from collections import namedtuple

    from data_processing.data_loader import ImageGraphDataset, PredLogitDataset
    from model import cnn_model
    from tests import cnn_data

    data, logits = str(tmp_path / "data") + "/", str(tmp_path / "logits")
    cnn_data.write(data, logits, ("BraTS_a", "BraTS_b"))
    image = ImageGraphDataset(data, "BraTS", read_image=True, read_graph=False, read_label=True)
    HP = namedtuple("HP", "n_epochs in_feats out_classes lr lr_decay w_decay class_weights layer_sizes")
    torch.manual_seed(4)
    model = cnn_model.RefinementModel(HP(1, 8, 4, 1e-3, 0.98, 1e-4, [0.1, 5.0, 15.0, 15.0], [16]), None,
                                      PredLogitDataset(logits))
    with monkeypatch.context() as m:
        m.setattr(cnn_model.metrics_ops, "hd95s", _host_hd95s)
        want = model.evaluate(image)
    _forbid_scipy(monkeypatch)
    got = model.evaluate(image)
    assert np.array_equal(got, want)
