"""The raw-scan segmenter on the MI355X: the I1-I3 intake kernels against numpy, the graph built without
networkx against the JSON round trip, and scripts.segment_scans end to end against preprocess_dataset +
generate_joint_predictions / generate_gnn_predictions."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gnn-tumor-seg_amd")
MEAN = np.array([0.4645, 0.6625, 0.4064, 0.3648], dtype=np.float32)
STD = np.array([0.1593, 0.1703, 0.1216, 0.1627], dtype=np.float32)


def _numpy_intake(vols):
    from data_processing.image_processing import determine_brain_crop, normalize_img, standardize_img

    image = np.stack([np.asarray(v, dtype=np.float32) for v in vols], axis=3)
    crop = determine_brain_crop(image)
    tops = np.quantile(image[crop], 0.995, axis=(0, 1, 2)).astype(np.float32)
    return crop, tops, standardize_img(normalize_img(image[crop]), MEAN, STD)


def _check_intake(vols):
    from gts import intake

    img, crop, tops = intake.prepare_scan(vols, MEAN, STD)
    want_crop, want_tops, want_img = _numpy_intake(vols)
    for got, want in zip(crop, want_crop):
        assert np.array_equal(got, want)
    assert tops.tobytes() == want_tops.tobytes(), (tops, want_tops)
    got = img.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want_img.shape
    assert np.array_equal(got, want_img)


def _synth(shape, seed):
    from gts import synth_mri

    img, _ = synth_mri.make_sample(seed, shape)
    return [img[..., c] for c in range(4)]


@pytest.mark.timeout(300)
def test_intake_full_size_int16_and_float32(hip_lib):
    vols = _synth((240, 240, 155), 7)
    _check_intake([np.asfortranarray(v.astype(np.int16)) for v in vols])
    rng = np.random.default_rng(7)
    cont = [np.asfortranarray(np.where(v > 0, v + rng.uniform(0, 1, v.shape).astype(np.float32), 0.0)
                              .astype(np.float32)) for v in vols]
    _check_intake(cont)


@pytest.mark.timeout(300)
def test_intake_small_odd_shapes(hip_lib):
    rng = np.random.default_rng(11)
    for shape in [(1, 1, 1), (7, 5, 3), (33, 17, 9), (65, 3, 18)]:
        vols = []
        for c in range(4):
            v = rng.uniform(-50.0, 200.0, shape).astype(np.float32)
            v[rng.random(shape) < 0.4] = 0.0
            v.flat[0] = 1.0 + c                    # an occupied voxel, and no channel whose top is 0 (0 / 0)
            vols.append(np.asfortranarray(v))
        _check_intake(vols)
        _check_intake([np.asfortranarray(np.rint(v).astype(np.int16)) for v in vols])


@pytest.mark.timeout(300)
def test_intake_black_interior_planes_and_constant_channel(hip_lib):
    vols = [np.asfortranarray(v.astype(np.int16)) for v in _synth((64, 60, 40), 3)]
    for v in vols:
        v[31, :, :] = 0                            # an all-black plane inside the brain, along each axis
        v[:, 29, :] = 0
        v[:, :, 20] = 0
    want_crop, _, _ = _numpy_intake(vols)
    assert not want_crop[0].ravel().tolist() == list(range(want_crop[0].min(), want_crop[0].max() + 1))
    _check_intake(vols)
    const = [v.astype(np.float32) for v in vols]
    const[2] = np.asfortranarray(np.full(const[2].shape, 3.0, dtype=np.float32))
    _check_intake(const)


@pytest.mark.timeout(300)
def test_intake_ranks_in_different_radix_buckets(hip_lib):
    from gts import intake

    shape = (10, 10, 2)                            # n = 200: ranks 198 and 199
    rng = np.random.default_rng(5)
    vols = [np.asfortranarray(rng.uniform(1.0, 100.0, shape).astype(np.float32)) for _ in range(4)]
    n = 200
    lo, hi = intake.quantile_ranks(n)
    for c, big in enumerate([1e6, 3e4, 2.5e9, 7e5]):
        flat = vols[c].reshape(-1, order="F")
        flat[: n - lo - 1] = big * (1 + np.arange(n - lo - 1, dtype=np.float32))   # rank hi lands on a big value
    for c in range(4):
        s = np.sort(vols[c].ravel())
        assert (s[lo].view(np.uint32) >> 24) != (s[hi].view(np.uint32) >> 24)       # differing top digit
    _check_intake(vols)


def _graph_arrays(g):
    return [np.asarray(getattr(g, a)) for a in ("indptr", "indices", "t_indptr", "t_indices", "t_pos", "t_slot")]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", [10, 0])
def test_direct_graph_equals_json_round_trip(hip_lib, tmp_path, k):
    import gts
    from data_processing import graph_io
    from gts import graphgen, intake
    from mri2graph.graphgen import img2graph

    vols = [np.asfortranarray(v.astype(np.int16)) for v in _synth((240, 240, 155), 21 + k)]
    img_dev, _, _ = intake.prepare_scan(vols, MEAN, STD)
    _, _, want_img = _numpy_intake(vols)
    nx_graph, feats, partition = img2graph(want_img, None, 6000, 0.5, k or None)
    fp = str(tmp_path / "g_nxgraph.json")
    graph_io.save_networkx_graph(nx_graph, fp)
    loaded = graph_io.load_networkx_graph(fp)
    want = gts.from_networkx(loaded)
    want_feats = np.array([loaded.nodes[n]["features"] for n in loaded.nodes])

    res = graphgen.build_graph(img_dev, None, 6000, 0.5, k, keep_on_device=True)
    assert all(isinstance(res[name], torch.Tensor) and res[name].is_cuda for name in ("partition", "feats"))
    got = graphgen.graph_from_edges(res["edges"], res["feats"].shape[0])
    assert got.n == want.n and got.number_of_edges() == want.number_of_edges()
    for a, b in zip(_graph_arrays(got), _graph_arrays(want)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(res["feats"].cpu().numpy(), want_feats)
    assert np.array_equal(res["feats"].to(torch.float32).cpu().numpy(), torch.FloatTensor(want_feats).numpy())
    assert np.array_equal(res["partition"].cpu().numpy(), partition)


# The two-step pipeline and the segmenter run in ONE process, so that both reach MIOpen's convolution with the
# same algorithm choice; that process is bounded by the subprocess timeout.
_E2E = r"""
import io, os, sys
from contextlib import redirect_stdout
import numpy as np, torch
from gts import synth_mri
from model.networks import CnnRefinementNet, init_graph_net
from utils.hyperparam_helpers import EvalParamSet
from scripts import generate_gnn_predictions, generate_joint_predictions, preprocess_dataset, segment_scans
tmp = sys.argv[1]
raw = os.path.join(tmp, "raw")
for i in range(2):
    synth_mri.write_sample(raw, f"BraTS_{i:03d}", 300 + i)
torch.manual_seed(0)
hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
gnn, cnn = os.path.join(tmp, "gnn.pt"), os.path.join(tmp, "cnn.pt")
torch.save(init_graph_net("GSpool", hp).state_dict(), gnn)
torch.save(CnnRefinementNet(8, 4, [16]).state_dict(), cnn)
ds = os.path.join(tmp, "ds")
j = lambda *p: os.path.join(tmp, *p)
with redirect_stdout(io.StringIO()):
    assert preprocess_dataset.main(["-d", raw, "-o", ds, "-n", "6000"]) == 0
    generate_joint_predictions.main(["-d", ds + "/", "-o", j("joint"), "-g", gnn, "-c", cnn])
    generate_gnn_predictions.main(["-d", ds + "/", "-o", j("gnn"), "-w", gnn, "-f", "preds"])
rc1 = segment_scans.main(["-d", raw, "-o", j("seg_joint"), "-g", gnn, "-c", cnn, "-n", "6000"])
rc2 = segment_scans.main(["-d", raw, "-o", j("seg_gnn"), "-g", gnn, "-n", "6000"])
rc3 = segment_scans.main(["-d", os.path.join(raw, "BraTS_001"), "-o", j("seg_docker"), "-g", gnn, "-c", cnn,
                          "-n", "6000"])
print("RC", rc1, rc2, rc3)
"""


@pytest.mark.timeout(1500)
def test_segmenter_equals_two_step_pipeline(hip_lib, tmp_path):
    from data_processing import nifti_io

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-c", _E2E, str(tmp_path)], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=1400)
    assert r.returncode == 0 and "RC 0 0 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    pairs = [("joint", "seg_joint"), ("gnn", "seg_gnn")]
    for i in range(2):
        sid = f"BraTS_{i:03d}"
        for want_dir, got_dir in pairs:
            want = nifti_io.read_nifti(str(tmp_path / want_dir / f"{sid}.nii.gz"), np.int16)
            got = nifti_io.read_nifti_raw(str(tmp_path / got_dir / f"{sid}.nii.gz"))
            assert got.dtype == np.int16 and got.shape == (240, 240, 155)
            assert np.array_equal(got, want), (sid, got_dir, int((got != want).sum()))
    docker = nifti_io.read_nifti_raw(str(tmp_path / "seg_docker" / "BraTS_001.nii.gz"))
    assert np.array_equal(docker, nifti_io.read_nifti(str(tmp_path / "joint" / "BraTS_001.nii.gz"), np.int16))


@pytest.mark.timeout(900)
def test_scan_with_nan_voxels_is_skipped(hip_lib, tmp_path):
    from data_processing import nifti_io
    from gts import synth_mri
    from model.networks import init_graph_net
    from utils.hyperparam_helpers import EvalParamSet

    raw = tmp_path / "raw"
    synth_mri.write_sample(str(raw), "BraTS_000", 400)
    bad = synth_mri.write_sample(str(raw), "BraTS_001", 401)
    flair = os.path.join(bad, "BraTS_001_flair.nii.gz")
    v = nifti_io.read_nifti(flair, np.float32)
    v[120, 120, 70] = np.nan
    nifti_io.save_as_nifti(v, flair)
    torch.manual_seed(1)
    hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
    gnn = str(tmp_path / "gnn.pt")
    torch.save(init_graph_net("GSpool", hp).state_dict(), gnn)
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-m", "scripts.segment_scans", "-d", str(raw), "-o", str(out), "-g", gnn,
                        "-n", "6000"], cwd=PKG, env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert "BraTS_001: skipped" in r.stdout and "non-finite" in r.stdout
    assert os.path.exists(out / "BraTS_000.nii.gz") and not os.path.exists(out / "BraTS_001.nii.gz")
