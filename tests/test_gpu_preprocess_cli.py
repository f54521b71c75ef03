"""scripts.preprocess_dataset end to end on the MI355X: synthetic BraTS NIfTI in, a dataset out that
the existing ImageGraphDataset loads and one GNN epoch trains on."""
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gnn-tumor-seg_amd")


def test_preprocess_cli_writes_a_trainable_dataset(hip_lib, tmp_path):
    from data_processing import nifti_io
    from data_processing.data_loader import ImageGraphDataset
    from gts import synth_mri
    from model.gnn_model import GNN
    from utils.hyperparam_helpers import FullParamSet

    raw = tmp_path / "raw"
    for i in range(2):
        synth_mri.write_sample(str(raw), f"BraTS_{i:03d}", 100 + i)
    out = str(tmp_path / "out")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-m", "scripts.preprocess_dataset", "-d", str(raw), "-l", "_seg.nii.gz",
                        "-o", out, "-n", "6000"], cwd=PKG, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for i in range(2):
        sid = f"BraTS_{i:03d}"
        for suffix in ("_nxgraph.json", "_input.nii.gz", "_label.nii.gz", "_supervoxels.nii.gz", "_crop.npz"):
            assert os.path.exists(os.path.join(out, sid, sid + suffix)), sid + suffix
    with redirect_stdout(io.StringIO()):
        ds = ImageGraphDataset(out + "/", "BraTS_", read_image=False, read_graph=True, read_label=True)
    assert len(ds) == 2
    for mri_id, graph, feats, labels in ds:
        feats = np.asarray(feats)
        assert feats.ndim == 2 and feats.shape[1] == 20 and graph.number_of_nodes() == feats.shape[0]
        svs = nifti_io.read_nifti(os.path.join(out, mri_id, mri_id + "_supervoxels.nii.gz"), np.int16)
        lab = nifti_io.read_nifti(os.path.join(out, mri_id, mri_id + "_label.nii.gz"), np.int16)
        assert svs.max() == feats.shape[0] - 1 and set(np.unique(svs[svs >= 0])) == set(range(feats.shape[0]))
        node_vox = np.append(np.asarray(labels), 0)[svs]          # node labels projected back onto voxels
        inside = svs >= 0
        assert (node_vox[inside] == lab[inside]).mean() > 0.8       # a node's label is its voxels' mode
    with redirect_stdout(io.StringIO()):
        hp = FullParamSet(3, 20, 4, 5e-3, 0.98, 1e-4, [0.1, 1, 2, 2], [64, 64], 0, None, None)
        torch.manual_seed(0)
        model = GNN("GSpool", hp, ds, batch_size=2)
    assert np.isfinite(model.run_epoch())
