"""Generate ref_dataset_stats.npz by IMPORTING the reference.

Needs a checkout of the reference (rsinghlab/GNN-Tumor-Seg); not part of the test suite:
    python tests/golden/make_dataset_stats_fixture.py /path/to/GNN-Tumor-Seg
The reference's scripts.preprocess_dataset is imported with environment shims only, its files untouched:
  - stub `nibabel` and `skimage.segmentation` modules (neither is installed; neither is reached);
  - the reference's nifti_io.read_in_patient_sample / read_in_labels replaced by functions that hand back
    seeded gts.synth_mri volumes (the "path" of a scan is its index in dataset_stats_ref.FIXTURE_SCANS).
DataPreprocessor.compute_dataset_stats is called on a stand-in object: with one id at a time it yields
that scan's own mean and sigma (the median of one row), with all ids the dataset's medians.
"""
import os
import sys
import types

import numpy as np

if len(sys.argv) != 2:
    raise SystemExit(f"usage: python {sys.argv[0]} /path/to/GNN-Tumor-Seg")
REF = os.path.abspath(sys.argv[1])
OUT = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, REF)

for name in ("nibabel", "skimage", "skimage.segmentation"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["skimage.segmentation"].slic = None
import networkx as nx  # noqa: E402

if not hasattr(nx, "from_numpy_matrix"):
    nx.from_numpy_matrix = nx.from_numpy_array

from scripts import preprocess_dataset as ref_prep  # noqa: E402  (the reference's)


def _load(module_name, path):
    import importlib.util

    spec = importlib.util.spec_from_file_location(module_name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


synth_mri = _load("_synth_mri", os.path.join(REPO, "gnn-tumor-seg_amd", "gts", "synth_mri.py"))
R = _load("_dataset_stats_ref", os.path.join(REPO, "tests", "dataset_stats_ref.py"))

_SAMPLES = {}


def _sample(index):
    if index not in _SAMPLES:
        seed, shape = R.FIXTURE_SCANS[int(index)]
        _SAMPLES[index] = synth_mri.make_sample(seed, shape)
    return _SAMPLES[index]


ref_prep.nifti_io.read_in_patient_sample = lambda path, exts: _sample(path)[0]
ref_prep.nifti_io.read_in_labels = lambda path, ext: _sample(path)[1]


def reference_stats(ids):
    stand_in = types.SimpleNamespace(all_ids=list(ids), id_to_fp={i: i for i in ids}, modality_extensions=None,
                                     label_extension=None)
    mean, sd = ref_prep.DataPreprocessor.compute_dataset_stats(stand_in)
    return np.asarray(mean), np.asarray(sd)


def main():
    ids = list(range(len(R.FIXTURE_SCANS)))
    per_scan = [reference_stats([i]) for i in ids]
    mean, sd = reference_stats(ids)
    data = {
        "seeds": np.array([s for s, _ in R.FIXTURE_SCANS], dtype=np.int32),
        "shapes": np.array([sh for _, sh in R.FIXTURE_SCANS], dtype=np.int32),
        "image_digests": np.array([R.digest(_sample(i)[0]) for i in ids]),
        "label_digests": np.array([R.digest(_sample(i)[1]) for i in ids]),
        "scan_mean": np.stack([m for m, _ in per_scan]), "scan_std": np.stack([s for _, s in per_scan]),
        "dataset_mean": mean, "dataset_std": sd,
    }
    assert data["scan_mean"].dtype == np.float32 and data["dataset_mean"].dtype == np.float32
    path = os.path.join(OUT, "ref_dataset_stats.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {os.path.getsize(path)} bytes\nmean {mean}\nstd {sd}")


if __name__ == "__main__":
    main()
