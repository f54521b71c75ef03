"""BraTS <-> internal label maps (reference scripts/preprocess_dataset.py:15,146-169).

BraTS files use {0, 1 NCR/NET, 2 edema, 4 enhancing}; the pipeline trains on
{0, 1 edema, 2 NET, 3 ET}."""
import numpy as np

LABEL_MAP = {4: 3, 2: 1, 1: 2}          # BraTS -> internal
INTERNAL_TO_BRATS = np.array([0, 2, 1, 4], dtype=np.int16)  # index = internal label


def _check(values, allowed):
    if np.setdiff1d(np.unique(values), allowed).size:
        raise RuntimeError("unexpected label")


def swap_labels_from_brats(label_data):
    _check(label_data, [0, 1, 2, 4])
    out = np.zeros_like(label_data, dtype=np.int16)
    for brats, internal in LABEL_MAP.items():
        out[label_data == brats] = internal
    return out


def swap_labels_to_brats(label_data):
    _check(label_data, [0, 1, 2, 3])
    return INTERNAL_TO_BRATS[np.asarray(label_data, dtype=np.int64)]


def swap_labels_from_brats_any(label_data):
    """swap_labels_from_brats for a file in either BraTS convention: {0, 1, 2, 4}, or the 2023 challenge's
    {0, 1, 2, 3} (3 and 4 both mean enhancing tumour).  A volume holding both 3 and 4, or any other value, is
    refused."""
    values = np.unique(label_data)
    if np.setdiff1d(values, [0, 1, 2, 3, 4]).size or (3 in values and 4 in values):
        raise RuntimeError(f"unexpected labels {values.tolist()}: neither {{0, 1, 2, 4}} nor {{0, 1, 2, 3}}")
    label_data = np.asarray(label_data)
    return swap_labels_from_brats(np.where(label_data == 3, 4, label_data))
