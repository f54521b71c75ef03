"""The standardization statistics of a dataset as a small JSON file: written by
scripts/compute_dataset_stats.py (and `preprocess_dataset --stats compute`), read back by
`preprocess_dataset --stats FILE` and `segment_scans --stats FILE`.

The file names the modality suffixes, in channel order, that the statistics were taken with; load_stats
refuses a file whose list differs from the caller's, since statistics applied to other modalities, or to
the same ones in another order, standardize every input wrongly without any other symptom.
"""
import json

import numpy as np

CHANNELS = 4
FILE_NAME = "standardization.json"    # where `preprocess_dataset --stats compute` puts it inside OUT_DIR


class StatsError(ValueError):
    """Statistics that cannot be used for this run (the command line tools report it and stop)."""


def _vector(values, what, path):
    try:
        arr = np.asarray(values, dtype=np.float32)
    except (TypeError, ValueError):
        raise StatsError(f"{path}: {what!r} is not a list of numbers") from None
    if arr.ndim != 1 or arr.shape[0] != CHANNELS:
        raise StatsError(f"{path}: {what!r} holds {arr.size if arr.ndim == 1 else arr.shape} value(s); intake and graph "
                         f"generation are built for exactly {CHANNELS} modalities, other counts are not supported")
    if not np.isfinite(arr).all():
        raise StatsError(f"{path}: {what!r} holds a non-finite value: {arr.tolist()}")
    return arr


def save_stats(path, mean, std, modality_extensions, quantile, per_scan):
    """Write the statistics file.  per_scan: {scan id: ScanStats-like with n, top, mean, std}, the scans
    whose medians mean and std are.  A float32 value is written as the decimal form of the double that
    equals it, so it reads back to the same float32."""
    def floats(v):
        return [float(x) for x in np.asarray(v, dtype=np.float32)]

    doc = {
        "mean": floats(mean),
        "std": floats(std),
        "modality_extensions": list(modality_extensions),
        "quantile": float(quantile),
        "n_scans": len(per_scan),
        "scans": {sid: {"n": int(s.n), "top": floats(s.top), "mean": floats(s.mean), "std": floats(s.std)}
                  for sid, s in sorted(per_scan.items())},
    }
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def load_stats(path, modality_extensions=None):
    """(mean float32 [4], std float32 [4]) of a statistics file.  StatsError (a ValueError), naming the cause, for a file
    with another number of values than four, non-finite values, a standard deviation that is not positive,
    or (when modality_extensions is given) a modality list that differs from it."""
    try:
        with open(path) as f:
            doc = json.load(f)
    except OSError as exc:
        raise StatsError(f"{path}: cannot be read ({exc.strerror})") from None
    except json.JSONDecodeError as exc:
        raise StatsError(f"{path}: not a JSON statistics file ({exc})") from None
    if not isinstance(doc, dict) or "mean" not in doc or "std" not in doc:
        raise StatsError(f"{path}: a statistics file needs 'mean' and 'std'")
    mean, std = _vector(doc["mean"], "mean", path), _vector(doc["std"], "std", path)
    if not (std > 0).all():
        raise StatsError(f"{path}: every standard deviation must be positive, got {std.tolist()}")
    if modality_extensions is not None:
        theirs = doc.get("modality_extensions")
        if theirs != list(modality_extensions):
            raise StatsError(f"{path}: taken with modalities {theirs}, but this run uses {list(modality_extensions)} "
                             "(same suffixes in the same order are required)")
    return mean, std
