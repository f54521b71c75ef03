"""Standardization statistics of a dataset on the MI355X: the device form of
DataPreprocessor.compute_dataset_stats (reference scripts/preprocess_dataset.py:93-115)

    healthy = np.logical_and(img[:, :, :, 0] > 0.001, lab == 0)
    img = normalize_img(img[healthy], is_flat=True)
    mu, sigma = np.mean(img, axis=0), np.std(img, axis=0)          # per scan
    np.median(mus, axis=0), np.median(sigmas, axis=0)              # per dataset

through the D1-D3 kernels of csrc/gts_dataset_stats.hip.  The tops are numpy's float32 quantiles bit for
bit; the mean and the standard deviation are accumulated in float64 on the device and rounded once to
float32, so they are the correctly rounded statistics of the normalized values (to within the last bit),
not the float32-accumulated ones the reference's np.mean / np.std return.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib, intake

CHANNELS = intake.CHANNELS
ScanStats = namedtuple("ScanStats", "n top mean std")


def stage_labels(labels):
    """[X, Y, Z] label volume (numpy, any layout) -> host int16 tensor [Z, Y, X], the voxel order of stage_scan."""
    lab = np.asarray(labels)
    if lab.ndim != 3:
        raise ValueError(f"the label volume must be 3-D, got shape {lab.shape}")
    host = torch.empty(lab.shape[::-1], dtype=torch.int16)
    host.numpy()[...] = lab.T
    return host


class _Scan:
    """The device side of one scan: uploaded volumes and labels, the shared workspace."""

    def __init__(self, volumes, labels):
        host = volumes if isinstance(volumes, torch.Tensor) else intake.stage_scan(volumes)
        lab = labels if isinstance(labels, torch.Tensor) else stage_labels(labels)
        if tuple(lab.shape) != tuple(host.shape[1:]):
            raise ValueError(f"labels {tuple(lab.shape)[::-1]} and volumes {tuple(host.shape[1:])[::-1]} differ in shape")
        self.shape = tuple(int(d) for d in host.shape[1:][::-1])
        dev = intake._device()
        self.lib = _lib.load()
        nbytes = int(self.lib.gts_dataset_stats_workspace(*self.shape))
        if nbytes < 0:
            raise ValueError(f"volume {self.shape} is outside the kernels' limits (extent <= 4096, < 2^31 voxels)")
        self.src = host.to(dev, non_blocking=True)
        self.lab = lab.to(dev, non_blocking=True)
        self.code = intake.DTYPE_CODES[intake._np_dtype(self.src)]
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def mask(self):
        """D1: (member count, members with a non-finite value)."""
        counts = torch.empty(2, dtype=torch.int64, device=self.src.device)
        _lib.check(self.lib.gts_dataset_stats_mask(self.src.data_ptr(), self.code, self.lab.data_ptr(), *self.shape,
                                                   counts.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                   _lib.current_stream()), "gts_dataset_stats_mask")
        n, bad = counts.cpu().tolist()
        return int(n), int(bad)

    def order_stats(self, n, ranks):
        """D2: float32 [4, 2], the values at ranks (lo, hi) of each channel's member values."""
        out = torch.empty((CHANNELS, 2), dtype=torch.float32, device=self.src.device)
        _lib.check(self.lib.gts_dataset_stats_order_stats(self.src.data_ptr(), self.code, *self.shape, n, ranks[0],
                                                          ranks[1], out.data_ptr(), self.ws.data_ptr(),
                                                          self.ws.numel(), _lib.current_stream()),
                   "gts_dataset_stats_order_stats")
        return out.cpu().numpy()

    def moments(self, n, top):
        """D3: float64 [4, 4]: sum y, sum y^2, mean, standard deviation, as the device holds them."""
        top = np.ascontiguousarray(top, dtype=np.float32)
        out = torch.empty((4, CHANNELS), dtype=torch.float64, device=self.src.device)
        _lib.check(self.lib.gts_dataset_stats_moments(self.src.data_ptr(), self.code, *self.shape, n,
                                                      top.ctypes.data_as(ctypes.c_void_p), out.data_ptr(),
                                                      self.ws.data_ptr(), self.ws.numel(), _lib.current_stream()),
                   "gts_dataset_stats_moments")
        return out.cpu().numpy()


def scan_stats(volumes, labels, q=intake.QUANTILE, timer=None, sums=None):
    """One scan -> ScanStats(n, top float32 [4], mean float32 [4], std float32 [4]).

    volumes: four [X, Y, Z] arrays (as nifti_io.read_nifti_raw returns them) or the host tensor of
    intake.stage_scan; labels: the [X, Y, Z] label volume in raw BraTS coding (as nifti_io.read_in_labels
    returns it) or the host tensor of stage_labels.  Raises ValueError when the healthy-tissue mask is empty,
    when a voxel inside it is non-finite, or when a channel's quantile is not positive (the reference would
    go on with NaN or inf).  timer(name) is called after each stage; sums, a list, receives the device's
    float64 [4, 4] block (sum y, sum y^2, mean, std) for the determinism tests."""
    tick = timer or (lambda name: None)
    scan = _Scan(volumes, labels)
    tick("upload")
    n, bad = scan.mask()
    tick("D1")
    if n == 0:
        raise ValueError("no healthy-tissue voxel (first modality > 0.001 and label 0): nothing to take statistics of")
    if bad:
        raise ValueError(f"{bad} healthy-tissue voxel(s) hold a non-finite value")
    stats = scan.order_stats(n, intake.quantile_ranks(n, q))
    top = np.array([intake.quantile_from_order_stats(stats[c, 0], stats[c, 1], n, q) for c in range(CHANNELS)],
                   dtype=np.float32)
    tick("D2")
    if not (top > 0).all():
        raise ValueError(f"the {q} quantile of the healthy tissue is not positive in every modality: {top.tolist()}")
    block = scan.moments(n, top)
    tick("D3")
    if sums is not None:
        sums.append(block)
    return ScanStats(n, top, block[2].astype(np.float32), block[3].astype(np.float32))


def dataset_stats(per_scan):
    """(mean float32 [4], std float32 [4]): the medians over the scans of the per-scan vectors
    (reference scripts/preprocess_dataset.py:112-113).  per_scan: ScanStats, or (mean, std) pairs."""
    rows = [(s.mean, s.std) if isinstance(s, ScanStats) else (s[0], s[1]) for s in per_scan]
    if not rows:
        raise ValueError("no scan to take the dataset statistics of")
    means = [np.asarray(m, dtype=np.float32) for m, _ in rows]
    stds = [np.asarray(s, dtype=np.float32) for _, s in rows]
    return np.median(means, axis=0), np.median(stds, axis=0)
