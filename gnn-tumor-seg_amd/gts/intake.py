"""Intake of a raw four-modality scan on the MI355X: the device form of the host step of
DataPreprocessor.load (scripts/preprocess_dataset.py)

    crop  = determine_brain_crop(image)
    image = standardize_img(normalize_img(image[crop]), mean, std)

through the I1-I3 kernels of csrc/gts_intake.hip.  The volumes are uploaded as NIfTI stores them
(int16 or float32, x fastest); the result is bit for bit the numpy one: the crop's np.ix_ triple, the
four float32 0.995-quantiles and the standardized float32 image [cx, cy, cz, 4] on the device.
"""
import ctypes

import numpy as np
import torch

from . import _lib, _volume
from ._operands import scratch

CHANNELS = 4
QUANTILE = 0.995
DTYPE_CODES = {np.dtype(np.int16): _volume.I16, np.dtype(np.float32): _volume.F32}   # NIfTI datatype codes
_TORCH = {np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32}


def _device():
    if not torch.cuda.is_available():
        raise _lib.GtsError("scan intake runs on the MI355X HIP path only: no GPU visible")
    return torch.device("cuda", torch.cuda.current_device())


def _virtual_index(n, q):
    # np.quantile casts a Python-float q to a float array's dtype (numpy >= 2), so for float32 data the
    # virtual index (n - 1) * q, its floor and the weight are float32 arithmetic
    vi = (n - 1) * np.asarray(q, dtype=np.float32)
    return vi, np.floor(vi)


def quantile_ranks(n, q=QUANTILE):
    """The two ranks np.quantile(x, q) (linear method) interpolates between for n float32 values."""
    vi, prev = _virtual_index(n, q)
    if vi >= n - 1:
        return n - 1, n - 1
    return int(prev), int(prev) + 1


def quantile_from_order_stats(lo_value, hi_value, n, q=QUANTILE):
    """np.quantile(x, q).astype(np.float32) of n float32 values from the two values at
    quantile_ranks(n, q): numpy 2.2's linear method and _lerp with numpy's own types — the weight
    t = vi - floor(vi) is float32 like the data, so the difference b - a, the product and the sum
    are float32 operations; the upper neighbour's form b - (b - a) * (1 - t) when t >= 0.5."""
    vi, prev = _virtual_index(n, q)
    a, b = np.float32(lo_value), np.float32(hi_value)
    if vi >= n - 1:
        return b
    t = np.asarray(vi - prev, dtype=vi.dtype)
    diff = b - a
    if t >= 0.5:
        return np.float32(b - diff * (1 - t))
    return np.float32(a + diff * t)


def stage_scan(volumes, pin=True):
    """Four [X, Y, Z] volumes (numpy, any layout) -> one host tensor [4, Z, Y, X] in their common
    stored dtype (int16 or float32; anything else, or mixed dtypes, becomes float32), pinned when
    a GPU is visible so that the upload is asynchronous."""
    vols = [np.asarray(v) for v in volumes]
    if len(vols) != CHANNELS:
        raise ValueError(f"expected {CHANNELS} modality volumes, got {len(vols)}")
    shape = vols[0].shape
    if len(shape) != 3 or any(v.shape != shape for v in vols):
        raise ValueError(f"modality volumes must share one 3-D shape, got {[v.shape for v in vols]}")
    dtypes = {v.dtype for v in vols}
    dt = dtypes.pop() if len(dtypes) == 1 else np.dtype(np.float32)
    if dt not in DTYPE_CODES:
        dt = np.dtype(np.float32)
    host = torch.empty((CHANNELS,) + shape[::-1], dtype=_TORCH[dt],
                       pin_memory=pin and torch.cuda.is_available())
    dst = host.numpy()
    for c, v in enumerate(vols):
        dst[c] = v.T                     # [Z, Y, X] C order = the volume's x-fastest order
    return host


def occupancy(src, shape):
    """I1: (three boolean plane masks, number of voxels with a non-finite value)."""
    X, Y, Z = shape
    dev = src.device
    flags = torch.empty(X + Y + Z, dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().gts_intake_occupancy(src.data_ptr(), DTYPE_CODES[_np_dtype(src)], X, Y, Z,
                                                flags.data_ptr(), flags[X:].data_ptr(), flags[X + Y:].data_ptr(),
                                                bad.data_ptr(), _lib.current_stream()), "gts_intake_occupancy")
    host = torch.cat([flags, bad.to(torch.int32)]).cpu().numpy()    # one device -> host copy
    f = host[:-1].astype(bool)
    return (f[:X], f[X:X + Y], f[X + Y:]), int(host[-1])     # the count is < X * Y * Z < 2^31


def _np_dtype(t):
    return np.dtype(np.int16) if t.dtype == torch.int16 else np.dtype(np.float32)


def _index_lists(masks, dev):
    idx = [np.flatnonzero(m).astype(np.int32) for m in masks]
    packed = torch.from_numpy(np.concatenate(idx)).to(dev)
    sizes = [len(i) for i in idx]
    return packed[:sizes[0]], packed[sizes[0]:sizes[0] + sizes[1]], packed[sizes[0] + sizes[1]:], sizes


def order_stats(src, shape, lists, sizes, ranks):
    """I2: float32 [4, 2], the values at ranks (lo, hi) of each channel's cropped values."""
    X, Y, Z = shape
    lib = _lib.load()
    dev = src.device
    ws = scratch(lib.gts_intake_select_workspace(), dev, torch.uint8)
    out = torch.empty((CHANNELS, 2), dtype=torch.float32, device=dev)
    xs, ys, zs = lists
    _lib.check(lib.gts_intake_order_stats(src.data_ptr(), DTYPE_CODES[_np_dtype(src)], X, Y, Z, xs.data_ptr(),
                                          sizes[0], ys.data_ptr(), sizes[1], zs.data_ptr(), sizes[2], ranks[0],
                                          ranks[1], out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.current_stream()), "gts_intake_order_stats")
    return out.cpu().numpy()


def standardize(src, shape, lists, sizes, top, mean, std):
    """I3: ((x / top_c) - mean_c) / std_c of the cropped region as float32 [cx, cy, cz, 4] on the device."""
    X, Y, Z = shape
    params = np.ascontiguousarray(np.concatenate([top, mean, std]).astype(np.float32))
    out = torch.empty(tuple(sizes) + (CHANNELS,), dtype=torch.float32, device=src.device)
    xs, ys, zs = lists
    _lib.check(_lib.load().gts_intake_standardize(src.data_ptr(), DTYPE_CODES[_np_dtype(src)], X, Y, Z, xs.data_ptr(),
                                                  sizes[0], ys.data_ptr(), sizes[1], zs.data_ptr(), sizes[2],
                                                  params.ctypes.data_as(ctypes.c_void_p), out.data_ptr(),
                                                  _lib.current_stream()), "gts_intake_standardize")
    return out


def prepare_scan(volumes, mean, std, q=QUANTILE, timer=None):
    """Raw scan -> (image [cx, cy, cz, 4] float32 on the device, crop np.ix_ triple, tops float32 [4]).

    volumes: four [X, Y, Z] arrays (as nifti_io.read_nifti_raw returns them), the host tensor of
    stage_scan, or a tensor of that layout already on the device ([4, Z, Y, X] int16 or float32, e.g. what
    gts.conform.conform_scan returns), which is used where it lies.  Equal to determine_brain_crop, normalize_img's quantiles and
    standardize_img(normalize_img(image[crop]), mean, std) of the stacked float32 image.  A scan
    with a non-finite voxel, or without any voxel above 0.01, raises ValueError.
    timer(name) is called after each stage (host clock hooks for the measurement tool)."""
    tick = timer or (lambda name: None)
    host = volumes if isinstance(volumes, torch.Tensor) else stage_scan(volumes)
    if host.dim() != 4 or host.shape[0] != CHANNELS or host.dtype not in (torch.int16, torch.float32):
        raise ValueError(f"a staged scan is an int16 or float32 tensor [{CHANNELS}, Z, Y, X], got {host.dtype} "
                         f"{tuple(host.shape)}")
    shape = tuple(int(d) for d in host.shape[1:][::-1])
    if host.is_cuda:
        src = host.contiguous()
    else:
        src = host.to(_device(), non_blocking=True)
    dev = src.device
    tick("upload")
    masks, bad = occupancy(src, shape)
    tick("I1")
    if bad:
        raise ValueError(f"scan holds {bad} voxel(s) with a non-finite value")
    if not all(m.any() for m in masks):
        raise ValueError("scan holds no voxel above 0.01: nothing to crop")
    crop = np.ix_(*masks)
    xs, ys, zs, sizes = _index_lists(masks, dev)
    n = sizes[0] * sizes[1] * sizes[2]
    ranks = quantile_ranks(n, q)
    stats = order_stats(src, shape, (xs, ys, zs), sizes, ranks)
    top = np.array([quantile_from_order_stats(stats[c, 0], stats[c, 1], n, q) for c in range(CHANNELS)],
                   dtype=np.float32)
    tick("I2")
    image = standardize(src, shape, (xs, ys, zs), sizes, top, np.asarray(mean, np.float32),
                        np.asarray(std, np.float32))
    tick("I3")
    return image, crop, top
