"""The host side of a launch that every wrapper shares: the operand checks, the scratch buffer of an entry point
(`gts_*_workspace(...)` bytes -> a tensor) and the buffers that are kept and grown per (device, stream)."""
import torch

from . import _lib
from ._lib import current_stream

_ITEM_BYTES = {torch.float32: 4, torch.uint8: 1, torch.int32: 4}


def expect(tensor, shape, name):
    """Operand shapes are checked on the host: the kernels index by the sizes they are given."""
    if tensor is not None and tuple(tensor.shape) != tuple(shape):
        raise _lib.GtsError(f"{name}: expected shape {tuple(shape)}, got {tuple(tensor.shape)}")


def f32(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise _lib.GtsError(f"gts kernels are fp32: got {t.dtype}")


def scratch(nbytes, device, dtype=torch.float32):
    """Fresh caller-owned scratch of at least `nbytes` bytes (what a gts_*_workspace query returned) as fp32 or
    uint8: rounded up to whole elements and never empty, so that its pointer is valid."""
    item = _ITEM_BYTES[dtype]
    return torch.empty(max(1, (int(nbytes) + item - 1) // item), dtype=dtype, device=device)


class StreamBuffers:
    """One buffer per (device, stream), grown on demand and reused: kernels on one stream run in order, so they can
    share it.  Every use (the GEMM workspace, the GAT workspace, the cluster counters) holds its own instance, so
    that two uses never alias.  zeroed: the buffer is zero when it is made (for kernels that leave it zero)."""

    def __init__(self, dtype=torch.float32, zeroed=False):
        self.dtype, self.item, self.make = dtype, _ITEM_BYTES[dtype], torch.zeros if zeroed else torch.empty
        self.held = {}

    def get(self, device, nbytes):
        key = (device, current_stream())
        buf = self.held.get(key)
        if buf is None or buf.numel() * self.item < nbytes:
            buf = self.make((nbytes + self.item - 1) // self.item, dtype=self.dtype, device=device)
            self.held[key] = buf
        return buf
