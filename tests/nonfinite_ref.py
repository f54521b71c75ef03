"""Helpers of the NaN / Inf tests (tests/test_gpu_nonfinite.py): the class rule a kernel's output is held to, and
operands carved out of a NaN-filled buffer.

The class rule is exact, not a tolerance: a sum whose fp64 value is +Inf has only +Inf among its infinite terms
whatever the order, and a NaN term makes every order NaN.  It stays exact as long as the finite test data is O(1)
(nothing overflows in fp32 that does not in fp64) and zeros are placed explicitly, never reached by underflow.
"""
import math

import torch

FENCE_BITS = 0x7FC0BEEF          # a quiet NaN with a payload no arithmetic produces
FENCE_ALIGN = 64                 # floats: the front pad keeps the operand at the alignment the allocator gives anyway


def zero_nonfinite(t):
    """|t| in fp64 with NaN / Inf replaced by 0: the operand of a magnitude bound."""
    t = t.detach().cpu().double()
    return torch.where(torch.isfinite(t), t.abs(), torch.zeros_like(t))


def classes_match(got, want64, bound64, rel=2e-6):
    """Element-wise: NaN where want64 is NaN, the same Inf where it is +-Inf, and elsewhere finite with
    |got - want64| <= rel * bound64 + 1e-30."""
    got = got.detach().cpu().double()
    want64 = want64.detach().cpu().double()
    bound64 = torch.as_tensor(bound64, dtype=torch.float64).detach().cpu().expand_as(want64)
    assert got.shape == want64.shape, f"shape {tuple(got.shape)} vs {tuple(want64.shape)}"
    nan, inf = torch.isnan(want64), torch.isinf(want64)
    fin = ~(nan | inf)
    bad_nan = nan & ~torch.isnan(got)
    assert not bad_nan.any(), (f"{int(bad_nan.sum())} of {int(nan.sum())} NaN elements came out as numbers, first at "
                               f"{bad_nan.nonzero()[0].tolist()}: {got[bad_nan][0].item()}")
    bad_inf = inf & ~(got == want64)
    assert not bad_inf.any(), (f"{int(bad_inf.sum())} of {int(inf.sum())} infinite elements differ, first at "
                               f"{bad_inf.nonzero()[0].tolist()}: {got[bad_inf][0].item()} vs {want64[bad_inf][0].item()}")
    bad_fin = fin & ~torch.isfinite(got)
    assert not bad_fin.any(), (f"{int(bad_fin.sum())} of {int(fin.sum())} finite elements came out non-finite, first at "
                               f"{bad_fin.nonzero()[0].tolist()}: {got[bad_fin][0].item()}")
    err = torch.where(fin, (got - want64).abs(), torch.zeros_like(got))
    tol = rel * torch.where(fin, bound64, torch.zeros_like(bound64)) + 1e-30
    over = err > tol
    assert not over.any(), (f"{int(over.sum())} finite elements past the bound, worst err {err.max():.3e} "
                            f"(bound {bound64[fin].max():.3e}), first at {over.nonzero()[0].tolist()}")


def _fill(buf, fill):
    if isinstance(fill, float) and math.isnan(fill):
        buf.view(torch.int32).fill_(FENCE_BITS - (1 << 32) if FENCE_BITS >= 1 << 31 else FENCE_BITS)
    else:
        buf.fill_(fill)


def fenced(t, fill=float("nan")):
    """(view, buf): a contiguous fp32 tensor equal to `t` on t's device, carved from the middle of the flat buffer
    `buf`, which is filled with `fill` (a NaN fill carries the FENCE_BITS payload).  The front pad is a multiple of
    FENCE_ALIGN floats, the back pad at least as large as the operand."""
    assert t.dtype == torch.float32
    n = t.numel()
    front = FENCE_ALIGN
    back = max(n, FENCE_ALIGN)
    back += (-(front + n + back)) % FENCE_ALIGN
    buf = torch.empty(front + n + back, dtype=torch.float32, device=t.device)
    _fill(buf, fill)
    view = buf[front:front + n].view(t.shape)
    view.copy_(t)
    return view, buf


def fenced_empty(shape, device, fill=float("nan")):
    """(view, buf) of an output: as `fenced`, with the view itself pre-filled with `fill` too."""
    n = math.prod(shape)
    front = FENCE_ALIGN
    back = max(n, FENCE_ALIGN)
    back += (-(front + n + back)) % FENCE_ALIGN
    buf = torch.empty(front + n + back, dtype=torch.float32, device=device)
    _fill(buf, fill)
    return buf[front:front + n].view(shape), buf


def fence_intact(buf, view):
    """True when both pads of `buf` around `view` still hold the FENCE_BITS pattern, compared as int32."""
    assert view.is_contiguous() and view.data_ptr() >= buf.data_ptr()
    front = (view.data_ptr() - buf.data_ptr()) // 4
    bits = buf.view(torch.int32)
    want = FENCE_BITS - (1 << 32) if FENCE_BITS >= 1 << 31 else FENCE_BITS
    return bool((bits[:front] == want).all()) and bool((bits[front + view.numel():] == want).all())
