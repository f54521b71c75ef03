"""The helpers of the NaN / Inf GPU tests against hand-made cases on CPU tensors: a yardstick that let a wrong
class or a one-word overwrite through would make every test built on it vacuous."""
import pytest
import torch

from tests.nonfinite_ref import (FENCE_ALIGN, FENCE_BITS, classes_match, fence_intact, fenced, fenced_empty,
                                 zero_nonfinite)

NAN, INF = float("nan"), float("inf")


def _t(*v):
    return torch.tensor(v, dtype=torch.float32)


def _t64(*v):
    return torch.tensor(v, dtype=torch.float64)


def test_equal_classes_and_values_inside_the_bound_pass():
    want = _t64(NAN, INF, -INF, 1.0, -2.0, 0.0)
    got = _t(NAN, INF, -INF, 1.0 + 1e-6, -2.0, 0.0)
    classes_match(got, want, _t64(0, 0, 0, 1.0, 2.0, 0.0))


@pytest.mark.parametrize("got,want", [
    ((0.0,), (NAN,)),            # a NaN erased to zero: what fmaxf(NaN, 0) does
    ((INF,), (NAN,)),
    ((NAN,), (0.0,)),            # a NaN the reference does not have
    ((NAN,), (INF,)),
    ((INF,), (-INF,)),           # the wrong infinity
    ((-INF,), (INF,)),
    ((3.0e38,), (INF,)),         # large is not infinite
    ((INF,), (1.0,)),
])
def test_a_wrong_class_is_refused(got, want):
    with pytest.raises(AssertionError):
        classes_match(_t(*got), _t64(*want), torch.ones(len(want), dtype=torch.float64))


def test_a_finite_error_is_held_to_the_bound_from_both_sides():
    want, bound = _t64(1.0, NAN), _t64(4.0, 0.0)
    inside = torch.tensor([1.0 + 0.99 * 2e-6 * 4.0, NAN], dtype=torch.float64)
    outside = torch.tensor([1.0 + 1.01 * 2e-6 * 4.0, NAN], dtype=torch.float64)
    classes_match(inside, want, bound)
    classes_match(2.0 - inside, want, bound)
    with pytest.raises(AssertionError):
        classes_match(outside, want, bound)
    with pytest.raises(AssertionError):
        classes_match(2.0 - outside, want, bound)
    classes_match(outside, want, bound, rel=4e-6)             # the bound scales with rel
    with pytest.raises(AssertionError):
        classes_match(_t(1e-20), _t64(0.0), _t64(0.0))        # a zero bound admits 1e-30 only
    with pytest.raises(AssertionError):
        classes_match(_t(1.0, 2.0), _t64(1.0), _t64(1.0))     # shapes must agree


def test_zero_nonfinite_is_the_magnitude_with_holes():
    assert torch.equal(zero_nonfinite(_t(NAN, -INF, INF, -2.0, 0.5)), _t64(0, 0, 0, 2.0, 0.5))


@pytest.mark.parametrize("shape", [(1,), (3, 5), (64,), (37, 4), (2, 3, 18, 3)])
def test_fenced_operand_sits_between_intact_pads(shape):
    t = torch.arange(1, 1 + torch.Size(shape).numel(), dtype=torch.float32).view(shape)
    view, buf = fenced(t)
    n = t.numel()
    front = (view.data_ptr() - buf.data_ptr()) // 4
    assert view.is_contiguous() and view.shape == t.shape and torch.equal(view, t)
    assert front > 0 and front % FENCE_ALIGN == 0 and buf.numel() - front - n >= n
    assert buf.dim() == 1 and torch.isnan(buf[:front]).all() and torch.isnan(buf[front + n:]).all()
    assert (buf.view(torch.int32)[0].item() & 0xFFFFFFFF) == FENCE_BITS
    assert fence_intact(buf, view)
    view.fill_(-1.0)                                          # writing the operand itself is not a fence break
    assert fence_intact(buf, view)
    for at in (front - 1, front + n, 0, buf.numel() - 1):     # one word of each pad, nearest and farthest
        keep = buf[at].clone()
        buf[at] = 0.0
        assert not fence_intact(buf, view)
        buf[at] = NAN                                         # a NaN of another payload is an overwrite too
        assert not fence_intact(buf, view)
        buf.view(torch.int32)[at] = keep.view(torch.int32)
        assert fence_intact(buf, view)


def test_fenced_with_a_finite_fill_and_fenced_outputs():
    view, buf = fenced(_t(1.0, 2.0), fill=7.0)
    assert torch.equal(view, _t(1.0, 2.0)) and int((buf == 7.0).sum()) == buf.numel() - 2
    out, obuf = fenced_empty((5, 4), torch.device("cpu"))
    assert out.shape == (5, 4) and out.is_contiguous() and fence_intact(obuf, out)
    assert (obuf.view(torch.int32) & 0xFFFFFFFF == FENCE_BITS).all()           # the output itself starts as the payload NaN
