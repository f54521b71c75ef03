"""torch-CPU fp64 restatement of the refinement CNN's replicate-padded 5x5x5 Conv3d on channels-last
volumes (reference model/networks.py:83-93), with the magnitude bounds the GPU tests compare against:
each bound is the same operation applied to absolute values, so |fp32 result - fp64 result| <= 2e-6 bound
is a rounding statement that holds whatever the operand signs."""
import torch
import torch.nn.functional as F


def conv(x, w, b=None):
    """x [cx, cy, cz, Cin] (any float dtype), w [Cout, Cin, 5, 5, 5] -> [cx cy cz, Cout]."""
    xp = F.pad(x.permute(3, 0, 1, 2)[None], (2,) * 6, mode="replicate")
    y = F.conv3d(xp, w, b)[0]
    return y.permute(1, 2, 3, 0).reshape(-1, w.shape[0])


def data_grad(dy, w, dims):
    """d <dy, conv(x, w)> / dx as [V, Cin] (the adjoint of the replicate clamp included)."""
    x = torch.zeros(*dims, w.shape[1], dtype=torch.float64, requires_grad=True)
    (conv(x, w) * dy).sum().backward()
    return x.grad.reshape(-1, w.shape[1])


def weight_grad(x, dy, cout):
    """(dw [Cout, Cin, 5, 5, 5], db [Cout]) of <dy, conv(x, w) + b>."""
    w = torch.zeros(cout, x.shape[3], 5, 5, 5, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    (conv(x, w, b) * dy).sum().backward()
    return w.grad, b.grad


def d64(t):
    return t.detach().cpu().double()
