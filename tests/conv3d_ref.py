"""torch-CPU fp64 restatement of the refinement CNN's replicate-padded 5x5x5 Conv3d on channels-last
volumes (reference model/networks.py:83-93), with the magnitude bounds the GPU tests compare against:
each bound is the same operation applied to absolute values, so |fp32 result - fp64 result| <= 2e-6 bound
is a rounding statement that holds whatever the operand signs."""
from collections import namedtuple

import torch
import torch.nn.functional as F

# What csrc/gts_conv3d.hip chooses for one layer (chunk_width, n_chunks, n_tiles16, geometry, wgrad_plan restated).
# A case list states its coverage through this; tests/test_conv3d_cases_host.py ties it to the workspace queries.
Plan = namedtuple("Plan", "cc chunks last nt bricks packed ntn groups target per_split nsplit last_split")

BRICK = (4, 4, 16)
WGRAD_TARGET_BLOCKS, WGRAD_TILES_PER_BLOCK = 512, 4 * 8
BIAS_PARTIAL_FLOATS = 64 * 32


def _cdiv(a, b):
    return -(-a // b)


def plan(dims, cin, cout):
    """The launch plan of a GEMM with `cin` input and `cout` output channels over a `dims` grid:
    cc, chunks   channel chunk width (4, 8, 12 or 16) and the number of chunks (1 or 2);
    last         real channels in the last chunk;
    nt           16-wide output tiles (NT of conv_kernel, MT of wgrad_kernel);
    bricks       4 x 4 x 16 bricks; packed: floats of the packed weights;
    ntn, groups  weight gradient: N tiles of one chunk and groups of 32 tiles;
    target       weight gradient: splits that fill the launch; per_split, nsplit and last_split (bricks in the last)."""
    r4 = _cdiv(cin, 4) * 4
    cc = min(r4, 16)
    chunks = _cdiv(r4, cc)
    nt = _cdiv(cout, 16)
    bricks = _cdiv(dims[0], BRICK[0]) * _cdiv(dims[1], BRICK[1]) * _cdiv(dims[2], BRICK[2])
    ntn = _cdiv(125 * cc, 16)
    groups = _cdiv(ntn, WGRAD_TILES_PER_BLOCK)
    target = _cdiv(WGRAD_TARGET_BLOCKS, chunks * groups)
    per_split = _cdiv(bricks, min(target, bricks))
    nsplit = _cdiv(bricks, per_split)
    return Plan(cc, chunks, cin - (chunks - 1) * cc, nt, bricks, chunks * 125 * (cc // 4) * nt * 64, ntn, groups,
                target, per_split, nsplit, bricks - (nsplit - 1) * per_split)


def data_plan(dims, cin, cout):
    """The data gradient of a cin -> cout layer: the same kernel with the channel counts swapped, on the grid
    padded by 2 per side."""
    return plan(tuple(d + 4 for d in dims), cout, cin)


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
