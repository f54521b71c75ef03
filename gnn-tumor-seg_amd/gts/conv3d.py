"""The refinement CNN's two 5x5x5 replicate-padded Conv3d layers for training (C1-C5, csrc/gts_conv3d.hip).

`refinement_logits(x, net)` is one autograd node: channels-last input [cx, cy, cz, Cin] and the two
`nn.Conv3d` modules of a `model.networks.CnnRefinementNet` -> logits [V, Cout] (V = cx cy cz, z fastest),
the same values as `net(x.movedim(-1, 0)[None])[0].movedim(0, -1).reshape(-1, Cout)`.  The weights are
read from the modules, so `state_dict` keys stay `conv_layers.{0,1}.{weight,bias}`.  Backward gives the
four parameter gradients; the input takes none (the first layer needs no data gradient).
"""
import torch

from . import _lib
from ._lib import check, current_stream, ptr, require_device
from ._operands import expect, f32, scratch

MAX_CHANNELS = 32


def _channels_ok(*counts):
    for c in counts:
        if not 1 <= c <= MAX_CHANNELS:
            raise _lib.GtsError(f"conv3d: channel count {c} outside 1..{MAX_CHANNELS}")


def _operands(x=None, w=None, b=None, dy=None, h=None, dims=None):
    """Host-side checks of every operand before a launch: fp32, contiguous, one device, and shapes that agree
    with the weights and the volume (the kernels index by the sizes they are given)."""
    f32(x, w, b, dy, h)
    require_device(x, w, b, dy, h)
    if w is not None and (w.dim() != 5 or tuple(w.shape[2:]) != (5, 5, 5)):
        raise _lib.GtsError(f"conv3d: weight must be [Cout, Cin, 5, 5, 5], got {tuple(w.shape)}")
    if x is not None and x.dim() != 4:
        raise _lib.GtsError(f"conv3d: input must be channels-last [cx, cy, cz, C], got {tuple(x.shape)}")
    if dims is not None and (len(dims) != 3 or min(dims) < 1):
        raise _lib.GtsError(f"conv3d: volume dimensions must be three positive sizes, got {dims}")


def conv3d_fwd(x, w, b, relu):
    """C1 / C2: act(conv(x) + b) for channels-last x [cx, cy, cz, Cin] -> [V, Cout]."""
    _operands(x=x, w=w, b=b)
    cx, cy, cz, cin = x.shape
    cout = w.shape[0]
    _channels_ok(cin, cout)
    expect(w, (cout, cin, 5, 5, 5), "conv3d_fwd weight")
    expect(b, (cout,), "conv3d_fwd bias")
    lib = _lib.load()
    ws = scratch(lib.gts_conv3d_fwd_workspace(cin, cout), x.device)
    y = torch.empty((cx * cy * cz, cout), dtype=torch.float32, device=x.device)
    check(lib.gts_conv3d_fwd_f32(ptr(x), ptr(w), ptr(b), ptr(y), cx, cy, cz, cin, cout, int(relu), ptr(ws),
                                 ws.numel() * 4, current_stream()), "gts_conv3d_fwd_f32")
    return y


def conv3d_bwd_data(dy, w, dims, h=None):
    """C3: [V, Cin] gradient of the layer input from dy [V, Cout]; zero where h (the ReLU output
    that fed the layer, [V, Cin]) is not positive."""
    _operands(w=w, dy=dy, h=h, dims=dims)
    cout, cin = w.shape[:2]
    _channels_ok(cin, cout)
    cx, cy, cz = dims
    v = cx * cy * cz
    expect(dy, (v, cout), "conv3d_bwd_data dy")
    expect(h, (v, cin), "conv3d_bwd_data h")
    lib = _lib.load()
    ws = scratch(lib.gts_conv3d_bwd_data_workspace(cx, cy, cz, cin, cout), dy.device)
    dx = torch.empty((cx * cy * cz, cin), dtype=torch.float32, device=dy.device)
    check(lib.gts_conv3d_bwd_data_f32(ptr(dy), ptr(w), ptr(h), ptr(dx), cx, cy, cz, cin, cout, ptr(ws),
                                      ws.numel() * 4, current_stream()), "gts_conv3d_bwd_data_f32")
    return dx


def conv3d_bwd_weight(x, dy, cout, want_bias=True):
    """C4 / C5: (dw [Cout, Cin, 5, 5, 5], db [Cout] or None) from the layer input x [cx, cy, cz, Cin]
    and dy [V, Cout]."""
    _operands(x=x, dy=dy)
    cx, cy, cz, cin = x.shape
    _channels_ok(cin, cout)
    expect(dy, (cx * cy * cz, cout), "conv3d_bwd_weight dy")
    lib = _lib.load()
    ws = scratch(lib.gts_conv3d_bwd_weight_workspace(cx, cy, cz, cin, cout), x.device)
    dw = torch.empty((cout, cin, 5, 5, 5), dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if want_bias else None
    check(lib.gts_conv3d_bwd_weight_f32(ptr(x), ptr(dy), ptr(dw), ptr(db), cx, cy, cz, cin, cout, ptr(ws),
                                        ws.numel() * 4, current_stream()), "gts_conv3d_bwd_weight_f32")
    return dw, db


class _Refinement(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        if ctx.needs_input_grad[0]:
            raise _lib.GtsError("refinement_logits: the input takes no gradient")
        h1 = conv3d_fwd(x, w1, b1, relu=True)
        y = conv3d_fwd(h1.view(*x.shape[:3], -1), w2, b2, relu=False)
        ctx.save_for_backward(x, h1, w2)
        ctx.cmid = w1.shape[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h1, w2 = ctx.saved_tensors
        dims = tuple(x.shape[:3])
        dy = dy.contiguous()
        dw2, db2 = conv3d_bwd_weight(h1.view(*dims, -1), dy, w2.shape[0])
        dz1 = conv3d_bwd_data(dy, w2, dims, h=h1)
        dw1, db1 = conv3d_bwd_weight(x, dz1, ctx.cmid)
        return None, dw1, db1, dw2, db2


def refinement_logits(x, net):
    """x: fp32 channels-last [cx, cy, cz, Cin] on the GPU; net: a CnnRefinementNet (its two Conv3d
    modules are used, not its forward).  Returns logits [cx * cy * cz, Cout]."""
    if x.dim() != 4:
        raise _lib.GtsError(f"refinement_logits takes [cx, cy, cz, C], got {tuple(x.shape)}")
    c1, c2 = net.conv_layers[0], net.conv_layers[1]
    params = (c1.weight, c1.bias, c2.weight, c2.bias)
    f32(x, *params)
    x = x.contiguous()
    require_device(x, *[p.detach() for p in params])
    if x.shape[3] != c1.in_channels or c2.in_channels != c1.out_channels:
        raise _lib.GtsError(f"input has {x.shape[3]} channels, the network takes {c1.in_channels}")
    return _Refinement.apply(x, *params)
