"""Python wrappers + autograd glue over the C-ABI HIP kernels (include/gts_hip.h).

Every function here enqueues on torch's current HIP stream and returns torch tensors that
own the memory; nothing falls back to PyTorch or the CPU when the library is missing.
"""
import ctypes

import torch

from . import _lib
from ._lesions import connectivity_arg
from ._lib import check, current_stream, ptr, require_device
from ._operands import StreamBuffers, expect, f32, scratch
from ._volume import SCAN_CODES, float32_out, label_volume, scan_volume, workspace
from .graph import _DeviceSchedule

_ARG_DTYPE = {0: torch.uint8, 1: torch.uint8, 4: torch.int32}

# bench.py installs callables here (kernel name -> wrapper) to bracket each launch of a kernel
# with HIP events; empty in normal use.  Names: "spmm_max_fwd_f256", "spmm_max_bwd_f256", "gat_fwd", "gat_bwd_edge",
# "gat_bwd_src" (the GAT kernels are bracketed for the HIDDEN-layer shape only: H * D >= 256; the 1-head classifier
# launches move a hundredth of the bytes and would dilute the means), 
# "project_rows".
KERNEL_TIMERS = {}
# True while bench.py runs its instrumented block: the fused layer stack then issues its launches one ctypes call at a
# time (the route the timers bracket) instead of through the one-call entry points.
INSTRUMENTED = False


def _timed(name, launch):
    timer = KERNEL_TIMERS.get(name)
    return timer(launch) if timer is not None else launch()


_counters = StreamBuffers(torch.int32, zeroed=True)
_COUNTER_BYTES = 4 * _lib.const("GTS_CLUSTER_COUNTER_WORDS")


def cluster_counters(device):
    """The unit counters of the clustered K1 / K2 kernels (include/gts_hip.h: GTS_CLUSTER_COUNTER_WORDS zero words that every launch
    leaves zero): one buffer per (device, stream), zeroed once."""
    return _counters.get(device, _COUNTER_BYTES)


# ---------------------------------------------------------------- raw kernel calls
def spmm_max_fwd(g, x, want_arg=True, relu_input=False):
    """K1.  x [N,F] -> (out [N,F], arg [N,F] slot ids or None).  relu_input: x is a ReLU output;
    maxima that are not positive get no winner, so spmm_max_bwd on this arg yields the gradient
    w.r.t. the pre-activation directly (no relu_src needed)."""
    x = x.contiguous()
    f32(x)
    require_device(x)
    d = g.dev()
    if x.dim() != 2 or x.shape[0] != g.n:
        raise _lib.GtsError(f"features must be [graph nodes = {g.n}, F], got {tuple(x.shape)}")
    n, f = g.n, x.shape[1]
    out = torch.empty((n, f), dtype=torch.float32, device=x.device)
    ab = g.arg_bytes if want_arg else 0
    arg = torch.empty((n, f), dtype=_ARG_DTYPE[ab], device=x.device) if want_arg else None
    lib = _lib.load()
    ds = _cluster_schedule(g, "in", n, f, ab)
    if ds is not None:      # LDS-staged neighbour tiles over the graph's cluster row schedule: same result, bit for bit
        def launch():
            return lib.gts_spmm_max_fwd_cluster_f32(*_DeviceSchedule.launch_args(ds), ptr(x), ptr(out), ptr(arg), ab,
                                                    1 if relu_input else 0, n, f, ptr(cluster_counters(x.device)),
                                                    current_stream())
    else:
        def launch():
            return lib.gts_spmm_max_fwd_f32(ptr(d.indptr), ptr(d.indices), ptr(x), ptr(out), ptr(arg),
                                            ab, 1 if relu_input else 0, n, f, current_stream())

    code = _timed("spmm_max_fwd_f256", launch) if (f == 256 and want_arg) else launch()
    check(code, "gts_spmm_max_fwd_f32")
    return out, arg


def _cluster_schedule(g, which, n, f, arg_bytes):
    """Device schedule for the clustered K1 / K2 kernels, or None when they do not apply (F != 256, 4-byte
    winners, tables of 4 GiB and more, no worthwhile schedule, GTS_CLUSTER_SPMM=0)."""
    from . import schedule

    if not schedule.ENABLED or f != 256 or arg_bytes not in (0, 1) or n * 1024 >= 2 ** 32 or n == 0:
        return None
    if which == "in" and n < schedule.MIN_ROWS_FORWARD:
        return None
    return g.dev_schedule(which)


def spmm_max_bwd(g, gout, arg, relu_src=None):
    """K2.  gout [N,F], arg from spmm_max_fwd -> gx [N,F]; optional fused ReLU mask."""
    gout = gout.contiguous()
    f32(gout, relu_src)
    require_device(gout, arg, relu_src)
    d = g.dev()
    if gout.dim() != 2 or gout.shape[0] != g.n:
        raise _lib.GtsError(f"gradient must be [graph nodes = {g.n}, F], got {tuple(gout.shape)}")
    n, f = g.n, gout.shape[1]
    expect(arg, (n, f), "arg")
    expect(relu_src, (n, f), "relu_src")
    if arg.dtype != _ARG_DTYPE[g.arg_bytes]:
        raise _lib.GtsError(f"arg dtype {arg.dtype} does not belong to this graph ({_ARG_DTYPE[g.arg_bytes]})")
    gx = torch.empty((n, f), dtype=torch.float32, device=gout.device)
    lib = _lib.load()
    ds = _cluster_schedule(g, "out", n, f, arg.element_size()) if relu_src is None else None
    if ds is not None:
        def launch():
            return lib.gts_spmm_max_bwd_cluster_f32(*_DeviceSchedule.launch_args(ds), ptr(gout), ptr(arg), 1, ptr(gx), n, f,
                                                    ptr(cluster_counters(gout.device)), current_stream())
    else:
        def launch():
            return lib.gts_spmm_max_bwd_f32(ptr(d.t_indptr), ptr(d.t_indices), ptr(d.t_slot), ptr(gout),
                                            ptr(arg), arg.element_size(), ptr(relu_src), ptr(gx), n, f,
                                            current_stream())

    check(_timed("spmm_max_bwd_f256", launch) if f == 256 else launch(), "gts_spmm_max_bwd_f32")
    return gx


def lowrank_bwd_applies(grad, w, arg):
    """The shapes gts_spmm_max_bwd_lowrank_f32 takes in the layer stack: a 256 -> 4 top layer with one-byte winners (the
    stack's C plan decides alike)."""
    return grad.shape[1] == 4 and tuple(w.shape) == (4, 256) and arg.element_size() == 1


def spmm_max_bwd_lowrank(g, grad, w, arg):
    """spmm_max_bwd(g, linear_bwd_input(grad, w), arg) for grad [N, 4], w [4, 256] without storing the [N, 256] product:
    the same bits.  Not bracketed as "spmm_max_bwd_f256": it moves a quarter of that kernel's bytes."""
    grad, w = grad.contiguous(), w.contiguous()
    f32(grad, w)
    require_device(grad, w, arg)
    d = g.dev()
    n = g.n
    if grad.dim() != 2 or grad.shape != (n, 4) or tuple(w.shape) != (4, 256):
        raise _lib.GtsError(f"spmm_max_bwd_lowrank takes a gradient [graph nodes = {n}, 4] and weights [4, 256], "
                            f"got {tuple(grad.shape)} and {tuple(w.shape)}")
    expect(arg, (n, 256), "arg")
    if arg.dtype != _ARG_DTYPE[g.arg_bytes]:
        raise _lib.GtsError(f"arg dtype {arg.dtype} does not belong to this graph ({_ARG_DTYPE[g.arg_bytes]})")
    gx = torch.empty((n, 256), dtype=torch.float32, device=grad.device)
    check(_lib.load().gts_spmm_max_bwd_lowrank_f32(ptr(d.t_indptr), ptr(d.t_indices), ptr(d.t_slot), ptr(grad), ptr(w),
                                                   ptr(arg), arg.element_size(), ptr(gx), n, 256, 4, current_stream()),
          "gts_spmm_max_bwd_lowrank_f32")
    return gx


def spmm_sum_raw(g, x, transposed=False, div_in=None, div_out=None, add_self=False, accum=None):
    """K3/K4.  Generic sum reducer over the in-CSR (or the out-CSR when transposed); `accum` [N,F] is added
    to the result (a gradient that reached the rows by another path)."""
    x = x.contiguous()
    f32(x, div_in, div_out, accum)
    require_device(x, div_in, div_out, accum)
    d = g.dev()
    indptr, indices = (d.t_indptr, d.t_indices) if transposed else (d.indptr, d.indices)
    n = g.n
    if x.dim() != 2 or x.shape[0] != n:
        raise _lib.GtsError(f"features must be [graph nodes = {n}, F], got {tuple(x.shape)}")
    f = x.shape[1]
    expect(div_in, (n,), "div_in")
    expect(div_out, (n,), "div_out")
    expect(accum, (n, f), "accum")
    out = torch.empty_like(x)
    check(_lib.load().gts_spmm_sum_f32(ptr(indptr), ptr(indices), ptr(x), ptr(out), ptr(div_in), ptr(div_out),
                                       ptr(accum), 1 if add_self else 0, n, f, current_stream()), "gts_spmm_sum_f32")
    return out


# ---------------------------------------------------------------- autograd: reducers
class _SpMMMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x):
        out, arg = spmm_max_fwd(g, x, want_arg=True)
        ctx.g = g
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, gout):
        (arg,) = ctx.saved_tensors
        return None, spmm_max_bwd(ctx.g, gout, arg)


class _SpMMReduce(torch.autograd.Function):
    """mode: 'sum' | 'mean' | 'gcn' (DGL reducers reached from SAGEConv)."""

    @staticmethod
    def forward(ctx, g, x, mode):
        ctx.g, ctx.mode = g, mode
        d = g.dev()
        if mode == "sum":
            return spmm_sum_raw(g, x)
        if mode == "mean":
            return spmm_sum_raw(g, x, div_out=d.deg_clamped)
        if mode == "gcn":
            return spmm_sum_raw(g, x, div_out=d.deg_plus1, add_self=True)
        raise ValueError(mode)

    @staticmethod
    def backward(ctx, gout):
        g, mode = ctx.g, ctx.mode
        d = g.dev()
        if mode == "sum":
            gx = spmm_sum_raw(g, gout, transposed=True)
        elif mode == "mean":
            gx = spmm_sum_raw(g, gout, transposed=True, div_in=d.deg_clamped)
        else:
            gx = spmm_sum_raw(g, gout, transposed=True, div_in=d.deg_plus1, add_self=True)
        return None, gx, None


def spmm_max(g, x):
    return _SpMMMax.apply(g, x)


def spmm_reduce(g, x, mode):
    return _SpMMReduce.apply(g, x, mode)


# ---------------------------------------------------------------- autograd: GAT
def _gat_fwd(g, ft, el, er, slope, bias=None, residual=None, activation=0):
    """(out, attn).  Operands are refused on the host (shape, dtype, device) before the library is loaded; strided
    operands are copied."""
    if ft.dim() != 3 or ft.shape[0] != g.n:
        raise _lib.GtsError(f"ft must be [graph nodes = {g.n}, H, D], got {tuple(ft.shape)}")
    n, h, dim = ft.shape
    expect(el, (n, h), "el")
    expect(er, (n, h), "er")
    expect(bias, (h * dim,), "bias")
    if residual is not None and (residual.shape[0] != n or residual.numel() != n * h * dim):
        raise _lib.GtsError(f"residual must hold [{n}, {h}*{dim}] values, got {tuple(residual.shape)}")
    if activation not in (0, 1):
        raise _lib.GtsError(f"_gat_fwd: activation must be 0 (none) or 1 (ELU), got {activation!r}")
    f32(ft, el, er, bias, residual)
    ft, el, er = ft.contiguous(), el.contiguous(), er.contiguous()
    bias = bias.contiguous() if bias is not None else None
    residual = residual.contiguous() if residual is not None else None
    require_device(ft, el, er, bias, residual)
    d = g.dev()
    out = torch.empty_like(ft)
    attn = torch.empty((g.number_of_edges(), h), dtype=torch.float32, device=ft.device)
    lib = _lib.load()
    ds = _gat_cluster_schedule(g, "gat_in", n, h, dim) if residual is None else None
    if ds is not None:      # LDS-staged neighbour slices over the graph's cluster row schedule: same result, bit for bit
        hs = ds.host
        nbytes = lib.gts_gat_cluster_workspace(hs.n_clusters, hs.limits[0], hs.loc_words, h, 0)
        ws = _gat_ws(ft.device, nbytes)
        launch = lambda: lib.gts_gat_fwd_cluster_f32(      # noqa: E731
            ptr(d.indptr), ptr(d.indices), *_DeviceSchedule.launch_args(ds, with_tag=True), ptr(ft), ptr(el), ptr(er),
            float(slope), ptr(bias), activation, ptr(out), ptr(attn), ptr(ws), nbytes, n, h, dim, g.max_in_degree,
            current_stream())
    else:
        launch = lambda: lib.gts_gat_fwd_f32(      # noqa: E731
            ptr(d.indptr), ptr(d.indices), ptr(ft), ptr(el), ptr(er), float(slope), ptr(bias), ptr(residual),
            activation, ptr(out), ptr(attn), n, h, dim, current_stream())
    check(_timed("gat_fwd", launch) if h * dim >= 256 else launch(), "gts_gat_fwd_f32")
    return out, attn


# _gat_ws(device, nbytes): scratch of the clustered GAT kernels (their weight blocks), grown on demand and reused: one per
# (device, stream); _gat_ws(device, 0) is the buffer the last launch used
_gat_ws = StreamBuffers().get


def _gat_cluster_schedule(g, which, n, heads, dim):
    """Device schedule for the clustered GATConv kernels, or None when they do not apply (D != 256, tables of 4 GiB and
    more, small graphs, rows of more than one 8-edge chunk, no worthwhile schedule, GTS_CLUSTER_GAT=0)."""
    from . import schedule

    if not schedule.ENABLED_GAT or dim != 256 or n < schedule.MIN_ROWS_GAT or n * heads * 1024 >= 2 ** 32 or heads > 64:
        return None
    if which.endswith("in") and g.max_in_degree > 64:
        return None
    return g.dev_schedule(which)


def _gat_bwd(g, ft, el, er, attn, gout, slope, attn_l=None, attn_r=None):
    """(gft, gel, ger); with attn_l/attn_r the score-dot-product gradient is folded into gft.  Operands are refused on
    the host (shape, dtype, device) before the library is loaded; strided operands are copied."""
    if ft.dim() != 3 or ft.shape[0] != g.n:
        raise _lib.GtsError(f"ft must be [graph nodes = {g.n}, H, D], got {tuple(ft.shape)}")
    n, h, dim = ft.shape
    expect(el, (n, h), "el")
    expect(er, (n, h), "er")
    expect(attn, (g.number_of_edges(), h), "attn")
    expect(gout, (n, h, dim), "gout")
    expect(attn_l, (h, dim), "attn_l")
    expect(attn_r, (h, dim), "attn_r")
    if (attn_l is None) != (attn_r is None):
        raise _lib.GtsError("_gat_bwd: attn_l and attn_r come together or not at all")
    f32(ft, el, er, attn, gout, attn_l, attn_r)
    ft, el, er, attn, gout = ft.contiguous(), el.contiguous(), er.contiguous(), attn.contiguous(), gout.contiguous()
    attn_l = attn_l.contiguous() if attn_l is not None else None
    attn_r = attn_r.contiguous() if attn_r is not None else None
    require_device(ft, el, er, attn, gout, attn_l, attn_r)
    d = g.dev()
    lib = _lib.load()
    ge = torch.empty_like(attn)
    ger = torch.empty_like(er)
    wide = h * dim >= 256
    es = _gat_cluster_schedule(g, "gat_edge_in", n, h, dim) if g.max_in_degree <= 8 else None
    if es is not None:
        hs = es.host
        nbytes = 2 * lib.gts_gat_cluster_workspace(hs.n_clusters, hs.limits[0], hs.loc_words, h, 0)
        ws_e = _gat_ws(ft.device, nbytes)
        edge = lambda: lib.gts_gat_bwd_edge_cluster_f32(      # noqa: E731
            ptr(d.indptr), ptr(d.indices), *_DeviceSchedule.launch_args(es, with_tag=True), ptr(ft), ptr(el), ptr(er),
            ptr(attn), ptr(gout), float(slope), ptr(ge), ptr(ger), ptr(ws_e), nbytes, n, h, dim, g.max_in_degree,
            current_stream())
    else:
        edge = lambda: lib.gts_gat_bwd_edge_f32(ptr(d.indptr), ptr(d.indices), ptr(ft), ptr(el), ptr(er), ptr(attn),   # noqa: E731
                                                ptr(gout), float(slope), ptr(ge), ptr(ger), n, h, dim, current_stream())
    check(_timed("gat_bwd_edge", edge) if wide else edge(), "gts_gat_bwd_edge_f32")
    gft = torch.empty_like(ft)
    gel = torch.empty_like(el)
    ds = _gat_cluster_schedule(g, "gat_out", n, h, dim)
    if ds is not None:
        hs = ds.host
        nbytes = lib.gts_gat_cluster_workspace(hs.n_clusters, hs.limits[0], hs.loc_words, h, 1)
        ws = _gat_ws(ft.device, nbytes)
        attn_lr = torch.stack([attn_l.reshape(-1), attn_r.reshape(-1)]) if attn_l is not None else None
        src = lambda: lib.gts_gat_bwd_src_cluster_f32(      # noqa: E731
            ptr(d.t_indptr), ptr(d.t_pos), *_DeviceSchedule.launch_args(ds, with_tag=True), ptr(attn), ptr(ge), ptr(gout),
            ptr(attn_lr), ptr(ger) if attn_l is not None else None, ptr(gft), ptr(gel), ptr(ws), nbytes, n, h, dim,
            g.max_out_degree, current_stream())
    else:
        src = lambda: lib.gts_gat_bwd_src_f32(ptr(d.t_indptr), ptr(d.t_indices), ptr(d.t_pos), ptr(attn), ptr(ge),     # noqa: E731
                                              ptr(gout), ptr(attn_l), ptr(attn_r),
                                              ptr(ger) if attn_l is not None else None, ptr(gft), ptr(gel), n, h, dim,
                                              current_stream())
    check(_timed("gat_bwd_src", src) if wide else src(), "gts_gat_bwd_src_f32")
    return gft, gel, ger


class _GATAggregate(torch.autograd.Function):
    """K5-K8.  (ft [N,H,D], el [N,H], er [N,H]) -> out [N,H,D]."""

    @staticmethod
    def forward(ctx, g, ft, el, er, negative_slope):
        ft, el, er = ft.contiguous(), el.contiguous(), er.contiguous()
        f32(ft, el, er)
        require_device(ft, el, er)
        out, attn = _gat_fwd(g, ft, el, er, negative_slope)
        ctx.g, ctx.slope = g, float(negative_slope)
        ctx.save_for_backward(ft, el, er, attn)
        return out

    @staticmethod
    def backward(ctx, gout):
        ft, el, er, attn = ctx.saved_tensors
        gft, gel, ger = _gat_bwd(ctx.g, ft, el, er, attn, gout.contiguous(), ctx.slope)
        return None, gft, gel, ger, None


def gat_aggregate(g, ft, el, er, negative_slope):
    return _GATAggregate.apply(g, ft, el, er, negative_slope)


def gat_scores(ft, attn_l, attn_r):
    """(el, er) [N,H]: <ft[n,h,:], attn_l[h,:]>, <ft[n,h,:], attn_r[h,:]> in one pass over ft."""
    ft, attn_l, attn_r = ft.contiguous(), attn_l.contiguous(), attn_r.contiguous()
    f32(ft, attn_l, attn_r)
    require_device(ft, attn_l, attn_r)
    if ft.dim() != 3:
        raise _lib.GtsError(f"ft must be [N, H, D], got {tuple(ft.shape)}")
    n, h, dim = ft.shape
    attn_l, attn_r = attn_l.reshape(-1, dim), attn_r.reshape(-1, dim)
    expect(attn_l, (h, dim), "attn_l")
    expect(attn_r, (h, dim), "attn_r")
    el = torch.empty((n, h), dtype=torch.float32, device=ft.device)
    er = torch.empty_like(el)
    check(_lib.load().gts_gat_scores_f32(ptr(ft), ptr(attn_l), ptr(attn_r), ptr(el), ptr(er), n, h, dim,
                                         current_stream()), "gts_gat_scores_f32")
    return el, er


def gat_fc_scores(h, w_fc, attn_l, attn_r, heads, dim, packed=None):
    """(ft [N,H,D], el [N,H], er [N,H]) = (h @ w_fc^T viewed [N,H,D], <ft, attn_l>, <ft, attn_r>): GATConv's projection
    with the attention scores computed in the GEMM's epilogue when the operands are tall (else GEMM + gat_scores).
    packed: dense.pack_weights copy of w_fc (fragment order; read by the panel kernels, same values)."""
    h, w_fc = h.contiguous(), w_fc.contiguous()
    attn_l, attn_r = attn_l.reshape(heads, dim).contiguous(), attn_r.reshape(heads, dim).contiguous()
    f32(h, w_fc, attn_l, attn_r)
    require_device(h, w_fc, attn_l, attn_r)
    n, k = h.shape
    if w_fc.dim() != 2 or w_fc.shape[1] != k:
        raise _lib.GtsError(f"shapes do not match: inner dims of h @ fc.weight^T ({k} vs {tuple(w_fc.shape)[-1]})")
    if w_fc.shape[0] != heads * dim:
        raise _lib.GtsError(f"shapes do not match: fc.weight rows ({w_fc.shape[0]}) vs heads * out_feats ({heads * dim})")
    if k % 4:
        raise _lib.GtsError("gat_fc_scores needs an input width that is a multiple of 4")
    lib = _lib.load()
    ft = torch.empty((n, heads, dim), dtype=torch.float32, device=h.device)
    el = torch.empty((n, heads), dtype=torch.float32, device=h.device)
    er = torch.empty_like(el)
    nbytes = lib.gts_gat_fc_scores_workspace(n, heads, dim)
    ws = scratch(nbytes, h.device)
    from . import dense
    if packed is not None:
        dense._packed_array((packed,), (w_fc,))      # size check only
    dense._timed("fwd", 2.0 * n * heads * dim * k, lambda: check(lib.gts_gat_fc_scores_f32(
        ptr(h), ptr(w_fc), ptr(attn_l), ptr(attn_r), ptr(ft), ptr(el), ptr(er), ptr(ws), ws.numel() * 4, n, heads, dim, k,
        ptr(packed), current_stream()), "gts_gat_fc_scores_f32"))
    return ft, el, er


def gat_act_bwd(gout, out, activation, want_bias_grad):
    """(g_pre, g_bias): g_pre = gout * act'(out) (activation 1 = ELU, 2 = ReLU, through the output; 0 = none),
    g_bias = g_pre.sum(0).  gout [N, ...] with N > 0 and a row of 4k floats; `out` (same shape) is read only when there is
    an activation.  Strided operands are copied; with activation 0 and a contiguous gout, g_pre IS gout."""
    if activation not in (0, 1, 2):
        raise _lib.GtsError(f"gat_act_bwd: activation must be 0 (none), 1 (ELU) or 2 (ReLU), got {activation!r}")
    if gout.dim() < 1 or gout.shape[0] == 0:
        raise _lib.GtsError(f"gat_act_bwd: gout must be [N, ...] with N > 0, got {tuple(gout.shape)}")
    if not activation:
        out = None                       # never read
    elif out is None:
        raise _lib.GtsError("gat_act_bwd: the activation's output is needed to differentiate through it")
    n, cols = gout.shape[0], gout[0].numel()
    if cols == 0 or cols % 4:
        raise _lib.GtsError(f"gat_act_bwd needs a row width that is a multiple of 4, got {cols}")
    expect(out, gout.shape, "out")
    f32(gout, out)
    gout = gout.contiguous()
    out = out.contiguous() if out is not None else None
    require_device(gout, out)
    g_pre = torch.empty_like(gout) if activation else gout
    g_bias = torch.empty(cols, dtype=torch.float32, device=gout.device) if want_bias_grad else None
    lib = _lib.load()
    ws = scratch(lib.gts_gat_reduce_workspace(n, cols), gout.device) if want_bias_grad else None
    check(lib.gts_gat_act_bwd_f32(ptr(gout), ptr(out), activation, ptr(g_pre) if activation else None,
                                          ptr(g_bias), ptr(ws), ws.numel() * 4 if ws is not None else 0,
                                          n, cols, current_stream()), "gts_gat_act_bwd_f32")
    return g_pre, g_bias


def gat_param_grad(ft, gel, ger):
    """(g_attn_l, g_attn_r) [H,D] = sum_n gel[n,h] ft[n,h,:], sum_n ger[n,h] ft[n,h,:].  ft [N,H,D] with N > 0 and
    D % 4 == 0, gel / ger [N,H]; strided operands are copied."""
    if ft.dim() != 3:
        raise _lib.GtsError(f"ft must be [N, H, D], got {tuple(ft.shape)}")
    n, h, dim = ft.shape
    expect(gel, (n, h), "gel")
    expect(ger, (n, h), "ger")
    if n == 0 or h == 0 or dim == 0 or dim % 4:
        raise _lib.GtsError(f"gat_param_grad needs N > 0, H > 0 and a head width that is a multiple of 4, "
                            f"got {tuple(ft.shape)}")
    f32(ft, gel, ger)
    ft, gel, ger = ft.contiguous(), gel.contiguous(), ger.contiguous()
    require_device(ft, gel, ger)
    gl = torch.empty((h, dim), dtype=torch.float32, device=ft.device)
    gr = torch.empty_like(gl)
    lib = _lib.load()
    ws = scratch(lib.gts_gat_reduce_workspace(n, h * dim), ft.device)
    check(lib.gts_gat_param_grad_f32(ptr(ft), ptr(gel), ptr(ger), ptr(gl), ptr(gr), ptr(ws),
                                             ws.numel() * 4, n, h, dim, current_stream()),
          "gts_gat_param_grad_f32")
    return gl, gr


# ---------------------------------------------------------------- node -> voxel projection
def project_rows(svs, table, bg_row):
    """K12.  svs int16 [...], table [N, ...] with 4/8/16-byte rows, bg_row one such row.
    Returns table_plus_bg[svs] with shape svs.shape + table.shape[1:]."""
    if svs.dtype != torch.int16:
        raise _lib.GtsError("supervoxel partitioning must be int16 (mri2graph/graphgen.py:77)")
    svs = svs.contiguous()          # NIfTI volumes arrive in Fortran order: C-order copy, same shape
    table = table.contiguous()
    bg_row = bg_row.to(table.dtype).contiguous()
    require_device(svs, table, bg_row)
    row_bytes = table.element_size() * (table[0].numel() if table.shape[0] else bg_row.numel())
    if bg_row.numel() * bg_row.element_size() != row_bytes:
        raise _lib.GtsError("background row does not match table rows")
    out = torch.empty(tuple(svs.shape) + tuple(table.shape[1:]), dtype=table.dtype, device=svs.device)
    if svs.numel() == 0:
        return out
    lib = _lib.load()
    check(_timed("project_rows", lambda: lib.gts_project_rows_i16(
        ptr(svs), ptr(table), ptr(bg_row), ptr(out), svs.numel(), table.shape[0], row_bytes,
        current_stream())), "gts_project_rows_i16")
    return out


def _check_relabel(relabel, n_classes):
    if relabel is not None and (relabel.dtype != torch.int16 or relabel.numel() < n_classes):
        raise _lib.GtsError("relabel must be int16 with one entry per class")


def project_argmax(svs, logits, relabel=None):
    """K12 fused: argmax over classes of the voxel's node, 0 for background; int16 out."""
    f32(logits)
    if svs.dtype != torch.int16:
        raise _lib.GtsError("supervoxel partitioning must be int16")
    svs, logits = svs.contiguous(), logits.contiguous()
    require_device(svs, logits, relabel)
    _check_relabel(relabel, logits.shape[1])
    out = torch.empty(svs.shape, dtype=torch.int16, device=svs.device)
    if svs.numel() == 0:
        return out
    check(_lib.load().gts_project_argmax_i16(ptr(svs), ptr(logits), ptr(relabel), ptr(out), svs.numel(),
                                             logits.shape[0], logits.shape[1], current_stream()),
          "gts_project_argmax_i16")
    return out


def project_argmax_occupancy(svs, logits):
    """K12 arg-max projection of a 3-D partitioning plus the tumour-plane flags of the result:
    (int16 labels [X,Y,Z], (any over (y,z) [X], any over (x,z) [Y], any over (x,y) [Z]) as uint8)."""
    f32(logits)
    if svs.dtype != torch.int16 or svs.dim() != 3:
        raise _lib.GtsError("supervoxel partitioning must be a 3-D int16 volume")
    svs, logits = svs.contiguous(), logits.contiguous()
    require_device(svs, logits)
    dx, dy, dz = svs.shape
    out = torch.empty(svs.shape, dtype=torch.int16, device=svs.device)
    occ = torch.zeros(dx + dy + dz, dtype=torch.uint8, device=svs.device)
    if svs.numel():
        check(_lib.load().gts_project_argmax_occupancy_i16(ptr(svs), ptr(logits), ptr(out), ptr(occ), dx, dy, dz,
                                                           logits.shape[0], logits.shape[1], current_stream()),
              "gts_project_argmax_occupancy_i16")
    return out, (occ[:dx], occ[dx:dx + dy], occ[dx + dy:])


class CropBox:
    """Outer product of three ascending plane-index vectors (what np.ix_ of boolean plane masks
    selects) inside a [X, Y, Z] volume; validated on the host, kept as int32 on the device."""

    def __init__(self, xs, ys, zs, volume_shape, device):
        import numpy as np

        self.volume_shape = tuple(int(d) for d in volume_shape)
        self.host = []
        for idx, extent in zip((xs, ys, zs), self.volume_shape):
            idx = np.asarray(idx).reshape(-1).astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= extent or np.any(np.diff(idx) <= 0)):
                raise _lib.GtsError("crop indices must be strictly ascending and inside the volume")
            self.host.append(idx)
        self.shape = tuple(len(i) for i in self.host)
        self.dev = [torch.from_numpy(i.astype(np.int32)).to(device) for i in self.host]
        self.device = device
        self._inverse_dev = None

    def as_ix(self):
        import numpy as np

        return np.ix_(*self.host)

    def inverse_host(self):
        """Per axis, int32 [extent]: plane index of the volume -> its index inside the crop, -1 for a plane
        outside it (what the adjoint of crop_concat_rows reads)."""
        import numpy as np

        tables = []
        for idx, extent in zip(self.host, self.volume_shape):
            inv = np.full(extent, -1, dtype=np.int32)
            inv[idx] = np.arange(len(idx), dtype=np.int32)
            tables.append(inv)
        return tables

    def inverse_dev(self):
        if self._inverse_dev is None:
            self._inverse_dev = [torch.from_numpy(t).to(self.device) for t in self.inverse_host()]
        return self._inverse_dev


def supervoxel_voxel_lists(svs, n_rows):
    """(list_ptr int32 [n_rows + 1], list_vox int32) of a partitioning [X, Y, Z] (integer array on the host):
    for every table row n the C-order linear indices of the voxels whose id resolves to n, ascending.  An id
    resolves as numpy indexes `table_plus_bg[id]` (negative ids wrap over n_rows + 1 rows); voxels that take
    the background row, or an id outside the table, are in no list.  Independent of any crop box."""
    import numpy as np

    ids = np.asarray(svs).reshape(-1).astype(np.int64)
    if ids.size >= 2 ** 31:
        raise _lib.GtsError("partitioning too large for int32 voxel indices")
    rows = np.where(ids < 0, ids + n_rows + 1, ids)
    vox = np.flatnonzero((rows >= 0) & (rows < n_rows))
    order = np.argsort(rows[vox], kind="stable")          # stable: raster order inside every row
    counts = np.bincount(rows[vox], minlength=n_rows)[:n_rows] if n_rows else np.zeros(0, dtype=np.int64)
    list_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return list_ptr, vox[order].astype(np.int32)


class SupervoxelLists:
    """One sample's device-resident partitioning (`svs`, int16 [X, Y, Z]) together with its
    supervoxel_voxel_lists for `n_rows` table rows: built once per sample, J2 reads the lists for every box.
    A tensor already on `device` is kept as it is (contiguous), anything else is uploaded."""

    def __init__(self, svs, n_rows, device):
        import numpy as np

        host = svs.detach().cpu().numpy() if isinstance(svs, torch.Tensor) else np.ascontiguousarray(svs)
        if host.ndim != 3 or host.dtype != np.int16:
            raise _lib.GtsError("supervoxel partitioning must be a 3-D int16 volume")
        on_device = isinstance(svs, torch.Tensor) and svs.device == torch.device(device) and svs.is_contiguous()
        self.svs = svs if on_device else torch.from_numpy(host).to(device)
        self.volume_shape = tuple(int(d) for d in host.shape)
        self.n_rows = int(n_rows)
        list_ptr, list_vox = supervoxel_voxel_lists(host, self.n_rows)
        self.list_ptr = torch.from_numpy(list_ptr).to(device)
        # never empty, so the pointer handed to the kernel is valid
        self.list_vox = torch.from_numpy(list_vox).to(device) if list_vox.size else \
            torch.zeros(1, dtype=torch.int32, device=device)


def _crop_operands(img, svs, table, bg_row, box, what):
    """The operand checks of crop_concat (K16) and crop_concat_rows (J1); returns (img, svs, table, bg_row, ci, ct),
    contiguous."""
    f32(img, table, bg_row)
    if svs.dtype != torch.int16 or tuple(svs.shape) != box.volume_shape:
        raise _lib.GtsError("partitioning must be int16 with the crop box's volume shape")
    ci = 0
    if img is not None:
        if img.dim() != 4 or tuple(img.shape[:3]) != box.volume_shape:
            raise _lib.GtsError("image must be [X, Y, Z, C] over the same volume")
        img, ci = img.contiguous(), img.shape[3]
    if table.dim() != 2:
        raise _lib.GtsError(f"{what}: table must be [N, C], got {tuple(table.shape)}")
    ct = table.shape[1]
    if bg_row.numel() != ct:
        raise _lib.GtsError("background row does not match table rows")
    svs, table, bg_row = svs.contiguous(), table.contiguous(), bg_row.contiguous()
    require_device(svs, table, bg_row, img, *box.dev)
    return img, svs, table, bg_row, ci, ct


def crop_concat_rows(img, svs, table, bg_row, box):
    """J1.  [cx, cy, cz, Ci + Ct] fp32 = cat([img, table_plus_bg[svs]], -1)[box], channels-last (what
    gts.conv3d reads); the same values as crop_concat(...)[0].movedim(0, -1).  Operands as crop_concat."""
    img, svs, table, bg_row, ci, ct = _crop_operands(img, svs, table, bg_row, box, "crop_concat_rows")
    cx, cy, cz = box.shape
    out = torch.empty((cx, cy, cz, ci + ct), dtype=torch.float32, device=svs.device)
    if out.numel():
        check(_lib.load().gts_crop_concat_rows_f32(ptr(img), ptr(svs), ptr(table), ptr(bg_row), ptr(box.dev[0]),
                                                   ptr(box.dev[1]), ptr(box.dev[2]), ptr(out), cx, cy, cz,
                                                   box.volume_shape[1], box.volume_shape[2], table.shape[0], ci, ct,
                                                   current_stream()), "gts_crop_concat_rows_f32")
    return out


def _rows_over_box(t, dims, what, min_cols=0):
    """t fp32 [V, K] or [cx, cy, cz, K] over a crop of extents dims (V = cx cy cz), K >= min_cols: its [V, K] view."""
    f32(t)
    cx, cy, cz = (int(d) for d in dims)
    v = cx * cy * cz
    if t.dim() == 4 and tuple(t.shape[:3]) == (cx, cy, cz):
        t = t.reshape(v, t.shape[3])
    if t.dim() != 2 or t.shape[0] != v or t.shape[1] < min_cols:
        raise _lib.GtsError(f"{what}: expected [{v}, K] or [{cx}, {cy}, {cz}, K] over the crop box with K >= {min_cols}, "
                            f"got {tuple(t.shape)}")
    return t


def crop_concat_rows_bwd(dx, lists, box, img_channels=0):
    """J2, the adjoint of crop_concat_rows with respect to `table`: d_table [N, Ct] from dx [V, Ci + Ct] (or
    [cx, cy, cz, Ci + Ct]) over the crop, Ci = img_channels (0 when dx holds the table's columns only).
    `lists`: the SupervoxelLists of the partitioning for N rows.  Deterministic (fixed-order sums)."""
    if img_channels < 0:
        raise _lib.GtsError(f"crop_concat_rows_bwd: {img_channels} image channels")
    dx = _rows_over_box(dx, box.shape, "crop_concat_rows_bwd", img_channels + 1)
    cx, cy, cz = box.shape
    if not isinstance(lists, SupervoxelLists) or lists.volume_shape != box.volume_shape:
        raise _lib.GtsError("crop_concat_rows_bwd: the voxel lists belong to another volume")
    dx = dx.contiguous()
    inv = box.inverse_dev()
    require_device(dx, lists.list_ptr, lists.list_vox, *inv)
    ct = dx.shape[1] - img_channels
    out = torch.empty((lists.n_rows, ct), dtype=torch.float32, device=dx.device)
    if out.numel():
        dim_x, dim_y, dim_z = box.volume_shape
        check(_lib.load().gts_crop_concat_rows_bwd_f32(ptr(dx), ptr(lists.list_ptr), ptr(lists.list_vox), ptr(inv[0]),
                                                       ptr(inv[1]), ptr(inv[2]), ptr(out), cx, cy, cz, dim_x, dim_y,
                                                       dim_z, lists.n_rows, img_channels, ct, current_stream()),
              "gts_crop_concat_rows_bwd_f32")
    return out


def crop_concat(img, svs, table, bg_row, box):
    """K16.  [1, Ci + Ct, cx, cy, cz] fp32 = cat([img, table_plus_bg[svs]], -1)[box] moved to
    channels-first, without materialising the voxel-logit volume.  img [X,Y,Z,Ci] fp32 (or None),
    svs [X,Y,Z] int16, table [N,Ct] fp32, bg_row [Ct]."""
    img, svs, table, bg_row, ci, ct = _crop_operands(img, svs, table, bg_row, box, "crop_concat")
    cx, cy, cz = box.shape
    out = torch.empty((1, ci + ct, cx, cy, cz), dtype=torch.float32, device=svs.device)
    if out.numel():
        check(_lib.load().gts_crop_concat_f32(ptr(img), ptr(svs), ptr(table), ptr(bg_row), ptr(box.dev[0]),
                                              ptr(box.dev[1]), ptr(box.dev[2]), ptr(out), cx, cy, cz,
                                              box.volume_shape[1], box.volume_shape[2], table.shape[0], ci, ct,
                                              current_stream()), "gts_crop_concat_f32")
    return out


def argmax_scatter(scores, box, relabel=None):
    """K17.  int16 [X,Y,Z] volume, zero outside the box, arg-max over channels of
    scores [C, cx, cy, cz] (or [1, C, ...]) inside."""
    f32(scores)
    if scores.dim() == 5 and scores.shape[0] == 1:
        scores = scores[0]
    if scores.dim() != 4 or tuple(scores.shape[1:]) != box.shape:
        raise _lib.GtsError("scores must be [C, cx, cy, cz] over the crop box")
    scores = scores.contiguous()
    require_device(scores, relabel, *box.dev)
    _check_relabel(relabel, scores.shape[0])
    out = torch.zeros(box.volume_shape, dtype=torch.int16, device=scores.device)
    cx, cy, cz = box.shape
    if scores.numel():
        check(_lib.load().gts_argmax_scatter_i16(ptr(scores), ptr(relabel), ptr(box.dev[0]), ptr(box.dev[1]),
                                                 ptr(box.dev[2]), ptr(out), cx, cy, cz, box.volume_shape[1],
                                                 box.volume_shape[2], scores.shape[0], current_stream()),
              "gts_argmax_scatter_i16")
    return out


def argmax_scatter_rows(scores, box, relabel=None):
    """E2.  K17 for channels-last scores: int16 [X,Y,Z] volume, zero outside the box, first-maximum arg-max over
    the columns of scores [cx * cy * cz, C] (or [cx, cy, cz, C]) inside."""
    cx, cy, cz = box.shape
    scores = _rows_over_box(scores, box.shape, "argmax_scatter_rows", 1).contiguous()
    require_device(scores, relabel, *box.dev)
    _check_relabel(relabel, scores.shape[1])
    out = torch.zeros(box.volume_shape, dtype=torch.int16, device=scores.device)
    if scores.numel():
        check(_lib.load().gts_argmax_scatter_rows_i16(ptr(scores), ptr(relabel), ptr(box.dev[0]), ptr(box.dev[1]),
                                                      ptr(box.dev[2]), ptr(out), cx, cy, cz, box.volume_shape[1],
                                                      box.volume_shape[2], scores.shape[1], current_stream()),
              "gts_argmax_scatter_rows_i16")
    return out


SOFTMAX_ACCUMULATE_MAX_CLASSES = 8


def softmax_accumulate(logit_sets, acc=None):
    """E1.  acc [rows, C] fp32 (+)= the sum over the tensors of `logit_sets` (each [rows, C] fp32, 1 <= C <= 8) of
    their row softmax, added in list order with plain fp32 adds: splitting the list over several calls gives the
    same bits.  acc None: a fresh tensor that starts from zero; otherwise acc is added onto in place.  Returns acc
    (the SUM: divide by the number of sets for the mean)."""
    logit_sets = list(logit_sets)
    if not logit_sets:
        raise _lib.GtsError("softmax_accumulate: no logit sets")
    f32(acc, *logit_sets)
    first = logit_sets[0]
    if first.dim() != 2 or not 1 <= first.shape[1] <= SOFTMAX_ACCUMULATE_MAX_CLASSES:
        raise _lib.GtsError(f"softmax_accumulate: logits must be [rows, 1..{SOFTMAX_ACCUMULATE_MAX_CLASSES}], "
                            f"got {tuple(first.shape)}")
    for t in logit_sets[1:]:
        expect(t, first.shape, "softmax_accumulate logits")
    expect(acc, first.shape, "softmax_accumulate acc")
    require_device(acc, *logit_sets)
    overwrite = acc is None
    if overwrite:
        acc = torch.empty_like(first)
    elif any(t.data_ptr() == acc.data_ptr() for t in logit_sets):
        raise _lib.GtsError("softmax_accumulate: acc must not be one of the logit sets")
    if first.numel():
        pointers = (ctypes.c_void_p * len(logit_sets))(*[t.data_ptr() for t in logit_sets])
        check(_lib.load().gts_softmax_accumulate_f32(pointers, len(logit_sets), ptr(acc), first.shape[0],
                                                     first.shape[1], int(overwrite), current_stream()),
              "gts_softmax_accumulate_f32")
    return acc


UNCERTAINTY_BINS = _lib.const("GTS_UNCERTAINTY_BINS")
UNCERTAINTY_CLASSES = 4     # the internal labels 0 healthy, 1 edema, 2 NET, 3 ET: the regions are sets of them


def _uncertainty_sums(total, terms, what):
    f32(total)
    if total.dim() < 1 or total.shape[-1] != UNCERTAINTY_CLASSES:
        raise _lib.GtsError(f"{what}: the class sums must have {UNCERTAINTY_CLASSES} columns, got "
                            f"{tuple(total.shape)}")
    if int(terms) != terms or not 1 <= terms <= 2 ** 31:
        raise _lib.GtsError(f"{what}: terms must be a whole number in 1..2^31, got {terms!r}")
    return int(terms)


def region_uncertainty_rows(total, terms, box):
    """U1.  uint8 [3, X, Y, Z] (WT, CT, ET), zero outside the box: the QU-BraTS style uncertainty 0..100 of the
    class sums `total` [cx * cy * cz, 4] (or [cx, cy, cz, 4]) that softmax_accumulate left over `terms` softmaxes
    (the SUM, before any division).  DESIGN.md 4u has the formula; it equals the numpy expression bit for bit."""
    terms = _uncertainty_sums(total, terms, "region_uncertainty_rows")
    total = _rows_over_box(total, box.shape, "region_uncertainty_rows", UNCERTAINTY_CLASSES).contiguous()
    require_device(total, *box.dev)
    out = torch.zeros((3,) + tuple(box.volume_shape), dtype=torch.uint8, device=total.device)
    cx, cy, cz = box.shape
    if total.numel():
        check(_lib.load().gts_region_uncertainty_rows_u8(ptr(total), ptr(box.dev[0]), ptr(box.dev[1]),
                                                         ptr(box.dev[2]), ptr(out), cx, cy, cz, *box.volume_shape,
                                                         total.shape[1], terms, current_stream()),
              "gts_region_uncertainty_rows_u8")
    return out


def region_uncertainty_nodes(svs, total, terms):
    """U1n.  uint8 [3, *svs.shape]: the uncertainty of the node class sums `total` [N, 4] (over `terms` members)
    at every voxel's node, ids resolved as project_argmax resolves them; background voxels get 0."""
    terms = _uncertainty_sums(total, terms, "region_uncertainty_nodes")
    if svs.dtype != torch.int16:
        raise _lib.GtsError("supervoxel partitioning must be int16")
    if total.dim() != 2:
        raise _lib.GtsError(f"region_uncertainty_nodes: the class sums must be [N, 4], got {tuple(total.shape)}")
    svs, total = svs.contiguous(), total.contiguous()
    require_device(svs, total)
    out = torch.empty((3,) + tuple(svs.shape), dtype=torch.uint8, device=svs.device)
    if svs.numel():
        check(_lib.load().gts_region_uncertainty_nodes_u8(ptr(svs), ptr(total), ptr(out), svs.numel(),
                                                          total.shape[0], total.shape[1], terms, current_stream()),
              "gts_region_uncertainty_nodes_u8")
    return out


def uncertainty_histogram(pred, truth, unc):
    """U2.  int64 [3, 4, 102] on the device: per region (WT, CT, ET) and outcome (TP, FP, FN, TN of the region
    masks of pred / truth, int16 internal labels 0..3) the number of voxels at each value 0..100 of the region's
    map unc[r] (uint8 [3, ...] over the same voxels); the last bin stays 0.  A map value above 100 or a label
    outside 0..3 raises GtsError (after the one pass that finds it)."""
    if pred.dtype != torch.int16 or truth.dtype != torch.int16:
        raise _lib.GtsError("uncertainty_histogram takes int16 labels")
    if unc.dtype != torch.uint8:
        raise _lib.GtsError(f"uncertainty_histogram takes uint8 maps, got {unc.dtype}")
    n = pred.numel()
    if truth.numel() != n:
        raise _lib.GtsError(f"uncertainty_histogram: {n} predictions vs {truth.numel()} labels")
    if unc.dim() < 1 or unc.shape[0] != 3 or unc.numel() != 3 * n:
        raise _lib.GtsError(f"uncertainty_histogram: the maps must be [3, {n} voxels], got {tuple(unc.shape)}")
    pred, truth, unc = pred.contiguous(), truth.contiguous(), unc.contiguous()
    require_device(pred, truth, unc)
    hist = torch.zeros((4, 4, UNCERTAINTY_BINS), dtype=torch.int64, device=pred.device)
    if n:
        check(_lib.load().gts_uncertainty_histogram(ptr(pred), ptr(truth), ptr(unc), ptr(hist), n, current_stream()),
              "gts_uncertainty_histogram")
    host = hist.cpu()
    if int(host[3, 0, 0]):
        raise _lib.GtsError(f"uncertainty_histogram: {int(host[3, 0, 0])} voxel(s) carry a label outside 0..3")
    if int(host[:3, :, UNCERTAINTY_BINS - 1].sum()):
        raise _lib.GtsError("uncertainty_histogram: the maps hold values above 100")
    return hist[:3]


def label_confusion(pred, truth):
    """K15.  int64 [5, 5] table on the device: entry [cp, ct] counts the positions where the
    predicted label has class cp and the true label class ct (class = label for 0..3, 4 for
    anything else).  pred / truth: int16 tensors of equal size."""
    if pred.dtype != torch.int16 or truth.dtype != torch.int16:
        raise _lib.GtsError("label_confusion takes int16 labels")
    if pred.numel() != truth.numel():
        raise _lib.GtsError(f"label_confusion: {pred.numel()} predictions vs {truth.numel()} labels")
    pred, truth = pred.contiguous(), truth.contiguous()
    require_device(pred, truth)
    counts = torch.zeros((5, 5), dtype=torch.int64, device=pred.device)
    if pred.numel():
        lib = _lib.load()
        ws = scratch(lib.gts_label_confusion_workspace(pred.numel()), pred.device, torch.uint8)
        check(lib.gts_label_confusion_i16(ptr(pred), ptr(truth), ptr(counts), ptr(ws), ws.numel(),
                                          pred.numel(), current_stream()), "gts_label_confusion_i16")
    return counts


# ---------------------------------------------------------------- class-weighted cross-entropy
def _weighted_ce_launch(logits, labels, class_w, want_grad):
    """The one gts_weighted_ce_f32 launch: (grad_unscaled [N, C] or None, stats = [num, den, num/den])."""
    logits, labels = logits.contiguous(), labels.contiguous()
    f32(logits, class_w)
    require_device(logits, labels, class_w)
    if logits.dim() != 2 or labels.dtype != torch.int64 or labels.shape != logits.shape[:1]:
        raise _lib.GtsError("weighted CE takes logits [N, C] and int64 labels [N]")
    n, c = logits.shape
    expect(class_w, (c,), "class_w")
    lib = _lib.load()
    ws = scratch(lib.gts_weighted_ce_workspace(n), logits.device)
    grad = torch.empty_like(logits) if want_grad else None
    stats = torch.empty(3, dtype=torch.float32, device=logits.device)
    check(lib.gts_weighted_ce_f32(ptr(logits), ptr(labels), ptr(class_w), ptr(grad), ptr(ws), ws.numel() * 4,
                                  ptr(stats), n, c, current_stream()), "gts_weighted_ce_f32")
    return grad, stats


class _WeightedCE(torch.autograd.Function):
    """(logits [N,C], labels int64 [N], class_w [C] or None) -> stats = [num, den, num/den]."""

    @staticmethod
    def forward(ctx, logits, labels, class_w):
        grad, stats = _weighted_ce_launch(logits, labels, class_w, ctx.needs_input_grad[0])
        ctx.save_for_backward(grad, stats)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)                 # an unused output arrives as None, not as a zero tensor
        return stats[2].clone(), stats[0].clone(), stats

    @staticmethod
    def backward(ctx, g_mean, g_sum, _g_stats):
        grad_unscaled, stats = ctx.saved_tensors
        # d(num)/dx = gu ; d(num/den)/dx = gu / den
        if g_mean is None and g_sum is None:
            return None, None, None
        if g_sum is None:
            scale = g_mean / stats[1]
        elif g_mean is None:
            scale = g_sum
        else:
            scale = g_sum + g_mean / stats[1]
        return grad_unscaled * scale, None, None


def weighted_cross_entropy(logits, labels, class_w=None, reduction="mean"):
    """F.cross_entropy(logits, labels, weight=class_w, reduction=...) as one fused HIP pass.
    'mean' is the weighted mean (sum_i w[y_i] nll_i / sum_i w[y_i]), 'sum' the numerator."""
    mean, total, _ = _WeightedCE.apply(logits, labels, class_w)
    if reduction == "mean":
        return mean
    if reduction == "sum":
        return total
    raise ValueError(reduction)


# ---------------------------------------------------------------- soft Dice + class-weighted cross-entropy
DICE_MAX_GROUPS = _lib.const("GTS_DICE_CE_MAX_GROUPS")
DICE_STATS_FLOATS = _lib.const("GTS_DICE_CE_STATS_FLOATS")
_DICE_LOSS, _DICE_CE, _DICE_LDICE, _DICE_DICE = (_lib.const("GTS_DICE_CE_STATS_" + part)
                                                 for part in ("LOSS", "CE", "LDICE", "DICE"))


def dice_region_masks(regions, n_classes):
    """Bitmasks over the classes of a named region set or of a sequence of class-index sequences.
    "brats": WT {1,2,3}, CT {2,3}, ET {3} of the internal labels (needs 4 classes); "classes": one region per
    class 1..C-1, background left out."""
    if isinstance(regions, str):
        if regions == "brats":
            if n_classes != 4:
                raise _lib.GtsError(f'regions "brats" are sets of the 4 internal labels: got {n_classes} classes')
            regions = ((1, 2, 3), (2, 3), (3,))
        elif regions == "classes":
            regions = tuple((c,) for c in range(1, n_classes))
        else:
            raise _lib.GtsError(f'unknown region set "{regions}": "brats", "classes" or a sequence of class sets')
    masks = []
    for members in regions:
        members = [int(c) for c in members]
        if not members or min(members) < 0 or max(members) >= n_classes:
            raise _lib.GtsError(f"a Dice region is a non-empty set of classes in [0, {n_classes}): got {members}")
        masks.append(sum(1 << c for c in set(members)))
    if not 1 <= len(masks) <= DICE_MAX_GROUPS:
        raise _lib.GtsError(f"1 to {DICE_MAX_GROUPS} Dice regions, got {len(masks)}")
    return tuple(masks)


class _DiceCE(torch.autograd.Function):
    """(logits [N,C], labels int64 [N], class_w [C] or None, region masks, weights) -> (loss, stats [40]).
    The forward runs the statistics pass (D1) alone; the gradient pass (D2) is launched from backward, takes the
    upstream gradient as a device scalar and writes the final gradient once."""

    @staticmethod
    def forward(ctx, logits, labels, class_w, masks, ce_weight, dice_weight, smooth):
        logits, labels = logits.contiguous(), labels.contiguous()
        f32(logits, class_w)
        require_device(logits, labels, class_w)
        if logits.dim() != 2 or labels.dtype != torch.int64 or labels.shape != logits.shape[:1]:
            raise _lib.GtsError("Dice + CE takes logits [N, C] and int64 labels [N]")
        n, c = logits.shape
        expect(class_w, (c,), "class_w")
        lib = _lib.load()
        host_masks = (ctypes.c_uint32 * len(masks))(*masks)
        ws = scratch(lib.gts_dice_ce_workspace(n, len(masks)), logits.device)
        stats = torch.empty(DICE_STATS_FLOATS, dtype=torch.float32, device=logits.device)
        check(lib.gts_dice_ce_fwd_f32(ptr(logits), ptr(labels), ptr(class_w), host_masks, len(masks), ce_weight,
                                      dice_weight, smooth, ptr(stats), ptr(ws), ws.numel() * 4, n, c,
                                      current_stream()), "gts_dice_ce_fwd_f32")
        ctx.save_for_backward(logits, labels, class_w, stats)
        ctx.terms = (host_masks, len(masks), ce_weight, dice_weight, smooth)
        ctx.mark_non_differentiable(stats)
        return stats[_DICE_LOSS].clone(), stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_stats):
        logits, labels, class_w, stats = ctx.saved_tensors
        host_masks, n_groups, ce_weight, dice_weight, smooth = ctx.terms
        scale = g_loss.to(torch.float32).contiguous()
        grad = torch.empty_like(logits)
        check(_lib.load().gts_dice_ce_bwd_f32(ptr(logits), ptr(labels), ptr(class_w), host_masks, n_groups,
                                              ce_weight, dice_weight, smooth, ptr(stats), ptr(scale), ptr(grad),
                                              logits.shape[0], logits.shape[1], current_stream()),
              "gts_dice_ce_bwd_f32")
        return grad, None, None, None, None, None, None


def dice_ce_loss(logits, labels, class_w=None, *, regions="brats", ce_weight=1.0, dice_weight=1.0, smooth=1.0,
                 return_parts=False):
    """ce_weight * weighted cross-entropy + dice_weight * (1 - mean soft Dice over `regions`) of voxel logits
    [N, C] against int64 labels [N], as two fused HIP passes.  Rows labelled -100 are ignored.
    regions: "brats", "classes" or a sequence of class-index sequences (dice_region_masks).  A term of weight 0
    is skipped.  return_parts: also a tensor [CE, L_dice, dice_0 .. dice_{G-1}] that carries no gradient."""
    ce_weight, dice_weight, smooth = float(ce_weight), float(dice_weight), float(smooth)
    if logits.dim() != 2:
        raise _lib.GtsError("Dice + CE takes logits [N, C] and int64 labels [N]")
    masks = dice_region_masks(regions, logits.shape[1])
    loss, stats = _DiceCE.apply(logits, labels, class_w, masks, ce_weight, dice_weight, smooth)
    if not return_parts:
        return loss
    return loss, torch.cat([stats[_DICE_CE:_DICE_LDICE + 1], stats[_DICE_DICE:_DICE_DICE + len(masks)]])


# ---------------------------------------------------------------- training-time augmentation
def _matrix_arg(matrix):
    """The plan's float64 [3, 3] matrix as the 9 host doubles A3 / A4 read during the call."""
    return (ctypes.c_double * 9)(*(float(m) for m in matrix.reshape(-1)))


def _crop_augment(x, labels, dims, image_channels, params, flip_mask, seed, step, what, matrix=None):
    """One A1 launch (A3 with a matrix) on x [cx, cy, cz, C] and / or labels [V]; returns fresh tensors (None where
    the input is)."""
    cx, cy, cz = (int(d) for d in dims)
    f32(x, params)
    require_device(x, labels, params)
    channels = 0
    if x is not None:
        if x.dim() != 4 or tuple(x.shape[:3]) != (cx, cy, cz):
            raise _lib.GtsError(f"{what}: expected x [{cx}, {cy}, {cz}, C], got {tuple(x.shape)}")
        channels = x.shape[3]
    if labels is not None and (labels.dtype != torch.int64 or labels.numel() != cx * cy * cz):
        raise _lib.GtsError(f"{what}: labels must be int64 with {cx * cy * cz} entries")
    x_out = torch.empty_like(x) if x is not None else None
    labels_out = torch.empty_like(labels) if labels is not None else None
    if x is None and labels is None:
        raise _lib.GtsError(f"{what}: nothing to do without x and without labels")
    if cx * cy * cz and matrix is None:
        check(_lib.load().gts_augment_crop_f32(ptr(x), ptr(labels), ptr(params), ptr(x_out), ptr(labels_out), cx, cy,
                                               cz, channels, image_channels, flip_mask, seed, step, current_stream()),
              "gts_augment_crop_f32")
    elif cx * cy * cz:
        check(_lib.load().gts_augment_spatial_f32(ptr(x), ptr(labels), ptr(params), _matrix_arg(matrix), ptr(x_out),
                                                  ptr(labels_out), cx, cy, cz, channels, image_channels, flip_mask,
                                                  seed, step, current_stream()),
              "gts_augment_spatial_f32")
    return x_out, labels_out


def augment_crop(x, labels, plan):
    """A1, or A3 when the plan is spatial.  (x', labels') of a cropped sample under a gts.augment.AugmentPlan: x
    [cx, cy, cz, C] fp32 channels-last whose first plan.channels channels are the image modalities (mirrored, x *
    scale + shift + sigma * noise; the other channels are mirrored only), labels int64 [cx * cy * cz] or
    [cx, cy, cz] (mirrored).  A spatial plan (plan.matrix differs from the identity) also rotates and zooms about the
    crop's centre: trilinear with a zero border for x, nearest for the labels (include/gts_hip.h).  Either may be
    None (labels alone must then be 3-D: they carry the extents).  Fresh tensors; not an autograd node."""
    if x is not None:
        dims = tuple(x.shape[:3])
    elif labels is not None and labels.dim() == 3:
        dims = tuple(labels.shape)
    else:
        raise _lib.GtsError("augment_crop: without x the labels must be [cx, cy, cz]")
    params = None
    ci = 0
    if x is not None:
        import numpy as np

        ci = plan.channels
        params = torch.from_numpy(np.stack([plan.scale, plan.shift, plan.sigma], axis=1)).to(x.device)
        x = x.contiguous()
    if labels is not None:
        labels = labels.contiguous()
    matrix = plan.matrix if plan.spatial else None
    return _crop_augment(x, labels, dims, ci, params, plan.flip_mask, plan.seed64, plan.step, "augment_crop", matrix)


def flip_crop(t, dims, flips):
    """A1 without image channels: t [V, K] or [cx, cy, cz, K] fp32 over a crop of extents dims, mirrored along the
    axes whose entry of flips (x, y, z) is true.  An involution and its own adjoint, which is how the joint step
    carries a gradient back through the mirror.  Returns a fresh tensor of t's shape; not an autograd node."""
    cx, cy, cz = (int(d) for d in dims)
    rows = _rows_over_box(t, dims, "flip_crop")
    view = rows.contiguous().view(cx, cy, cz, rows.shape[1])
    flips = tuple(bool(f) for f in flips)
    if len(flips) != 3:
        raise _lib.GtsError("flip_crop: flips are three booleans (x, y, z)")
    mask = sum(1 << a for a in range(3) if flips[a])
    return _crop_augment(view, None, (cx, cy, cz), 0, None, mask, 0, 0, "flip_crop")[0].view(t.shape)


def spatial_crop_bwd(t, dims, plan):
    """A4.  The adjoint of augment_crop's mirror and resample (not of its affine or noise) on t [V, K] or
    [cx, cy, cz, K] fp32, a gradient with respect to the augmented crop of extents dims: what the joint step carries
    back to the node logits.  Deterministic (a gather, float64 sums in a fixed order).  For a plan that is not spatial
    it is flip_crop.  Returns a fresh tensor of t's shape; not an autograd node."""
    if not plan.spatial:
        return flip_crop(t, dims, plan.flips)
    cx, cy, cz = (int(d) for d in dims)
    dy = _rows_over_box(t, dims, "spatial_crop_bwd").contiguous()
    require_device(dy)
    dx = torch.empty_like(dy)
    if dy.numel():
        check(_lib.load().gts_augment_spatial_bwd_f32(ptr(dy), _matrix_arg(plan.matrix), ptr(dx), cx, cy, cz,
                                                      dy.shape[1], plan.flip_mask, current_stream()),
              "gts_augment_spatial_bwd_f32")
    return dx.view(t.shape)


def augment_features(feats, batch_num_nodes, plans):
    """A2.  Node features [N, F] fp32 of a batch of graphs under one gts.augment.AugmentPlan per graph: feature f of a
    row of graph g becomes f * scale[g][m] + shift[g][m] with m = f // (F // M), M the plans' channel count (the five
    quantile columns of a modality move with the modality) plus feature_sigma * noise.  batch_num_nodes: the
    graphs' row counts (graph.batch_num_nodes()).  The noise of the call is keyed by the first plan's seed and step
    and indexed by the row inside the batch.  Returns a NEW tensor: the dataset cache and resident batches keep the
    originals.  Not an autograd node."""
    import numpy as np

    sizes = np.asarray(batch_num_nodes.cpu() if isinstance(batch_num_nodes, torch.Tensor) else batch_num_nodes,
                       dtype=np.int64).reshape(-1)
    plans = list(plans)
    if feats.dim() != 2 or len(plans) != len(sizes) or not plans:
        raise _lib.GtsError("augment_features takes features [N, F] and one plan per graph")
    f32(feats)
    feats = feats.contiguous()
    require_device(feats)
    modalities = plans[0].channels
    if any(p.channels != modalities or p.feature_sigma != plans[0].feature_sigma for p in plans):
        raise _lib.GtsError("augment_features: the plans of one batch share the channel count and the feature sigma")
    row_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    params = np.stack([np.stack([p.scale, p.shift], axis=1) for p in plans]).astype(np.float32)
    out = torch.empty_like(feats)
    n, f = feats.shape
    row_ptr_dev = torch.from_numpy(row_ptr).to(feats.device)
    params_dev = torch.from_numpy(params).to(feats.device)
    check(_lib.load().gts_augment_features_f32(ptr(feats), ptr(row_ptr_dev), row_ptr.ctypes.data, ptr(params_dev),
                                               ptr(out), n, f, modalities, len(sizes), plans[0].feature_sigma,
                                               plans[0].seed64, plans[0].step, current_stream()),
          "gts_augment_features_f32")
    return out


def weighted_ce_numerator_grad(logits, labels, class_w=None):
    """(d numerator / d logits [N, C], [num, den, num/den]) from one launch, outside autograd: what the
    data-parallel step back-propagates with `logits.backward(grad)` — no clone / fill / scale kernels around
    the loss (the normalisation by the GLOBAL denominator happens after the all-reduce)."""
    return _weighted_ce_launch(logits.detach(), labels, class_w, True)


def weighted_cross_entropy_stats(logits, labels, class_w=None):
    """(numerator, [num, den, num/den]) — the numerator carries the gradient (used by the
    data-parallel step, which normalises by the global denominator after the all-reduce)."""
    _, total, stats = _WeightedCE.apply(logits, labels, class_w)
    return total, stats


# ---------------------------------------------------------------- co-registration
REGISTER_MAX_MATRICES = _lib.const("GTS_REGISTER_MAX_MATRICES")
REGISTER_BINS = (16, 32, 64)
RESAMPLE_AUTO, RESAMPLE_PLAIN, RESAMPLE_TILED = 0, 1, 2


def _matrices_arg(matrices, what):
    """Row-major 3 x 4 (or 4 x 4, last row dropped) float64 matrices as the host doubles R1 / R2 read: [K, 12]."""
    import numpy as np

    m = np.asarray(matrices, dtype=np.float64)
    if m.ndim >= 2 and m.shape[-2:] == (4, 4):
        m = m[..., :3, :]
    if m.size == 0 or m.size % 12 or not np.all(np.isfinite(m)):
        raise _lib.GtsError(f"{what} takes finite 3 x 4 matrices, got an array of shape {m.shape}")
    return np.ascontiguousarray(m.reshape(-1, 12))


def affine_resample(volume, matrix, out_shape, out=None, path=RESAMPLE_AUTO):
    """R1.  float32 [OZ, OY, OX]: `volume` ([Z, Y, X] int16 or float32, x fastest) sampled trilinearly where the 3 x 4
    float64 `matrix` sends the output voxel index (x, y, z); 0 outside (include/gts_hip.h).  out_shape = (OX, OY, OZ).
    out: a contiguous float32 tensor of that shape to write (a channel slice of a scan).  path: RESAMPLE_AUTO, or one
    of the two lane maps forced (same bits)."""
    code, z, y, x = scan_volume(volume, "affine_resample")
    ox, oy, oz = (int(n) for n in out_shape)
    m = _matrices_arg(matrix, "affine_resample")
    if len(m) != 1:
        raise _lib.GtsError(f"affine_resample takes one matrix, got {len(m)}")
    out = float32_out(out, (oz, oy, ox), volume)
    check(_lib.load().gts_affine_resample(ptr(volume), code, x, y, z, m.ctypes.data, ox, oy, oz, ptr(out), int(path),
                                          current_stream()), "gts_affine_resample")
    return out


def joint_histogram(fixed, moving, matrices, stride, bins, ranges, grid_blocks=0):
    """R2.  int64 [K, bins * bins + 1] on the device: for each of the K 3 x 4 float64 `matrices` (fixed voxel index ->
    moving voxel coordinates) the joint histogram of `fixed` (float32 [FZ, FY, FX]) and the trilinearly sampled
    `moving` ([Z, Y, X] int16 or float32) over the fixed voxels whose indices are multiples of `stride`; the last entry
    of a row counts the samples outside the moving volume.  ranges = (lo_f, scale_f, lo_m, scale_m): bin = clamp(floor(
    (v - lo) * scale), 0, bins - 1), a non-finite value goes to bin 0.  grid_blocks: workgroups (0: the library's
    choice); the counts do not depend on it."""
    code, z, y, x = scan_volume(moving, "joint_histogram")
    if not isinstance(fixed, torch.Tensor) or fixed.dim() != 3 or fixed.numel() == 0:
        raise _lib.GtsError("joint_histogram takes a non-empty fixed volume [FZ, FY, FX]")
    f32(fixed)
    require_device(fixed, moving)
    m = _matrices_arg(matrices, "joint_histogram")
    k = len(m)
    if k > REGISTER_MAX_MATRICES:
        raise _lib.GtsError(f"joint_histogram takes 1..{REGISTER_MAX_MATRICES} matrices, got {k}")
    if int(bins) not in REGISTER_BINS or int(stride) != stride or stride < 1:
        raise _lib.GtsError(f"joint_histogram: bins in {REGISTER_BINS} and a whole stride >= 1, got {bins!r}, {stride!r}")
    lo_f, scale_f, lo_m, scale_m = (float(v) for v in ranges)
    counts = torch.empty((k, int(bins) ** 2 + 1), dtype=torch.int64, device=fixed.device)
    fz, fy, fx = (int(n) for n in fixed.shape)
    check(_lib.load().gts_joint_histogram(ptr(fixed), fx, fy, fz, ptr(moving), code, x, y, z, m.ctypes.data, k,
                                          int(stride), int(bins), lo_f, scale_f, lo_m, scale_m, ptr(counts),
                                          int(grid_blocks), current_stream()), "gts_joint_histogram")
    return counts


# ---------------------------------------------------------------- bias-field correction
BIAS_BINS = _lib.const("GTS_BIAS_BINS")
BIAS_MAX_SPANS = _lib.const("GTS_BIAS_MAX_SPANS")


class BiasTables:
    """The device operands Z2-Z5 share for one volume shape (X, Y, Z) and one lattice set: the B-spline weights and
    cells of every axis index at every level (float64 / int32 arrays laid out as include/gts_hip.h says; gts.bias.tables
    builds them), per level the fit weights of Z4, and the kernels' workspace."""

    def __init__(self, shape, spans0, levels, weights, cells, fit, device):
        import numpy as np

        self.shape = tuple(int(n) for n in shape)
        self.spans0, self.levels = int(spans0), int(levels)
        if self.spans0 < 1 or self.levels < 1 or self.spans0 << (self.levels - 1) > BIAS_MAX_SPANS:
            raise _lib.GtsError(f"bias lattices: spans0 {spans0} and levels {levels} give more than {BIAS_MAX_SPANS} "
                                "spans, or none")
        total = sum(self.shape)
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1)
        if weights.size != self.levels * 4 * total or cells.size != self.levels * total or len(fit) != self.levels:
            raise _lib.GtsError("bias tables do not match the shape and the number of levels")
        self.ws, _ = workspace(lambda *extents: _lib.load().gts_bias_workspace(*extents, self.spans0 << (self.levels - 1)),
                               *self.shape, device, "bias tables", "extent <= 65535, < 2^31 voxels")
        self.weights = torch.from_numpy(weights).to(device)
        self.cells = torch.from_numpy(cells).to(device)
        self.fit = []
        for f in fit:
            f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
            if f.size != 8 * total:
                raise _lib.GtsError("bias fit weights do not match the shape")
            self.fit.append(torch.from_numpy(f).to(device))
        self.device = self.weights.device

    def points(self, level):
        return (self.spans0 << level) + 3

    def lattice_size(self):
        return sum(self.points(level) ** 3 for level in range(self.levels))

    def lattice_slice(self, level):
        start = sum(self.points(k) ** 3 for k in range(level))
        return slice(start, start + self.points(level) ** 3)


def _bias_operands(u, tables, lattice, what, dtype=torch.float32):
    if not isinstance(u, torch.Tensor) or u.dim() != 3 or tuple(u.shape) != tables.shape[::-1]:
        raise _lib.GtsError(f"{what} takes a [Z, Y, X] tensor of the tables' shape {tables.shape[::-1]}")
    if dtype is not None and u.dtype != dtype:
        raise _lib.GtsError(f"{what}: dtype {u.dtype} is not supported ({dtype})")
    if lattice.dtype != torch.float64 or lattice.numel() != tables.lattice_size():
        raise _lib.GtsError(f"{what} takes the float64 lattices of every level, {tables.lattice_size()} entries")
    require_device(u, lattice, tables.weights)
    x, y, z = tables.shape
    return (x, y, z, ptr(tables.weights), ptr(tables.cells), ptr(lattice), tables.spans0, tables.levels)


def bias_log(volume, threshold=0.0):
    """Z1.  (u, n): u float32 [Z, Y, X] = float32(log(float64(v))) where the volume ([Z, Y, X] int16 or float32) is
    finite and above `threshold` (>= 0), NaN elsewhere; n, an int64 device tensor [1], counts the mask voxels."""
    code, z, y, x = scan_volume(volume, "bias_log")
    u = torch.empty(volume.shape, dtype=torch.float32, device=volume.device)
    count = torch.empty(1, dtype=torch.int64, device=volume.device)
    check(_lib.load().gts_bias_log(ptr(volume), code, x, y, z, float(threshold), ptr(u), ptr(count), current_stream()),
          "gts_bias_log")
    return u, count


def bias_range(u, tables, lattice, grid_blocks=0):
    """Z2.  float64 [2] on the device: min and max of d = float64(u) - field over the mask (the voxels where u is not
    NaN); (+inf, -inf) for an empty mask."""
    args = _bias_operands(u, tables, lattice, "bias_range")
    out = torch.empty(2, dtype=torch.float64, device=u.device)
    check(_lib.load().gts_bias_range(ptr(u), *args, ptr(out), ptr(tables.ws), tables.ws.numel(), int(grid_blocks),
                                     current_stream()), "gts_bias_range")
    return out


def bias_histogram(u, tables, lattice, lo, hi, grid_blocks=0):
    """Z3.  int64 [BIAS_BINS] on the device: the mask voxels by clamp(floor((d - lo) / w + 0.5), 0, BINS - 1), w = (hi -
    lo) / (BINS - 1).  The counts do not depend on grid_blocks."""
    args = _bias_operands(u, tables, lattice, "bias_histogram")
    counts = torch.empty(BIAS_BINS, dtype=torch.int64, device=u.device)
    check(_lib.load().gts_bias_histogram(ptr(u), *args, float(lo), float(hi), ptr(counts), int(grid_blocks),
                                         current_stream()), "gts_bias_histogram")
    return counts


def bias_fit(u, tables, lattice, level, lo, hi, table, grid_blocks=0):
    """Z4.  float64 [3, n, n, n] on the device (n = the level's control points per axis): num, den and delta = num /
    den (0 where den == 0) of the B-spline fit of r = d - E(d) at `level`; `table` holds the BIAS_BINS sharpened values
    E is linear between.  Bit-equal between runs and for every grid_blocks."""
    import numpy as np

    args = _bias_operands(u, tables, lattice, "bias_fit")
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.shape != (BIAS_BINS,) or not 0 <= int(level) < tables.levels:
        raise _lib.GtsError(f"bias_fit takes a table of {BIAS_BINS} values and a level below {tables.levels}")
    n = tables.points(int(level))
    out = torch.empty((3, n, n, n), dtype=torch.float64, device=u.device)
    check(_lib.load().gts_bias_fit(ptr(u), *args, int(level), ptr(tables.fit[int(level)]), float(lo), float(hi),
                                   table.ctypes.data, ptr(out), ptr(tables.ws), tables.ws.numel(), int(grid_blocks),
                                   current_stream()), "gts_bias_fit")
    return out


def bias_mean(u, tables, lattice, grid_blocks=0):
    """Z5.  float64 [3] on the device: the sum of the field over the mask, the mask's size, the mean (0 when empty)."""
    args = _bias_operands(u, tables, lattice, "bias_mean")
    out = torch.empty(3, dtype=torch.float64, device=u.device)
    check(_lib.load().gts_bias_mean(ptr(u), *args, ptr(out), ptr(tables.ws), tables.ws.numel(), int(grid_blocks),
                                    current_stream()), "gts_bias_mean")
    return out


def bias_apply(volume, tables, lattice, mean, want_field=False, out=None, grid_blocks=0):
    """Z5.  float32 [Z, Y, X] = float32(float64(v) / exp(field - mean)) at every voxel of the volume (int16 or float32);
    with want_field also float32(field - mean).  out: a contiguous float32 tensor to write (a channel of a scan)."""
    code = scan_volume(volume, "bias_apply")[0]
    args = _bias_operands(volume, tables, lattice, "bias_apply", dtype=None)
    out = float32_out(out, volume.shape, volume)
    field = torch.empty(volume.shape, dtype=torch.float32, device=volume.device) if want_field else None
    check(_lib.load().gts_bias_apply(ptr(volume), code, *args, float(mean), ptr(out), ptr(field), int(grid_blocks),
                                     current_stream()), "gts_bias_apply")
    return (out, field) if want_field else out


# ---------------------------------------------------------------- brain extraction
BRAIN_BINS = _lib.const("GTS_BRAIN_BINS")
BRAIN_MAX_R2 = _lib.const("GTS_BRAIN_MAX_R2")


def _brain_mask(mask, what):
    """(the int16 mask of three axes on the device, contiguous, its kernels' workspace, the workspace's size)."""
    mask = label_volume(mask, what, three_d=True, noun="masks")
    return (mask,) + workspace(_lib.load().gts_brainmask_workspace, *mask.shape, mask.device, what,
                               "fewer than 2^31 voxels")


def brain_range(volume, grid_blocks=0):
    """S1.  (n, hi): the number of voxels of the volume (int16 or float32, three axes) that are finite and > 0, and
    their maximum as a Python float (0.0 when there is none).  One host synchronisation."""
    import struct

    code, x, y, z = scan_volume(volume, "brain_range")
    out = torch.empty(2, dtype=torch.int64, device=volume.device)
    check(_lib.load().gts_brain_range(ptr(volume), code, x, y, z, ptr(out), int(grid_blocks), current_stream()),
          "gts_brain_range")
    n, bits = out.tolist()
    return int(n), float(struct.unpack("<f", struct.pack("<I", bits))[0])


def brain_histogram(volume, hi, grid_blocks=0):
    """S2.  int64 [BRAIN_BINS] on the device: the finite voxels > 0 by min(BINS - 1, floor(float64(v) / hi * BINS)).
    The counts do not depend on grid_blocks."""
    code, x, y, z = scan_volume(volume, "brain_histogram")
    counts = torch.empty(BRAIN_BINS, dtype=torch.int64, device=volume.device)
    check(_lib.load().gts_brain_histogram(ptr(volume), code, x, y, z, float(hi), ptr(counts), int(grid_blocks),
                                          current_stream()), "gts_brain_histogram")
    return counts


def brain_threshold(volume, t, grid_blocks=0):
    """S2.  (mask int16 0/1 of the volume's shape, count int64 device tensor [1]): finite, > 0 and float64(v) >= t."""
    code, x, y, z = scan_volume(volume, "brain_threshold")
    mask = torch.empty(volume.shape, dtype=torch.int16, device=volume.device)
    count = torch.empty(1, dtype=torch.int64, device=volume.device)
    check(_lib.load().gts_brain_threshold(ptr(volume), code, x, y, z, float(t), ptr(mask), ptr(count), int(grid_blocks),
                                          current_stream()), "gts_brain_threshold")
    return mask, count


def ball_morph(mask, r2, target, outside, invert, grid_blocks=0):
    """S3.  int16 0/1: ((squared distance to the nearest voxel whose value (!= 0) equals `target` <= r2) != invert),
    positions outside the volume counting as `target` iff `outside` (include/gts_hip.h)."""
    mask, ws, size = _brain_mask(mask, "ball_morph")
    if int(r2) != r2 or not 0 <= int(r2) <= BRAIN_MAX_R2:
        raise _lib.GtsError(f"ball_morph: squared radius {r2!r} is outside 0..{BRAIN_MAX_R2}")
    out = torch.empty_like(mask)
    check(_lib.load().gts_ball_morph_i16(ptr(mask), *mask.shape, int(r2), int(bool(target)), int(bool(outside)), ptr(out),
                                         ptr(ws), size, int(bool(invert)), int(grid_blocks), current_stream()),
          "gts_ball_morph_i16")
    return out


def ball_erode(mask, r2, border_value=0, grid_blocks=0):
    """scipy.ndimage.binary_erosion(mask, ball(r2), border_value=border_value) as int16 0/1."""
    return ball_morph(mask, r2, 0, not border_value, True, grid_blocks)


def ball_dilate(mask, r2, grid_blocks=0):
    """scipy.ndimage.binary_dilation(mask, ball(r2)) as int16 0/1."""
    return ball_morph(mask, r2, 1, False, False, grid_blocks)


def largest_component(mask, connectivity=6, grid_blocks=0):
    """S4.  (keep int16 0/1, stats int64 device tensor [5] = components, voxels of the largest, of the second largest,
    the winner's root, voxels of the mask): the component of mask != 0 with the most voxels, a tie going to the smaller root.  An empty
    mask gives an empty keep and zeros; gts.brainmask.largest_component raises for it."""
    mask, ws, size = _brain_mask(mask, "largest_component")
    connectivity = connectivity_arg(connectivity, "largest_component")
    keep = torch.empty_like(mask)
    stats = torch.empty(5, dtype=torch.int64, device=mask.device)
    check(_lib.load().gts_largest_component_i16(ptr(mask), *mask.shape, connectivity, ptr(keep), ptr(stats), ptr(ws),
                                                size, int(grid_blocks), current_stream()), "gts_largest_component_i16")
    return keep, stats


def fill_holes(mask, grid_blocks=0):
    """S5.  (filled int16 0/1, stats int64 device tensor [2] = voxels of the result, voxels filled):
    scipy.ndimage.binary_fill_holes."""
    mask, ws, size = _brain_mask(mask, "fill_holes")
    out = torch.empty_like(mask)
    stats = torch.empty(2, dtype=torch.int64, device=mask.device)
    check(_lib.load().gts_fill_holes_i16(ptr(mask), *mask.shape, ptr(out), ptr(stats), ptr(ws), size, int(grid_blocks),
                                         current_stream()), "gts_fill_holes_i16")
    return out, stats


def apply_mask(scan, mask, grid_blocks=0):
    """S6.  (masked scan of scan's dtype, count int64 device tensor [1]): scan ([C, *mask.shape] or mask's shape, int16
    or float32) where mask != 0, 0 elsewhere (NaN and Inf included)."""
    mask = label_volume(mask, "apply_mask", three_d=True, noun="masks")
    shape = tuple(mask.shape)
    if not isinstance(scan, torch.Tensor) or scan.dtype not in SCAN_CODES:
        raise _lib.GtsError("apply_mask takes an int16 or float32 tensor")
    if tuple(scan.shape[-3:]) != shape or scan.dim() not in (3, 4) or scan.numel() == 0:
        raise _lib.GtsError(f"apply_mask: scan {tuple(scan.shape)} does not lie over the mask {shape}")
    require_device(scan, mask)
    channels = int(scan.shape[0]) if scan.dim() == 4 else 1
    out = torch.empty_like(scan)
    count = torch.empty(1, dtype=torch.int64, device=mask.device)
    check(_lib.load().gts_apply_mask(ptr(scan), SCAN_CODES[scan.dtype], channels, *shape, ptr(mask), ptr(out),
                                     ptr(count), int(grid_blocks), current_stream()), "gts_apply_mask")
    return out, count
