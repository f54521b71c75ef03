"""Cases and references of the plain CSR reducers' edge suite (tests/test_gpu_spmm_edges.py: K1 max forward, K2 max
backward, K3/K4 sum family of csrc/gts_spmm.hip); validated on the CPU by tests/test_spmm_ref_host.py.  Plain numpy: the
only product import is gts.Graph, which builds the CSR arrays on the host.

The references are per-row loops written from the rules below, not from oracle/torch_ref.py (which walks slot by slot
over all rows at once): the host test holds the two against each other bit for bit.

  max      slots in order, strict '<' from -inf: the FIRST maximum wins, a NaN never wins; an empty row or a +-Inf
           maximum gives +0.0 and no winner; with relu_input a maximum that is not > 0 keeps its value, loses its winner.
  max bwd  from +0.0, the gout entries whose recorded slot is this edge's, in out-CSR order, one fp32 add each;
           masked by relu_src > 0.
  sum      from +0.0, neighbours in slot order (each x[u] / div_in[u]), then the self term (x[v] / div_in[v]), then
           / div_out[v], then accum[v] + result; every operation rounded to fp32 once (-ffp-contract=off).
"""
import numpy as np

import gts

# ---------------------------------------------------------------- launch geometry, restated
KWAVE = 64              # csrc/gts_common.h:10
WAVES_PER_BLOCK = 4     # csrc/gts_common.h:11-12 (kBlock / kWave)
UNROLL = 8              # csrc/gts_rows.h:10
# preferred_seq of the three entry points (csrc/gts_spmm.hip:246, :271, :292); 0 = pick_seq's own choice
SEQ_K1, SEQ_K2, SEQ_SUM = 2, 1, 0


def lanes_per_row(vec_cols):
    """csrc/gts_common.h:79-83: smallest power of two >= vec_cols, capped at 64."""
    lanes = 1
    while lanes < 64 and lanes < vec_cols:
        lanes <<= 1
    return lanes


def pick_seq(n_rows, rows_per_wave_step, preferred, rows_per_wave=0):
    """csrc/gts_rows.h:156-164.  rows_per_wave: GTS_OPT_SPMM_ROWS_PER_WAVE (g_spmm_seq), which overrides everything."""
    if rows_per_wave > 0:
        return rows_per_wave
    if preferred > 0:
        return preferred
    steps = (n_rows + rows_per_wave_step - 1) // rows_per_wave_step
    seq = 1
    while seq < 4 and steps // (seq * 2) >= 8192:
        seq *= 2
    return seq


def geometry(n_rows, n_feat, seq, rows_per_wave=0):
    """(vec, lpr, rows_per_block, grid) of a launch over n_rows x n_feat whose entry point prefers `seq` rows per wave
    (SEQ_K1 / SEQ_K2 / SEQ_SUM): make_geometry, csrc/gts_rows.h:171-180."""
    vec = 4 if n_feat % 4 == 0 else 1
    lpr = lanes_per_row(n_feat // vec)
    rows_per_step = KWAVE // lpr
    seq = pick_seq(n_rows, rows_per_step, seq, rows_per_wave)
    rows_per_block = rows_per_step * seq * WAVES_PER_BLOCK
    return vec, lpr, rows_per_block, (n_rows + rows_per_block - 1) // rows_per_block


def tile_of(block, grid):
    """xcd_contiguous_tile, csrc/gts_common.h:18-21."""
    q, r, x = grid >> 3, grid & 7, block & 7
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (block >> 3)


def row_counts(rows_per_block):
    """Rows on both sides of one workgroup and of the grids 8, 9 and 18 (q = 1 with r = 0, q = 1 with r != 0, q = 2)."""
    r = rows_per_block
    out = []
    for n in (1, r - 1, r, r + 1, 7 * r + 1, 8 * r, 9 * r - 1, 17 * r + 3):
        if n > 0 and n not in out:
            out.append(n)
    return out


# ---------------------------------------------------------------- case lists
WIDTHS_VEC1 = [1, 2, 3, 5, 9, 17, 33, 63, 65, 129]
WIDTHS_VEC4 = [4, 8, 12, 16, 28, 32, 60, 64, 124, 128, 252, 256, 260, 512, 516]
WIDTHS = WIDTHS_VEC1 + WIDTHS_VEC4
# one width per (VEC, LPR) instantiation of GTS_DISPATCH_GEOM, LPR = 1, 2, 4, 8, 16, 32, 64
ROW_COUNT_WIDTHS = [1, 2, 3, 5, 9, 17, 65, 4, 8, 12, 28, 60, 124, 260]
OPTION_WIDTHS = [1, 20, 256, 260]
OPTION_ROWS_PER_WAVE = [1, 2, 3, 4, 8]
OPTION_STREAMING = [0, 1, 2, 3]
VALUE_WIDTHS = [3, 64, 256]
VALUE_ROWS = 1000        # rows of the value-class graph: room for rows whose sources no other placed row shares
HUB_DEGREES = [253, 254, 255, 256]
HUB_WIDTHS = [4, 256]

DEGREES_U8 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15, 16, 17, 23, 24, 25, 63, 64, 65, 127, 128, 253, 254]
DEGREES_I32 = DEGREES_U8 + [255, 256, 300]
LADDERS = {"u8": DEGREES_U8, "i32": DEGREES_I32}


# ---------------------------------------------------------------- degree-ladder graphs
def _ladder_degrees(n, degrees, rng):
    """Degree of every row: degrees[perm[v % L]]; below L rows a subset that keeps the maximum, 0 and, while they fit,
    one degree above 8 of every remainder mod 8 the ladder has."""
    count = len(degrees)
    if n >= count:
        perm = rng.permutation(count)
        return np.asarray([degrees[perm[v % count]] for v in range(n)], dtype=np.int64)
    must = [max(degrees), 0]
    for r in rng.permutation(8):
        if any(d > 8 and d % 8 == r for d in must):
            continue
        fits = [d for d in degrees if d > 8 and d % 8 == r]
        if fits:
            must.append(fits[int(rng.integers(len(fits)))])
    must = must[:n]
    rest = [d for d in degrees if d not in must]
    chosen = must + [int(d) for d in rng.choice(rest, n - len(must), replace=False)]
    return np.asarray(chosen, dtype=np.int64)[rng.permutation(n)]


def ladder_graph(n, degrees, seed, transpose=False):
    """gts.Graph (host) of n rows whose in-degrees (transpose: out-degrees) walk the ladder `degrees`, so that empty rows
    and hubs share a wave.  The other end of every edge is uniform with replacement (multi-edges and self-loops occur)
    and the COO order is shuffled."""
    rng = np.random.default_rng(seed)
    deg = _ladder_degrees(n, degrees, rng)
    fixed = np.repeat(np.arange(n, dtype=np.int64), deg)
    free = rng.integers(0, n, size=fixed.size)
    order = rng.permutation(fixed.size)
    src, dst = (fixed, free) if transpose else (free, fixed)
    g = gts.Graph(src[order], dst[order], n)
    if transpose:
        assert np.array_equal(np.diff(g.t_indptr), deg) and g.max_out_degree == int(deg.max())
        assert g.arg_bytes == (1 if g.max_in_degree <= 254 else 4)
    else:
        assert np.array_equal(np.diff(g.indptr), deg)
        assert g.arg_bytes == (1 if max(degrees) <= 254 else 4)
    return g


_graphs = {}


def ladder(n, name, seed, transpose=False):
    """ladder_graph over LADDERS[name], built once per (n, ladder, seed, transpose)."""
    key = (n, name, seed, transpose)
    if key not in _graphs:
        _graphs[key] = ladder_graph(n, LADDERS[name], seed, transpose)
    return _graphs[key]


def forget_graphs_above(n_edges):
    """Drop the cached graphs with more edges than that (the largest row counts belong to one test each)."""
    for key in [k for k, g in _graphs.items() if g.number_of_edges() > n_edges]:
        del _graphs[key]


def width_graph(width, name, transpose=False):
    """The graph of the every-width test: 2 R + 1 rows for K1's rows per workgroup R (three workgroups, the last with one
    row; K2 and the sums, with half as many rows per workgroup, get five)."""
    return ladder(2 * geometry(1, width, SEQ_K1)[2] + 1, name, width, transpose)


def hub_graph(deg, seed=0):
    """Row 0 has in-degree `deg` with the distinct sources 1 .. deg in slot order; every other row has two random
    in-edges; COO order shuffled among rows (a stable sort keeps row 0's order)."""
    rng = np.random.default_rng(seed + deg)
    n = deg + 8
    others = np.repeat(np.arange(1, n, dtype=np.int64), 2)
    src = np.concatenate([np.arange(1, deg + 1, dtype=np.int64), rng.integers(0, n, size=others.size)])
    dst = np.concatenate([np.zeros(deg, dtype=np.int64), others])
    hub = np.sort(rng.permutation(src.size)[:deg])      # positions the hub's edges take, in their own order
    order = np.empty(src.size, dtype=np.int64)
    mask = np.zeros(src.size, dtype=bool)
    mask[hub] = True
    order[mask] = np.arange(deg)
    order[~mask] = deg + rng.permutation(others.size)
    g = gts.Graph(src[order], dst[order], n)
    assert np.array_equal(g.indices[:deg], np.arange(1, deg + 1)) and g.max_in_degree == deg
    assert g.arg_bytes == (1 if deg <= 254 else 4)
    return g


def hub_features(deg, n_feat, seed=0):
    """Column c of the hub's sources: c % 3 == 0 a unique maximum in the first slot, 1 in the last slot, 2 a full tie."""
    rng = np.random.default_rng(seed + 7 * deg)
    x = rng.integers(-3, 4, size=(deg + 8, n_feat)).astype(np.float32)
    cols = np.arange(n_feat)
    x[1, cols % 3 == 0] = 5
    x[deg, cols % 3 == 1] = 5
    x[1:deg + 1, cols % 3 == 2] = 2
    return x


# ---------------------------------------------------------------- features
def integers(n, n_feat, seed):
    """-3 .. 3: ties everywhere, exact sums."""
    return np.random.default_rng(seed).integers(-3, 4, size=(n, n_feat)).astype(np.float32)


def gaussian(n, n_feat, seed):
    return np.random.default_rng(seed).standard_normal((n, n_feat)).astype(np.float32)


def divisors(g, kind, seed):
    """[n] fp32: in-degree + 1, or random positive values that are no powers of two (a division by them rounds)."""
    if kind == "deg":
        return (np.diff(g.indptr) + 1).astype(np.float32)
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 9, size=g.n) + rng.uniform(0.1, 0.9, size=g.n)).astype(np.float32)


def width_inputs(width, name, transpose=False):
    """What the every-width test feeds its kernels (and the host test its deliberately wrong variants)."""
    g = width_graph(width, name, transpose)
    return dict(g=g, integers=integers(g.n, width, width), gaussian=gaussian(g.n, width, width + 1000),
                gout=gaussian(g.n, width, width + 2000), accum=gaussian(g.n, width, width + 3000),
                divisors={"deg": divisors(g, "deg", 0), "random": divisors(g, "random", width + 4000)})


def _place_rows(g, rng, wants):
    """name -> row for every (name, degree test, source test) of `wants`, rows whose sources no other placed row has."""
    deg = np.diff(g.indptr)
    used = np.zeros(g.n, dtype=bool)
    rows = {}
    for name, deg_ok, src_ok in wants:
        for v in rng.permutation(g.n):
            u = g.indices[g.indptr[v]:g.indptr[v + 1]]
            if deg_ok(int(deg[v])) and src_ok(u) and not used[u].any() and not used[v]:
                rows[name] = int(v)
                used[u] = True
                break
        else:
            raise AssertionError(f"no row for {name}: the graph is too small")
    return rows


def _distinct(u):
    return np.unique(u).size == u.size


def signed_zeros(g, n_feat, seed):
    """(x, rows): sources that are whole rows of -0.0, of +0.0, of both mixed by column, or of -1 (so that a zero is
    the maximum wherever there is one), and three placed rows: 'neg' sees only -0.0, 'neg_then_pos' -0.0 in its first
    slot and +0.0 after it, 'pos_then_neg' the reverse."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(4, size=g.n, p=[0.35, 0.25, 0.25, 0.15])
    x = np.where(rng.random((g.n, n_feat)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    x[kind == 0] = -0.0
    x[kind == 1] = 0.0
    x[kind == 3] = -1.0
    small = lambda d: 3 <= d <= 10
    rows = _place_rows(g, rng, [(k, small, _distinct) for k in ("neg", "neg_then_pos", "pos_then_neg")])
    for name, first, rest in (("neg", -0.0, -0.0), ("neg_then_pos", -0.0, 0.0), ("pos_then_neg", 0.0, -0.0)):
        u = g.indices[g.indptr[rows[name]]:g.indptr[rows[name] + 1]]
        x[u[1:]] = rest
        x[u[0]] = first
    return x, rows


def nonfinite(g, n_feat, seed):
    """(x, rows): gaussian features with placed rows: 'nan_only' has only NaN neighbours, 'nan_among' one NaN among
    finite values, 'pos_inf' a +Inf maximum, 'neg_inf_single' a single neighbour of -Inf, and 'last_slot', of degree 254,
    sees values <= 0 in every slot but its last."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((g.n, n_feat)).astype(np.float32)
    small = lambda d: 3 <= d <= 10
    last_unique = lambda u: int((u == u[-1]).sum()) == 1
    rows = _place_rows(g, rng, [("last_slot", lambda d: d == 254, last_unique), ("nan_only", small, _distinct),
                                ("nan_among", small, _distinct), ("pos_inf", small, _distinct),
                                ("neg_inf_single", lambda d: d == 1, _distinct)])
    src = {k: g.indices[g.indptr[v]:g.indptr[v + 1]] for k, v in rows.items()}
    u = src["last_slot"]
    x[u] = -np.abs(x[u])
    x[u[::5]] = 0.0
    x[u[-1]] = np.abs(rng.standard_normal(n_feat)).astype(np.float32) + 1
    x[src["nan_only"]] = np.nan
    x[src["nan_among"][1]] = np.nan
    x[src["pos_inf"][-1]] = np.inf
    x[src["neg_inf_single"]] = -np.inf
    return x, rows


# ---------------------------------------------------------------- references
def max_ref_full(g, x, relu_input=False):
    """(out fp32 [n, F], winner's source id [n, F], winner's slot in its in-CSR row [n, F]); -1 = no winner."""
    n, f = g.n, x.shape[1]
    out = np.zeros((n, f), dtype=np.float32)
    src = np.full((n, f), -1, dtype=np.int64)
    win = np.full((n, f), -1, dtype=np.int64)
    cols = np.arange(f)
    ptr = g.indptr.tolist()
    if np.isnan(x).any():
        x = np.where(np.isnan(x), np.float32(-np.inf), x)            # `best < NaN` is false: a NaN never wins
    for v in range(n):
        u = g.indices[ptr[v]:ptr[v + 1]]
        if u.size == 0:
            continue
        vals = x[u]                                                  # [deg, F] in slot order
        slot = np.argmax(vals, axis=0)                               # first occurrence of the maximum == strict '<'
        best = vals[slot, cols]
        dead = np.isinf(best)                                        # nothing above -inf, or a +inf maximum
        out[v] = np.where(dead, np.float32(0), best)
        keep = ~dead & (best > 0) if relu_input else ~dead
        src[v] = np.where(keep, u[slot], -1)
        win[v] = np.where(keep, slot, -1)
    return out, src, win


def max_ref(g, x, relu_input=False, slots=False):
    """(out, winner's source id or -1); slots=True: the winner's slot instead, as K1 records it."""
    out, src, win = max_ref_full(g, x, relu_input)
    return out, (win if slots else src)


def _chain(terms):
    """+0.0 + terms[0] + terms[1] + ... along axis 0, one rounding per add (accumulate is sequential by definition)."""
    start = np.zeros((1,) + terms.shape[1:], dtype=terms.dtype)
    return np.add.accumulate(np.concatenate([start, terms]), axis=0)[-1]


def max_bwd_ref(g, gout, winners, relu_src=None):
    """fp32 [n, F].  winners: slots as K1 records them, -1 = none.  An edge that did not win adds +0.0, which changes no
    bit of a sum that started from +0.0."""
    n, f = g.n, gout.shape[1]
    gx = np.zeros((n, f), dtype=np.float32)
    ptr = g.t_indptr.tolist()
    for u in range(n):
        beg, end = ptr[u], ptr[u + 1]
        if beg == end:
            continue
        d = g.t_indices[beg:end]
        won = winners[d] == g.t_slot[beg:end, None]
        gx[u] = _chain(np.where(won, gout[d], np.float32(0)))
    if relu_src is not None:
        gx = np.where(relu_src > 0, gx, np.float32(0))
    return gx


def _sum(indptr, indices, x, div_in, div_out, add_self, accum, dtype):
    x = x.astype(dtype)
    div_in, div_out, accum = (None if a is None else a.astype(dtype) for a in (div_in, div_out, accum))
    n = indptr.size - 1
    out = np.zeros((n, x.shape[1]), dtype=dtype)
    ptr = indptr.tolist()
    with np.errstate(all="ignore"):
        for v in range(n):
            u = indices[ptr[v]:ptr[v + 1]]
            terms = x[u] if div_in is None else x[u] / div_in[u, None]
            acc = _chain(terms)
            if add_self:
                acc = acc + (x[v] if div_in is None else x[v] / div_in[v])
            if div_out is not None:
                acc = acc / div_out[v]
            out[v] = acc if accum is None else accum[v] + acc
    return out


def sum_ref(indptr, indices, x, div_in=None, div_out=None, add_self=False, accum=None):
    """gts_spmm_sum_f32 in fp32, every operation rounded once."""
    return _sum(indptr, indices, x, div_in, div_out, add_self, accum, np.float32)


def sum_ref64(indptr, indices, x, div_in=None, div_out=None, add_self=False, accum=None):
    return _sum(indptr, indices, x, div_in, div_out, add_self, accum, np.float64)


SUM_FLAGS = [(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)]   # div_in, div_out, add_self, accum


def same_bits(a, b):
    """Equal as int32 bit patterns, or both NaN (only the sum family may produce a NaN)."""
    a, b = (np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32) for t in (a, b))
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())
