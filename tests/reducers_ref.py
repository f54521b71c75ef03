"""Host restatements (numpy, no GPU) of the column reducers in csrc/gts_gat_reduce.hip and of the AdamW rule in
csrc/gts_optim.hip, for tests/test_gpu_reducers.py.

The reducers add in a fixed, documented order, and the library is built with -ffp-contract=off, so an fp32 restatement
of that order is expected to give the device's bits: `chunked_colsum_f32` is that restatement.  The float64 functions are
the independent judges (a restatement can copy a bug; a plain float64 sum cannot)."""
import numpy as np

MAX_CHUNKS = 512          # kMaxChunks: at most this many row chunks, one workgroup each
LANES = 16                # sum_chunks_kernel: 16 adder lanes per column group
U = 2.0 ** -24            # fp32 unit roundoff (round to nearest)


def chunk_geometry(n):
    """(rows_per_chunk, n_chunks) of an n-row reduction: rows_per_chunk = ceil(n / 512), and as many chunks of that many
    rows as cover [0, n); the last one may be short."""
    n = int(n)
    if n <= 0:
        raise ValueError("n must be positive")
    rpc = (n + MAX_CHUNKS - 1) // MAX_CHUNKS
    return rpc, (n + rpc - 1) // rpc


def chain_depth(n):
    """Length of the longest chain of additions behind one output of the chunked sum."""
    rpc, chunks = chunk_geometry(n)
    return rpc + (chunks + LANES - 1) // LANES + LANES


def chunked_colsum_f32(rows):
    """Column sums of fp32 rows [n, cols] in the device's association, every addition rounded to fp32:
    per chunk the rows in row order onto 0; lane j of 16 adds the chunk sums j, j+16, ... in order onto 0; the 16 lane
    totals are added in lane order starting from lane 0."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 2
    n, cols = rows.shape
    rpc, chunks = chunk_geometry(n)
    first = np.arange(chunks, dtype=np.int64) * rpc
    part = np.zeros((chunks, cols), np.float32)
    for r in range(rpc):
        live = first + r < n                      # every chunk but, past its end, the short last one
        part[live] = part[live] + rows[first[live] + r]
    lane = np.zeros((LANES, cols), np.float32)
    for t in range((chunks + LANES - 1) // LANES):
        k = min(LANES, chunks - t * LANES)        # lanes that still have a chunk on this trip
        lane[:k] = lane[:k] + part[t * LANES:t * LANES + k]
    total = lane[0].copy()
    for j in range(1, LANES):
        total = total + lane[j]
    assert total.dtype == np.float32
    return total


def colsum_f64(rows):
    """(sum, sum of magnitudes) per column in float64, without a float64 copy of the whole array."""
    s = np.zeros(rows.shape[1], np.float64)
    a = np.zeros(rows.shape[1], np.float64)
    for lo in range(0, rows.shape[0], 4096):
        blk = rows[lo:lo + 4096].astype(np.float64)
        s += blk.sum(0)
        a += np.abs(blk).sum(0)
    return s, a


def act_bwd_terms(gout, out, act):
    """g_pre [n, cols] in fp32: the gradient carried through the activation's OUTPUT (1 = ELU, 2 = ReLU, 0 = none)."""
    gout = np.asarray(gout)
    assert gout.dtype == np.float32
    if act == 0:
        return gout
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == gout.shape
    if act == 1:
        return np.where(out > 0, gout, gout * (out + np.float32(1.0)))
    if act == 2:
        return np.where(out > 0, gout, np.float32(0.0))
    raise ValueError(act)


def act_bwd_ref(gout, out, act):
    """(g_pre, g_bias) as gts_gat_act_bwd_f32 forms them, in fp32."""
    g_pre = act_bwd_terms(gout, out, act)
    return g_pre, chunked_colsum_f32(g_pre.reshape(g_pre.shape[0], -1))


def param_grad_terms(ft, g):
    """The fp32 products g[n,h] * ft[n,h,:] (rounded once), as rows [n, H*D]."""
    ft, g = np.asarray(ft), np.asarray(g)
    assert ft.dtype == np.float32 and g.dtype == np.float32 and ft.ndim == 3 and g.shape == ft.shape[:2]
    return (g[:, :, None] * ft).reshape(ft.shape[0], -1)


def param_grad_ref(ft, gel, ger):
    """(g_attn_l, g_attn_r) [H, D] as gts_gat_param_grad_f32 forms them, in fp32."""
    shape = ft.shape[1:]
    return (chunked_colsum_f32(param_grad_terms(ft, gel)).reshape(shape),
            chunked_colsum_f32(param_grad_terms(ft, ger)).reshape(shape))


def adamw_ref64(p, g, m, v, lr, betas, eps, wd, step, with_delta=False):
    """One AdamW update (the rule in the header of gts_optim.hip) in float64 from fp32 inputs:
    (p, m, v) after the step; with_delta adds the bias-corrected step that was subtracted from the decayed p."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    beta1, beta2 = float(betas[0]), float(betas[1])
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    delta = (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    p = p - delta
    return (p, m, v, delta) if with_delta else (p, m, v)


def adamw_f32(p, g, m, v, lr, betas, eps, wd, step):
    """The same update the way the kernel forms it: constants in double rounded to fp32 once, then fp32 arithmetic with one
    rounding per operation.  Used on the host to show that a correct fp32 implementation meets the bars of the GPU test."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    beta1, beta2 = float(betas[0]), float(betas[1])
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    decay, w1, b2, w2 = f(1.0 - lr * wd), f(1.0 - beta1), f(beta2), f(1.0 - beta2)
    step_size, bc2_sqrt, eps = f(lr / bc1), f(np.sqrt(bc2)), f(eps)
    p = p * decay
    m = m + w1 * (g - m)
    v = b2 * v + w2 * (g * g)
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def adamw_bars(p_old, g, m_old, ref_v, delta):
    """The three one-step bars of the GPU test (absolute, per element): see test_gpu_reducers.py."""
    p_old, g, m_old = (np.abs(np.asarray(a, dtype=np.float64)) for a in (p_old, g, m_old))
    return 16 * U * (p_old + np.abs(delta)), 4 * U * (m_old + g), 4 * U * ref_v


def adamw_cancellation_allowance(g, m_old, ref_v, lr, betas, eps, step):
    """What the p bar lacks when m + (1 - beta1)(g - m) cancels (g and m of opposite sign): the first moment then carries
    an ABSOLUTE error of up to 4u(|m_old| + |g|) however small it comes out, and the step passes it on multiplied by
    (lr / bc1) / (sqrt(v) / sqrt(bc2) + eps)."""
    g, m_old = (np.abs(np.asarray(a, dtype=np.float64)) for a in (g, m_old))
    bc1, bc2 = 1.0 - float(betas[0]) ** step, 1.0 - float(betas[1]) ** step
    return (lr / bc1) / (np.sqrt(ref_v) / np.sqrt(bc2) + eps) * 4 * U * (m_old + g)


def adamw_case(n, step, seed, agree=True):
    """fp32 (p, g, m, v) for an n-element update: m = v = 0 at step 1, random m and positive v afterwards; exact zeros and
    values near 1e-6 and 1e3 are planted in g.  agree: m has the sign of g wherever g != 0 (a first moment is a running
    mean of gradients), so that beta1 * m + (1 - beta1) * g does not cancel: the condition under which the p bar is a
    theorem (test_gpu_reducers.py).  agree=False leaves the signs independent."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n, dtype=np.float32)
    g = rng.standard_normal(n, dtype=np.float32)
    k = np.arange(n)
    g[k % 7 == 3] = 0.0
    g[k % 11 == 5] *= np.float32(1e-6)
    g[k % 13 == 2] *= np.float32(1e3)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = np.float32(0.3) * rng.standard_normal(n, dtype=np.float32)
        if agree:
            m = np.where(g != 0, np.copysign(m, g), m)
        v = rng.random(n, dtype=np.float32) + np.float32(1e-3)
    return p, g, m, v
