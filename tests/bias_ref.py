"""numpy reference of the bias-field correction, written from the definition and independently of
gts/bias.py: what csrc/gts_bias.hip and the host loop are held to.  Volumes are [Z, Y, X] arrays, x fastest.

The field's arithmetic is fixed to the last bit (float64, elementwise numpy products and sums in the order the
definition gives, which numpy neither contracts nor reorders); the sharpening uses a plain O(P^2) DFT, no numpy.fft;
the fit is an einsum, whose order is its own: the GPU tests hold the fit to a rounding bound, not to its bits.
"""
import numpy as np

BINS = 200


def log_image(v, threshold=0.0):
    """float32 [Z, Y, X]: log of the voxels that are finite and above the threshold, NaN elsewhere."""
    v64 = np.asarray(v).astype(np.float64)
    member = np.isfinite(v64) & (v64 > np.float64(threshold))
    u = np.full(v64.shape, np.nan, dtype=np.float32)
    u[member] = np.log(v64[member]).astype(np.float32)
    return u


def basis(n, spans):
    """(cell [n] int64, weights [n, 4] float64) of an axis of extent n cut into `spans` cells."""
    cell = np.empty(n, dtype=np.int64)
    w = np.empty((n, 4), dtype=np.float64)
    for i in range(n):
        t = np.float64(i * spans) / np.float64(n)
        c = np.floor(t)
        s = t - c
        a = np.float64(1.0) - s
        s2 = s * s
        s3 = s2 * s
        cell[i] = int(c)
        w[i, 0] = ((a * a) * a) / 6.0
        w[i, 1] = ((3.0 * s3 - 6.0 * s2) + 4.0) / 6.0
        w[i, 2] = (((-3.0 * s3 + 3.0 * s2) + 3.0 * s) + 1.0) / 6.0
        w[i, 3] = s3 / 6.0
    return cell, w


def points(spans0, level):
    return (spans0 << level) + 3


def empty_lattices(spans0, levels):
    return [np.zeros((points(spans0, k),) * 3, dtype=np.float64) for k in range(levels)]


def level_field(lattice, shape, spans):
    """float64 [Z, Y, X] of one lattice [n, n, n] (z slowest): sum_a Bx_a (sum_b By_b (sum_c Bz_c L[cz+c][cy+b][cx+a])),
    every sum ascending from its first term."""
    Z, Y, X = shape
    cz, wz = basis(Z, spans)
    cy, wy = basis(Y, spans)
    cx, wx = basis(X, spans)
    tz = wz[:, 0, None, None] * lattice[cz]
    for c in range(1, 4):
        tz = tz + wz[:, c, None, None] * lattice[cz + c]                    # [Z, n, n]
    ty = wy[None, :, 0, None] * tz[:, cy, :]
    for b in range(1, 4):
        ty = ty + wy[None, :, b, None] * tz[:, cy + b, :]                   # [Z, Y, n]
    f = wx[None, None, :, 0] * ty[:, :, cx]
    for a in range(1, 4):
        f = f + wx[None, None, :, a] * ty[:, :, cx + a]                     # [Z, Y, X]
    return f


def field(lattices, shape, spans0):
    """The levels added in ascending order, starting from the first."""
    f = level_field(lattices[0], shape, spans0)
    for k in range(1, len(lattices)):
        f = f + level_field(lattices[k], shape, spans0 << k)
    return f


def residual_image(u, lattices, spans0):
    """(d float64 [Z, Y, X], mask): d = float64(u) - field; the mask is where u is not NaN."""
    return u.astype(np.float64) - field(lattices, u.shape, spans0), ~np.isnan(u)


def value_range(d, mask):
    if not mask.any():
        return np.float64(np.inf), np.float64(-np.inf)
    return d[mask].min(), d[mask].max()


def histogram(d, mask, lo, hi):
    w = (np.float64(hi) - np.float64(lo)) / np.float64(BINS - 1)
    pos = (d[mask] - np.float64(lo)) / w
    idx = np.clip(np.floor(pos + 0.5), 0, BINS - 1).astype(np.int64)
    return np.bincount(idx, minlength=BINS).astype(np.int64)


_DFT = {}


def _dft(x, inverse=False):
    n = len(x)
    if (n, inverse) not in _DFT:                 # the matrix of the transform, made once per size
        jk = np.outer(np.arange(n), np.arange(n)) % n
        _DFT[n, inverse] = np.exp((2j if inverse else -2j) * np.pi * jk / n)
    y = _DFT[n, inverse] @ np.asarray(x, dtype=np.complex128)
    return y / n if inverse else y


def sharpen(counts, lo, hi):
    """The sharpened value of every bin: Wiener deconvolution with a Gaussian of FWHM 0.15 on 512 points, then the
    conditional mean under the blur.  Plain DFT."""
    counts = np.asarray(counts, dtype=np.float64)
    bins = len(counts)
    P = 1
    while P < 2 * bins:
        P *= 2
    off = (P - bins) // 2
    w = (np.float64(hi) - np.float64(lo)) / (bins - 1)
    H = np.zeros(P)
    H[off:off + bins] = counts
    sigma = 0.15 / w / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    gauss = np.array([np.exp(-min(j, P - j) ** 2 / (2.0 * sigma ** 2)) for j in range(P)])
    gauss /= gauss.sum()
    F = _dft(gauss)
    G = np.conj(F) / (np.abs(F) ** 2 + 0.01)
    U = np.maximum(_dft(_dft(H) * G, inverse=True).real, 0.0)
    centre = lo + (np.arange(P) - off) * w
    top = _dft(_dft(centre * U) * F, inverse=True).real
    bottom = _dft(_dft(U) * F, inverse=True).real
    E = centre.copy()
    good = bottom > 1e-12 * bottom.max()
    E[good] = top[good] / bottom[good]
    return E[off:off + bins]


def residual(d, mask, lo, hi, E):
    """r = d - E(d), E linear between the table's entries; 0 outside the mask."""
    w = (np.float64(hi) - np.float64(lo)) / np.float64(BINS - 1)
    pos = (np.where(mask, d, lo) - np.float64(lo)) / w
    i0 = np.clip(np.floor(pos), 0, BINS - 2).astype(np.int64)
    fr = pos - i0
    r = d - (E[i0] + (E[i0 + 1] - E[i0]) * fr)
    return np.where(mask, r, 0.0)


def _scatter(n, spans, values):
    """[N, spans + 3]: values[i, a] at column cell(i) + a."""
    cell, _ = basis(n, spans)
    m = np.zeros((n, spans + 3), dtype=np.float64)
    for a in range(4):
        m[np.arange(n), cell + a] = values[:, a]
    return m


def fit(r, mask, spans, bounds=True):
    """Lee's B-spline approximation of the residual at one level: a dict of float64 [n, n, n] arrays: num, den, delta
    (num / den, 0 where den == 0), and with `bounds`, for the tests' bounds, abs_num = sum |term| of num and terms =
    the number of mask voxels that sit on each control point."""
    mats = []
    for n in r.shape:
        _, w = basis(n, spans)
        q = w ** 2
        p = w ** 3 / (q[:, 0] + q[:, 1] + q[:, 2] + q[:, 3])[:, None]
        mats.append((_scatter(n, spans, p), _scatter(n, spans, q), _scatter(n, spans, np.ones_like(w))))
    (pz, qz, sz), (py, qy, sy), (px, qx, sx) = mats
    m = mask.astype(np.float64)
    path = "zc,yb,xa,zyx->cba"
    num = np.einsum(path, pz, py, px, r, optimize=True)
    den = np.einsum(path, qz, qy, qx, m, optimize=True)
    delta = np.zeros_like(num)
    np.divide(num, den, out=delta, where=den != 0)
    out = {"num": num, "den": den, "delta": delta}
    if bounds:
        out["abs_num"] = np.einsum(path, pz, py, px, np.abs(r), optimize=True)
        out["terms"] = np.rint(np.einsum(path, sz, sy, sx, m, optimize=True)).astype(np.int64)
    return out


def mask_mean(f, mask):
    return f[mask].sum() / np.float64(mask.sum())


def apply(v, f, mean):
    """(out, field volume): float32(float64(v) / exp(field - mean)) everywhere, float32(field - mean)."""
    g = f - np.float64(mean)
    with np.errstate(all="ignore"):
        return (np.asarray(v).astype(np.float64) / np.exp(g)).astype(np.float32), g.astype(np.float32)


def correct_volume(v, levels=4, spans0=1, iterations=50, tol=1e-3, threshold=0.0):
    """(corrected float32, field float32 (mean-free over the mask), report) by the definition's loop."""
    u = log_image(v, threshold)
    lattices = empty_lattices(spans0, levels)
    report, flat = [], False
    for level in range(levels):
        rounds, change = 0, None
        while rounds < iterations and not flat:
            d, mask = residual_image(u, lattices, spans0)
            lo, hi = value_range(d, mask)
            if not hi > lo:
                flat = True
                break
            E = sharpen(histogram(d, mask, lo, hi), lo, hi)
            delta = fit(residual(d, mask, lo, hi, E), mask, spans0 << level, bounds=False)["delta"]
            lattices[level] = lattices[level] + delta
            change = float(np.abs(delta).max())
            rounds += 1
            if change < tol:
                break
        report.append({"spans": spans0 << level, "iterations": rounds, "last_change": change})
    f = field(lattices, u.shape, spans0)
    mask = ~np.isnan(u)
    out, g = apply(v, f, mask_mean(f, mask))
    return out, g, report


# ---- the phantom of the issue -----------------------------------------------------------------------------------------

def phantom(shape=(36, 40, 48), seed=0):
    """(biased float32 [Z, Y, X], clean float32, true log field float64, classes int [Z, Y, X] with 0 = background):
    an ellipsoidal head of three nested tissue classes with 5 %, 3 % and 2 % noise, multiplied by exp of the log field
    0.25 x - 0.2 y^2 + 0.15 z x + 0.1 z on [-1, 1]^3."""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    z, y, x = np.meshgrid(np.linspace(-1, 1, Z), np.linspace(-1, 1, Y), np.linspace(-1, 1, X), indexing="ij")
    rad = np.sqrt((x / 0.92) ** 2 + (y / 0.88) ** 2 + (z / 0.9) ** 2)
    classes = np.zeros(shape, dtype=np.int64)
    classes[rad < 1.0] = 1
    classes[rad < 0.75] = 2
    classes[rad < 0.4] = 3
    level = np.array([0.0, 400.0, 700.0, 1000.0])[classes]
    noise = np.array([0.0, 0.05, 0.03, 0.02])[classes]
    clean = level * (1.0 + noise * rng.standard_normal(shape))
    clean = np.where(classes > 0, np.maximum(clean, 1.0), 0.0)
    log_field = 0.25 * x - 0.2 * y ** 2 + 0.15 * z * x + 0.1 * z
    return (clean * np.exp(log_field)).astype(np.float32), clean.astype(np.float32), log_field, classes


def score(estimate, truth, mask):
    """(correlation, rms residual) of an estimated log field against the true one over the mask, both mean-free."""
    e = np.asarray(estimate, dtype=np.float64)[mask]
    t = np.asarray(truth, dtype=np.float64)[mask]
    e = e - e.mean()
    t = t - t.mean()
    return float((e * t).sum() / np.sqrt((e * e).sum() * (t * t).sum())), float(np.sqrt(((e - t) ** 2).mean()))


def class_cv(volume, classes):
    """The coefficient of variation of each tissue class."""
    v = np.asarray(volume, dtype=np.float64)
    return [float(v[classes == k].std() / v[classes == k].mean()) for k in (1, 2, 3)]
