"""The rotated / zoomed crop's definition in numpy float64 (include/gts_hip.h A3 / A4), written from
the definition, not from the kernels.

Crop extents n, centre c = (n - 1) / 2.  Output voxel o is mirrored to o' on the axes of the plan's flips, d = o' - c,
  p_a = c_a + ((M[a][0] d_0 + M[a][1] d_1) + M[a][2] d_2)        (float64, products and sums rounded one by one)
clamped into [-2, n_a + 1]; f = floor(p), t = p - f.  Float channels: the eight corners (f_a | f_a + 1), 0.0 outside
the crop, lerped along x, then y, then z as a + (b - a) t, rounded once to float32, then the float32 affine of the
image channels.  Labels: labels[floor(p + 0.5)], 0 outside.  The adjoint scatters w(o, q) dy[o] in float64."""
import numpy as np

from tests import augment_ref


def matrix_from(angles, zoom):
    """M = Rz(gamma) Ry(beta) Rx(alpha) / zoom, angles (alpha, beta, gamma) in degrees about x, y, z."""
    a, b, g = (np.deg2rad(float(t)) for t in angles)
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]], dtype=np.float64)
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]], dtype=np.float64)
    rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]], dtype=np.float64)
    return rz.dot(ry).dot(rx) / float(zoom)


def source_points(dims, plan):
    """(p float64 [cx, cy, cz, 3] clamped, o' int64 [cx, cy, cz, 3]) of every OUTPUT voxel."""
    n = np.asarray(dims, dtype=np.int64)
    m = np.asarray(plan.matrix, dtype=np.float64)
    o = np.stack(np.meshgrid(*[np.arange(e) for e in n], indexing="ij"), axis=-1).astype(np.int64)
    mirrored = o.copy()
    for a in range(3):
        if plan.flips[a]:
            mirrored[..., a] = n[a] - 1 - o[..., a]
    c = (n - 1) / 2.0
    d = mirrored - c
    p = np.empty(d.shape, dtype=np.float64)
    for a in range(3):
        p[..., a] = c[a] + ((m[a, 0] * d[..., 0] + m[a, 1] * d[..., 1]) + m[a, 2] * d[..., 2])
        p[..., a] = np.clip(p[..., a], -2.0, n[a] + 1.0)
    return p, mirrored


def _corner(x, idx):
    """x [cx, cy, cz, C] at integer indices idx [..., 3] as float64, 0.0 where any index is outside."""
    n = np.asarray(x.shape[:3])
    inside = np.all((idx >= 0) & (idx < n), axis=-1)
    safe = np.where(inside[..., None], idx, 0)
    values = x[safe[..., 0], safe[..., 1], safe[..., 2]].astype(np.float64)
    return np.where(inside[..., None], values, 0.0)


def resample_values(x, plan):
    """The resampled float channels before the affine: float32 [cx, cy, cz, C]."""
    p, _ = source_points(x.shape[:3], plan)
    f = np.floor(p)
    t = p - f
    f = f.astype(np.int64)

    def at(dx, dy, dz):
        return _corner(x, f + np.array([dx, dy, dz]))

    def lerp(a, b, w):
        return a + (b - a) * w[..., None]

    along_y = []
    for dz in (0, 1):
        along_x = [lerp(at(0, dy, dz), at(1, dy, dz), t[..., 0]) for dy in (0, 1)]
        along_y.append(lerp(along_x[0], along_x[1], t[..., 1]))
    return lerp(along_y[0], along_y[1], t[..., 2]).astype(np.float32)


def resample(x, labels, plan):
    """(x', labels') of A3 at sigma == 0: float32 [cx, cy, cz, C] / int64 [cx, cy, cz]; either input may be None."""
    out = lab = None
    if x is not None:
        out = resample_values(np.asarray(x, dtype=np.float32), plan)
        for c in range(plan.channels):
            out[..., c] = augment_ref.affine_f32(out[..., c], plan.scale[c], plan.shift[c])
    if labels is not None:
        labels = np.asarray(labels)
        p, _ = source_points(labels.shape, plan)
        m = np.floor(p + 0.5).astype(np.int64)
        n = np.asarray(labels.shape)
        inside = np.all((m >= 0) & (m < n), axis=-1)
        safe = np.where(inside[..., None], m, 0)
        lab = np.where(inside, labels[safe[..., 0], safe[..., 1], safe[..., 2]], 0).astype(np.int64)
    return out, lab


def adjoint_terms(dy, dims, plan):
    """(dx float64 [cx, cy, cz, K], sum of |terms| float64 [cx, cy, cz, K]): the scatter-add of w(o, q) dy[o] over the
    eight corners of every output voxel, in float64; the second array bounds what another order of the sum can move."""
    dims = tuple(int(d) for d in dims)
    dy = np.asarray(dy, dtype=np.float64).reshape(dims + (-1,))
    p, _ = source_points(dims, plan)
    f = np.floor(p)
    t = p - f
    f = f.astype(np.int64)
    n = np.asarray(dims)
    dx = np.zeros(dy.shape, dtype=np.float64)
    mass = np.zeros(dy.shape, dtype=np.float64)
    for corner in np.ndindex(2, 2, 2):
        q = f + np.array(corner)
        w = np.ones(dims, dtype=np.float64)
        for a in range(3):
            w = w * (t[..., a] if corner[a] else 1.0 - t[..., a])
        inside = np.all((q >= 0) & (q < n), axis=-1)
        qi = q[inside]
        term = w[inside][:, None] * dy[inside]
        np.add.at(dx, (qi[:, 0], qi[:, 1], qi[:, 2]), term)
        np.add.at(mass, (qi[:, 0], qi[:, 1], qi[:, 2]), np.abs(term))
    return dx, mass


def adjoint(dy, dims, plan):
    """A4 in float64: dx [cx, cy, cz, K] = sum_o w(o, q) dy[o, k] (the resample and the mirror, no affine)."""
    return adjoint_terms(dy, dims, plan)[0]
