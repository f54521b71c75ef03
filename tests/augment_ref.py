"""The augmentation kernels' definition in numpy (include/gts_hip.h): Philox4x32-10, the Box-Muller
mapping of its words to normals in float64, np.flip, the float32 affine, and the feature map by np.repeat of the
graph sizes.  Written from the definitions, not from the kernels."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: two 32-bit words -> uint32 [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _32, p0 & _LOW, p1 >> _32, p1 & _LOW
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def normals_from_words(words):
    """uint32 [..., 4] -> float64 [..., 4]: normals 0, 1 from words (0, 1), normals 2, 3 from words (2, 3)."""
    w = np.asarray(words).astype(np.uint64)
    out = np.empty(w.shape, dtype=np.float64)
    for p in (0, 2):
        u = ((w[..., p] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        theta = 2.0 * np.pi * (w[..., p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u))
        out[..., p], out[..., p + 1] = r * np.cos(theta), r * np.sin(theta)
    return out


def normals(n_index, n_channels, seed, step, stream):
    """float64 [n_index, n_channels]: n(idx, c) of stream 0 (A1, idx = output voxel) or 1 (A2, idx = row).
    seed: (low, high) key words; step: the 64-bit counter."""
    groups = (n_channels + 3) // 4
    idx = np.arange(n_index, dtype=np.uint64)[:, None]
    g = np.arange(groups, dtype=np.uint64)[None, :]
    counter = np.empty((n_index, groups, 4), dtype=np.uint32)
    counter[..., 0] = (idx & _LOW) + 0 * g
    counter[..., 1] = (idx >> _32) | (g << np.uint64(24)) | np.uint64(stream << 31)
    counter[..., 2] = step & 0xFFFFFFFF
    counter[..., 3] = (step >> 32) & 0xFFFFFFFF
    n = normals_from_words(philox4x32_10(counter, seed))
    return n.reshape(n_index, groups * 4)[:, :n_channels]


def flip(a, flips):
    axes = tuple(ax for ax in range(3) if flips[ax])
    return np.flip(a, axis=axes) if axes else a


def affine_f32(x, a, b):
    """numpy float32 x * a + b (a multiply, then an add, each rounded), a channel with a == 1 and b == 0 copied."""
    x, a, b = np.asarray(x, dtype=np.float32), np.float32(a), np.float32(b)
    return x.copy() if (a == 1 and b == 0) else x * a + b


def crop_no_noise(x, labels, plan):
    """(x', labels') of A1 without its noise term, float32 / int64: what the kernel must equal bit for bit at
    sigma == 0.  x [cx, cy, cz, C] or None, labels [cx, cy, cz] or None."""
    out = None
    if x is not None:
        out = np.ascontiguousarray(flip(x, plan.flips)).astype(np.float32)
        for c in range(plan.channels):
            out[..., c] = affine_f32(out[..., c], plan.scale[c], plan.shift[c])
    lab = np.ascontiguousarray(flip(labels, plan.flips)) if labels is not None else None
    return out, lab


def crop_noise(shape, n_channels, plan):
    """float64 [cx, cy, cz, n_channels]: sigma_c * n(v, c) for the image channels, 0 for the others."""
    v = int(np.prod(shape))
    n = normals(v, n_channels, plan.seed, plan.step, 0).reshape(*shape, n_channels)
    sigma = np.zeros(n_channels)
    sigma[:plan.channels] = plan.sigma.astype(np.float64)
    return n * sigma


def crop(x, labels, plan):
    """A1 in float64: (x' [cx, cy, cz, C], labels')."""
    base, lab = crop_no_noise(x, labels, plan)
    if base is None:
        return None, lab
    return base.astype(np.float64) + crop_noise(x.shape[:3], x.shape[3], plan), lab


def feature_params(sizes, plans, n_feats):
    """(a, b) float32 [N, F]: the scale and shift every feature of every row takes."""
    modalities = plans[0].channels
    per = n_feats // modalities
    a = np.stack([np.repeat(p.scale, per) for p in plans]).reshape(len(plans), n_feats)
    b = np.stack([np.repeat(p.shift, per) for p in plans]).reshape(len(plans), n_feats)
    return np.repeat(a, sizes, axis=0), np.repeat(b, sizes, axis=0)


def features_no_noise(feats, sizes, plans):
    """A2 without its noise term in float32: feats * a + b, elements with a == 1 and b == 0 copied."""
    feats = np.asarray(feats, dtype=np.float32)
    a, b = feature_params(sizes, plans, feats.shape[1])
    return np.where((a == 1) & (b == 0), feats, feats * a + b)


def features_noise(n_rows, n_feats, plan):
    return plan.feature_sigma * normals(n_rows, n_feats, plan.seed, plan.step, 1)
