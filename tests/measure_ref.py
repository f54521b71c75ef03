"""The per-lesion measurements of gts.measure in scipy and numpy, written straight from the
definition and independent of the package: no candidate pruning, no tiles, int64 / Python integers, and the fixed
float64 expressions.  Also the label volumes the host and the GPU tests share, so the host test can check that
this quadratic reference stays cheap on every one of them."""
import functools
import math

import numpy as np
from scipy import ndimage

REGIONS = ("WT", "CT", "ET")
MAX_LESION_VOXELS = 4096        # the pairwise step below is quadratic: no test lesion is larger


def region_mask(labels, region):
    region = REGIONS.index(region) if region in REGIONS else region
    return (labels != 0, (labels == 2) | (labels == 3), labels == 3)[region]


def spacing_units(spacing_mm):
    """((u_x, u_y, u_z), scale_mm): steps of 1e-4 mm over their common divisor with 10000."""
    steps = [int(round(float(s) * 10000)) for s in spacing_mm]
    g = math.gcd(*steps, 10000)
    return tuple(u // g for u in steps), g / 10000


def diameter2(points):
    """The largest squared distance between two rows of an int64 [n, k] array, every pair taken."""
    top = 0
    for i in range(0, len(points), 256):
        diff = points[i:i + 256, None, :] - points[None, :, :]
        top = max(top, int((diff * diff).sum(axis=2).max()))
    return top


def plane_measure(points):
    """(D2, W, tied pairs) of an int64 [n, 2] footprint in physical units: the largest squared distance, the largest
    caliper width p.P_r range over the pairs that reach it (p perpendicular to the pair's difference, same length),
    and how many unordered pairs reach it."""
    diff = points[:, None, :] - points[None, :, :]
    dist = (diff * diff).sum(axis=2)
    d2 = int(dist.max())
    if d2 == 0:
        return 0, 0, 0
    width, pairs = 0, 0
    for a, b in zip(*np.nonzero(np.triu(dist == d2))):
        d = points[b] - points[a]
        proj = points[:, 0] * (-d[1]) + points[:, 1] * d[0]
        width = max(width, int(proj.max() - proj.min()))
        pairs += 1
    return d2, width, pairs


def lesion_plane(points, units):
    """(z*, D2, W) of a lesion's voxels (int64 [n, 3]): per slice of constant z the plane_measure of its footprint;
    z* is the smallest z with the largest W."""
    best = None
    for z in np.unique(points[:, 2]):
        d2, w, _ = plane_measure(points[points[:, 2] == z][:, :2] * np.array(units[:2], dtype=np.int64))
        if best is None or w > best[2]:
            best = (int(z), d2, w)
    return best


def lesion_table(labels, region, units=(1, 1, 1), connectivity=26):
    """The integer table of gts.measure.lesion_table for a numpy label volume, field by field."""
    labels = np.asarray(labels)
    mask = region_mask(labels, region)
    structure = ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1)
    lab, count = ndimage.label(mask, structure=structure)
    padded = np.pad(mask, 1)
    u = np.array(units, dtype=np.int64)
    out = {k: [] for k in ("root", "n", "n_class", "box", "coord_sum", "faces", "d3", "plane_z", "plane_d2", "plane_w")}
    for k in range(1, count + 1):                       # scipy labels in order of the first voxel: ascending root
        pts = np.argwhere(lab == k).astype(np.int64)
        assert len(pts) <= MAX_LESION_VOXELS, "the reference is quadratic: keep test lesions small"
        values = labels[tuple(pts.T)]
        out["root"].append(1 + int(np.ravel_multi_index(tuple(pts[0]), labels.shape)))
        out["n"].append(len(pts))
        out["n_class"].append([int((values == c).sum()) for c in (1, 2, 3)])
        out["box"].append([v for a in range(3) for v in (int(pts[:, a].min()), int(pts[:, a].max()) + 1)])
        out["coord_sum"].append([int(pts[:, a].sum()) for a in range(3)])
        faces = []
        for a in range(3):
            step = np.zeros(3, dtype=np.int64)
            step[a] = 1
            faces.append(int((~padded[tuple((pts + 1 - step).T)]).sum() + (~padded[tuple((pts + 1 + step).T)]).sum()))
        out["faces"].append(faces)
        out["d3"].append(diameter2(pts * u))
        z, d2, w = lesion_plane(pts, units)
        out["plane_z"].append(z)
        out["plane_d2"].append(d2)
        out["plane_w"].append(w)
    shapes = dict(n_class=(0, 3), box=(0, 6), coord_sum=(0, 3), faces=(0, 3))
    return {k: np.array(v, dtype=np.int64).reshape(np.shape(v) if v else shapes.get(k, (0,))) for k, v in out.items()}


def derive(table, k, units, scale_mm):
    """The float64 quantities of lesion k, the expressions of DESIGN.md 4y over Python integers."""
    u, s = units, scale_mm
    n = int(table["n"][k])
    box = [int(v) for v in table["box"][k]]
    sums = [int(v) for v in table["coord_sum"][k]]
    fx, fy, fz = (int(v) for v in table["faces"][k])
    d3, d2, w = int(table["d3"][k]), int(table["plane_d2"][k]), int(table["plane_w"][k])
    mm3 = float(n * u[0] * u[1] * u[2]) * (s * s * s)
    return dict(root=int(table["root"][k]), n=n, n_class=[int(v) for v in table["n_class"][k]], box=box,
                volume_mm3=mm3, volume_ml=mm3 / 1000.0,
                class_ml=[float(int(c) * u[0] * u[1] * u[2]) * (s * s * s) / 1000.0 for c in table["n_class"][k]],
                centroid_voxel=[sums[a] / n for a in range(3)],
                centroid_mm=[(sums[a] * u[a]) / n * s for a in range(3)],
                extent_mm=[float((box[2 * a + 1] - box[2 * a]) * u[a]) * s for a in range(3)],
                face_area_mm2=float(fx * u[1] * u[2] + fy * u[0] * u[2] + fz * u[0] * u[1]) * (s * s),
                diameter_mm=math.sqrt(d3) * s, plane_z=int(table["plane_z"][k]),
                plane_major_mm=math.sqrt(d2) * s, plane_minor_mm=w / math.sqrt(d2) * s if d2 else 0.0,
                plane_product_mm2=float(w) * (s * s))


def lesion_measurements(labels, region, spacing_mm=(1, 1, 1), connectivity=26):
    units, scale = spacing_units(spacing_mm)
    table = lesion_table(labels, region, units, connectivity)
    return [derive(table, k, units, scale) for k in range(len(table["n"]))]


def tumour_report(labels, spacing_mm=(1, 1, 1), connectivity=26, min_lesion_voxels=1):
    units, scale = spacing_units(spacing_mm)

    def ml(voxels):
        return float(voxels * units[0] * units[1] * units[2]) * (scale * scale * scale) / 1000.0

    report = {}
    for region in REGIONS:
        mask = region_mask(np.asarray(labels), region)
        lesions = lesion_measurements(labels, region, spacing_mm, connectivity)
        listed = sorted((m for m in lesions if m["n"] >= min_lesion_voxels), key=lambda m: (-m["n"], m["root"]))
        report[region] = dict(voxels=int(mask.sum()), ml=ml(int(mask.sum())),
                              class_ml=[ml(int((mask & (labels == c)).sum())) for c in (1, 2, 3)],
                              n_lesions=len(lesions), lesions=listed)
    return report


# ------------------------------------------------------------------ hull-vertex pruning, as the device applies it
def candidates(points, axes):
    """The rows of an int64 point set [n, k] that lack one of their two neighbours in the set along each of the
    first `axes` axes."""
    have = {tuple(p) for p in points.tolist()}
    keep = []
    for p in points.tolist():
        ok = True
        for a in range(axes):
            lo, hi = list(p), list(p)
            lo[a] -= 1
            hi[a] += 1
            ok = ok and not (tuple(lo) in have and tuple(hi) in have)
        if ok:
            keep.append(p)
    return np.array(keep, dtype=np.int64).reshape(-1, points.shape[1])


# ------------------------------------------------------------------ the volumes the tests share
RANDOM_SHAPES = ((13, 17, 9), (16, 16, 16), (33, 5, 20), (1, 40, 33), (1, 1, 40), (40, 1, 1))
RANDOM_P = (0.05, 0.10, 0.20, 0.31, 0.45, 0.7)
SPACINGS = ((1, 1, 1), (0.9375, 0.9375, 5), (1, 0.5, 2.5))


def random_volume(shape, p):
    """Bernoulli(p) foreground with labels 1..3, seeded by the case."""
    rng = np.random.default_rng([int(p * 100)] + list(shape))
    return np.where(rng.random(shape) < p, rng.integers(1, 4, shape), 0).astype(np.int16)


def embed(block, shape, corner, label=3):
    vol = np.zeros(shape, dtype=np.int16)
    vol[tuple(slice(c, c + s) for c, s in zip(corner, block.shape))] = np.where(block, label, 0)
    return vol


def box_block():
    return np.ones((5, 3, 2), dtype=bool)


def ellipsoid_block():
    x, y, z = np.ogrid[:14, :14, :6]
    return (x - 6.5) ** 2 + (y - 6.5) ** 2 + (2 * (z - 2.5)) ** 2 <= 36


def tie_block():
    block = np.zeros((3, 3, 1), dtype=bool)
    for x, y in ((0, 1), (1, 0), (1, 1), (2, 1), (2, 2)):
        block[x, y, 0] = True
    return block


def placements(block, margin=3):
    """{name: volume}: the block at a corner of a larger volume, on one of its faces and in its interior."""
    shape = tuple(s + 2 * margin for s in block.shape)
    return {"corner": embed(block, shape, (0, 0, 0)), "face": embed(block, shape, (margin, 0, margin)),
            "interior": embed(block, shape, (margin, margin, margin))}


def checkerboard_box(extent, parity_axes=3):
    """A volume with the checkerboard (the coordinates' sum even) of a box `extent` one voxel inside it, labels
    cycling 1..3.  parity_axes 2: the sum of x and y only (a footprint; give the box a z extent of 1)."""
    grid = np.indices(extent)
    board = grid[:parity_axes].sum(axis=0) % 2 == 0
    labels = (grid.sum(axis=0) % 3 + 1).astype(np.int16)
    vol = np.zeros(tuple(e + 2 for e in extent), dtype=np.int16)
    vol[1:-1, 1:-1, 1:-1] = np.where(board, labels, 0)
    return vol


def tile_boxes(tile, planar):
    """{voxel count: box extent} with tile - 1, tile, tile + 1 and 2 * tile + 1 checkerboard voxels, for tile 256."""
    assert tile == 256
    if planar:
        return {255: (15, 34, 1), 256: (16, 32, 1), 257: (19, 27, 1), 513: (27, 38, 1)}
    return {255: (5, 6, 17), 256: (8, 8, 8), 257: (3, 9, 19), 513: (6, 9, 19)}


def lattice_volume():
    """1 000 single-voxel lesions on the stride-2 lattice of a 20 x 20 x 20 volume."""
    vol = np.zeros((20, 20, 20), dtype=np.int16)
    grid = np.indices((10, 10, 10)).sum(axis=0)
    vol[::2, ::2, ::2] = (grid % 3 + 1).astype(np.int16)
    return vol


def face_touching_volume():
    """One lesion that touches all six faces: three crossing bars through a 9 x 8 x 7 volume, and a speck."""
    vol = np.zeros((9, 8, 7), dtype=np.int16)
    vol[:, 3:5, 3] = 1
    vol[4, :, 2:4] = 2
    vol[3:5, 4, :] = 3
    vol[0, 0, 6] = 3
    return vol


def gpu_volumes():
    """{name: label volume}: every volume of tests/test_gpu_measure.py but the CLI's."""
    vols = {f"random-{'x'.join(map(str, s))}-{p}": random_volume(s, p) for s in RANDOM_SHAPES for p in RANDOM_P}
    for count, extent in tile_boxes(256, False).items():
        vols[f"board3-{count}"] = checkerboard_box(extent)
    for count, extent in tile_boxes(256, True).items():
        vols[f"board2-{count}"] = checkerboard_box(extent, 2)
    vols["lattice"] = lattice_volume()
    vols["faces"] = face_touching_volume()
    for name, block in (("box", box_block()), ("ellipsoid", ellipsoid_block()), ("tie", tie_block())):
        for where, vol in placements(block).items():
            vols[f"{name}-{where}"] = vol
    vols["tie-alone"] = embed(tie_block(), (3, 3, 1), (0, 0, 0))
    return vols


@functools.lru_cache(maxsize=None)
def cached_volumes():
    return gpu_volumes()


@functools.lru_cache(maxsize=None)
def cached_table(name, region, units, connectivity):
    """lesion_table of a gpu_volumes() entry, computed once per session and shared (do not modify the arrays)."""
    return lesion_table(cached_volumes()[name], region, units, connectivity)
