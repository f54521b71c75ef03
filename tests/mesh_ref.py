"""The tumour surfaces of gts.mesh in plain numpy and Python, written from the definition and
independent of the package: marching tetrahedra on the six Kuhn tetrahedra of every cell of the zero-padded mask,
vertices and triangles in the defined order, the per-lesion integer table, the ordered-loop Taubin smoothing and the
per-triangle float64 terms.  The closed forms the tests hold it against are kept in the tests, not here."""
import functools
import itertools
import math

import numpy as np
from scipy import ndimage

from tests import measure_ref

AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
# tetrahedron t: the path 000 -> 111 adding the axes in the order of the t-th permutation of (x, y, z), lexicographic
PATHS = []
for _perm in itertools.permutations(range(3)):
    _path = [(0, 0, 0)]
    for _axis in _perm:
        _path.append(tuple(a + b for a, b in zip(_path[-1], AXES[_axis])))
    PATHS.append(_path)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def tet_triangles(inside):
    """The triangles of one tetrahedron: a list of triples of (path position, path position) midpoint edges, before
    orientation.  inside: four booleans in path order."""
    ins = [k for k in range(4) if inside[k]]
    outs = [k for k in range(4) if not inside[k]]
    if len(ins) == 1:
        return [[(ins[0], o) for o in outs]]
    if len(outs) == 1:
        return [[(outs[0], i) for i in ins]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        q = [(a, c), (a, d), (b, d), (b, c)]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def normal_class(n):
    """1..7 = 4|nx| + 2|ny| + |nz| for the seven non-zero normals of {0,1}^3, 8 for anything else."""
    a = tuple(abs(v) for v in n)
    return 4 * a[0] + 2 * a[1] + a[2] if max(a) == 1 else 8


def surface(mask, lab=None):
    """(vertices int32 [V, 3] in half-index units, faces int32 [F, 3], face roots int64 [F]) of a boolean volume.
    lab: an integer volume of lesion roots (0 outside); a triangle takes the smallest root among the inside corners
    of its tetrahedron.  Without it every face root is 1."""
    mask = np.asarray(mask, dtype=bool)
    if lab is None:
        lab = mask.astype(np.int64)
    pad = np.pad(mask, 1)
    plab = np.pad(np.asarray(lab, dtype=np.int64), 1)
    cells = tuple(n + 1 for n in mask.shape)
    verts = {}                    # (owner cell linear index, d) -> the half-index point
    tris = []                     # ((cell, t, k), three vertex keys, root)
    corners = [pad[tuple(slice(d[a], d[a] + cells[a]) for a in range(3))] for d in itertools.product((0, 1), repeat=3)]
    occupied = np.logical_or.reduce(corners) & ~np.logical_and.reduce(corners)
    for cx, cy, cz in np.argwhere(occupied):          # the cells whose eight corners are not all alike, in C order
        cell = (int(cx), int(cy), int(cz))
        m = tuple(c - 1 for c in cell)                # the minimum corner's voxel index
        index = (cell[0] * cells[1] + cell[1]) * cells[2] + cell[2]
        for t, path in enumerate(PATHS):
            corner = [tuple(cell[a] + path[k][a] for a in range(3)) for k in range(4)]      # in the padded volume
            inside = [bool(pad[c]) for c in corner]
            ins = [k for k in range(4) if inside[k]]
            outs = [k for k in range(4) if not inside[k]]
            if not ins or not outs:
                continue
            root = min(int(plab[corner[k]]) for k in ins)
            voxel = [tuple(m[a] + path[k][a] for a in range(3)) for k in range(4)]
            sum_in = [sum(path[k][a] for k in ins) for a in range(3)]
            sum_out = [sum(path[k][a] for k in outs) for a in range(3)]
            # (centroid of O - centroid of I) times |I| |O|
            outward = tuple(len(ins) * sum_out[a] - len(outs) * sum_in[a] for a in range(3))
            for k, tri in enumerate(tet_triangles(inside)):
                keys, pts = [], []
                for a, b in tri:
                    lo, hi = min(a, b), max(a, b)     # path order: the lower end comes first
                    d = tuple(path[hi][i] - path[lo][i] for i in range(3))
                    owner = tuple(cell[i] + path[lo][i] for i in range(3))
                    key = ((owner[0] * cells[1] + owner[1]) * cells[2] + owner[2], 4 * d[0] + 2 * d[1] + d[2])
                    point = tuple(voxel[lo][i] + voxel[hi][i] for i in range(3))
                    assert verts.setdefault(key, point) == point
                    keys.append(key)
                    pts.append(point)
                if _dot(_cross(_sub(pts[1], pts[0]), _sub(pts[2], pts[0])), outward) < 0:
                    keys[1], keys[2] = keys[2], keys[1]
                tris.append(((index, t, k), keys, root))
    order = sorted(verts)
    number = {key: i for i, key in enumerate(order)}
    vertices = np.array([verts[key] for key in order], dtype=np.int32).reshape(-1, 3)
    tris.sort(key=lambda item: item[0])
    faces = np.array([[number[key] for key in keys] for _, keys, _ in tris], dtype=np.int32).reshape(-1, 3)
    roots = np.array([root for _, _, root in tris], dtype=np.int64)
    return vertices, faces, roots


def lesion_roots(mask, connectivity):
    """Per voxel 1 + the smallest C-order index of its component, 0 outside."""
    structure = ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1)
    lab, count = ndimage.label(mask, structure=structure)
    first = np.zeros(count + 1, dtype=np.int64)
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    first[flat[idx][::-1]] = idx[::-1] + 1            # the last write is the smallest index
    return first[lab]


def integer_table(vertices, faces, face_roots):
    """{root, triangles, classes [L, 8] (class 1..7, then anything else), v6} per lesion in ascending root, exact."""
    roots = sorted(set(int(r) for r in face_roots))
    row = {r: i for i, r in enumerate(roots)}
    tris = [0] * len(roots)
    classes = [[0] * 8 for _ in roots]
    v6 = [0] * len(roots)
    for f, r in zip(faces.tolist(), face_roots.tolist()):
        p = [tuple(int(v) for v in vertices[i]) for i in f]
        i = row[r]
        tris[i] += 1
        classes[i][normal_class(_cross(_sub(p[1], p[0]), _sub(p[2], p[0]))) - 1] += 1
        v6[i] += _dot(p[0], _cross(p[1], p[2]))
    return dict(root=np.array(roots, dtype=np.int64), triangles=np.array(tris, dtype=np.int64),
                classes=np.array(classes, dtype=np.int64).reshape(-1, 8), v6=np.array(v6, dtype=np.int64))


def region_mesh(labels, region, units=(1, 1, 1), connectivity=26):
    """The raw mesh of a region of a label volume and its table; face_lesion indexes the table's rows."""
    mask = measure_ref.region_mask(np.asarray(labels), region)
    vertices, faces, face_roots = surface(mask, lesion_roots(mask, connectivity))
    table = integer_table(vertices, faces, face_roots)
    return dict(vertices_half=vertices, faces=faces, face_lesion=np.searchsorted(table["root"], face_roots).astype(np.int32),
                **table)


def closed_form_v48(mask):
    """48 x the volume in voxels: the sum over tetrahedra of (0, 1, 4, 7, 8)[number of inside corners]."""
    pad = np.pad(np.asarray(mask, dtype=bool), 1)
    total = 0
    for path in PATHS:
        count = sum(pad[tuple(slice(p[a], pad.shape[a] - 1 + p[a]) for a in range(3))].astype(np.int64) for p in path)
        total += int(np.array([0, 1, 4, 7, 8])[count].sum())
    return total


def raw_area_mm2(classes, units, scale_mm):
    """sum_k count_k * 0.5 * sqrt((nx uy uz)^2 + (ny ux uz)^2 + (nz ux uy)^2) / 4 * s^2 over the classes in ascending
    order, left to right."""
    ux, uy, uz = units
    total = 0.0
    for k in range(1, 8):
        nx, ny, nz = (k >> 2) & 1, (k >> 1) & 1, k & 1
        total = total + int(classes[k - 1]) * (0.5 * math.sqrt(float((nx * uy * uz) ** 2 + (ny * ux * uz) ** 2 +
                                                                     (nz * ux * uy) ** 2)) / 4.0 * (scale_mm * scale_mm))
    return total


def positions_mm(vertices, units, scale_mm):
    """float(half * u_a) * s / 2.0."""
    return (vertices.astype(np.int64) * np.array(units, dtype=np.int64)).astype(np.float64) * scale_mm / 2.0


def neighbours(faces, n_vertices):
    """Per vertex the ascending list of { b : (a, b) is a directed edge of a face }."""
    rows = [[] for _ in range(n_vertices)]
    for a, b, c in faces.tolist():
        rows[a].append(b)
        rows[b].append(c)
        rows[c].append(a)
    return [sorted(r) for r in rows]


def smooth(positions, rows, iterations, lam=0.5, mu=-0.53):
    """Taubin: `iterations` times a Jacobi step with factor lam, then one with mu.  The neighbours' sum runs left to
    right in ascending id; one float64 operation at a time."""
    p = positions.copy()
    for _ in range(iterations):
        for factor in (lam, mu):
            q = np.empty_like(p)
            for v, row in enumerate(rows):
                total = p[row[0]].copy()
                for b in row[1:]:
                    total = total + p[b]
                q[v] = p[v] + factor * (total / float(len(row)) - p[v])
            p = q
    return p


def face_terms(positions, faces):
    """(area, volume) per face: 0.5 sqrt((cx cx + cy cy) + cz cz) with c = (p1 - p0) x (p2 - p0), and ((p0x dx + p0y dy)
    + p0z dz) / 6 with d = p1 x p2."""
    p0, p1, p2 = (positions[faces[:, i]] for i in range(3))
    a, b = p1 - p0, p2 - p0
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    dx = p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1]
    dy = p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2]
    dz = p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]
    return area, ((p0[:, 0] * dx + p0[:, 1] * dy) + p0[:, 2] * dz) / 6.0


def directed_edges(faces):
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])


def is_closed_manifold(faces):
    """Every directed edge occurs once and its reverse once."""
    edges = directed_edges(np.asarray(faces, dtype=np.int64))
    keys = set(map(tuple, edges.tolist()))
    return len(keys) == len(edges) and all((b, a) in keys for a, b in keys)


def euler_characteristic(n_vertices, faces):
    edges = directed_edges(np.asarray(faces, dtype=np.int64))
    undirected = {(min(a, b), max(a, b)) for a, b in edges.tolist()}
    return n_vertices - len(undirected) + len(faces)


def ball(radius2, size):
    """x^2 + y^2 + z^2 <= radius2 about the centre of a size^3 volume."""
    g = np.ogrid[:size, :size, :size]
    c = size // 2
    return sum((a - c) ** 2 for a in g) <= radius2


def all_configurations():
    """The 256 corner configurations as 2 x 2 x 2 blocks four voxels apart in one 66 x 66 x 4 int16 volume (label 3)."""
    vol = np.zeros((64, 64, 4), dtype=np.int16)
    for m in range(256):
        block = np.array([(m >> d) & 1 for d in range(8)], dtype=np.int16).reshape(2, 2, 2) * 3
        x, y = 4 * (m // 16), 4 * (m % 16)
        vol[x:x + 2, y:y + 2, 1:3] = block
    return np.pad(vol, ((1, 1), (1, 1), (0, 0)))


@functools.lru_cache(maxsize=None)
def cached_mesh(name, region, units, connectivity):
    """region_mesh of a measure_ref.gpu_volumes() entry or of one of this module's, once per session (do not modify)."""
    return region_mesh(volumes()[name], region, units, connectivity)


# Volumes whose number of active cells (cells with triangles), of vertices or of triangles sits at a workgroup edge:
# 2 x 2 x 2 blocks (bit d of the code: corner d = 4 x + 2 y + z is set) three voxels apart along x.  On every mask tried
# (all 2 x 2 x 2 and 1 x 2 x 3 blocks) the vertex count is even and the triangle count a multiple of 4, so 255, 257 and
# 513 cannot be had for those two; the nearest counts stand in: 254 / 258 / 514 vertices, 252 / 260 / 516 triangles.
COUNT_RECIPES = {
    ("cells", 255): [127] * 9 + [30], ("cells", 256): [127] * 9 + [31], ("cells", 257): [127] * 9 + [61],
    ("cells", 513): [127] * 19 + [22],
    ("vertices", 254): [127, 126, 63, 22], ("vertices", 256): [127, 127, 63, 22], ("vertices", 258): [126, 126, 126, 22],
    ("vertices", 514): [127] * 5 + [126, 126],
    ("triangles", 252): [126, 47], ("triangles", 256): [126, 31], ("triangles", 260): [191, 63],
    ("triangles", 516): [191, 126, 126, 23],
}


def count_volume(codes):
    vol = np.zeros((3 * len(codes) - 1, 2, 2), dtype=np.int16)
    for k, code in enumerate(codes):
        vol[3 * k:3 * k + 2] = np.array([(code >> d) & 1 for d in range(8)], dtype=np.int16).reshape(2, 2, 2) * (1 + k % 3)
    return vol


def active_cells(mask):
    """The number of cells of the padded mask whose eight corners are not all alike."""
    pad = np.pad(np.asarray(mask, dtype=bool), 1)
    cells = tuple(n + 1 for n in mask.shape)
    corners = [pad[tuple(slice(d[a], d[a] + cells[a]) for a in range(3))] for d in itertools.product((0, 1), repeat=3)]
    return int((np.logical_or.reduce(corners) & ~np.logical_and.reduce(corners)).sum())


def read_ply(path):
    """(comments, vertices float32 [V, 3], faces int32 [F, 3], lesion int32 [F]) of a file gts.mesh.write_ply wrote:
    the tests' own reader."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = [line.split() for line in lines if line.startswith("element")]
    assert [e[1] for e in elements] == ["vertex", "face"]
    props = [line for line in lines if line.startswith("property")]
    assert props == ["property float x", "property float y", "property float z",
                     "property list uchar int vertex_indices", "property int lesion"]
    n_v, n_f = int(elements[0][2]), int(elements[1][2])
    vertices = np.frombuffer(raw, dtype="<f4", count=3 * n_v, offset=end).reshape(n_v, 3)
    record = np.dtype([("n", "u1"), ("v", "<i4", (3,)), ("lesion", "<i4")])
    body = np.frombuffer(raw, dtype=record, count=n_f, offset=end + 12 * n_v)
    assert len(raw) == end + 12 * n_v + 17 * n_f and (body["n"] == 3).all()
    return [line for line in lines if line.startswith("comment")], vertices, body["v"], body["lesion"]


@functools.lru_cache(maxsize=None)
def volumes():
    vols = dict(measure_ref.cached_volumes())
    vols["configurations"] = all_configurations()
    vols["ball8"] = np.where(ball(64, 21), 3, 0).astype(np.int16)
    vols["one"] = np.full((1, 1, 1), 3, dtype=np.int16)
    vols["plate"] = np.full((3, 3, 1), 2, dtype=np.int16)
    full = np.zeros((5, 4, 6), dtype=np.int16)
    full[:, 1:3, 2:4] = 1
    full[2, :, 2:4] = 2
    full[1:3, 1:3, :] = 3
    vols["six-faces"] = full
    for (what, count), codes in COUNT_RECIPES.items():
        vols[f"{what}-{count}"] = count_volume(codes)
    for z1 in (63, 64, 65):
        rng = np.random.default_rng(z1)
        vols[f"row-{z1}"] = np.where(rng.random((3, 4, z1 - 1)) < 0.4, rng.integers(1, 4, (3, 4, z1 - 1)), 0).astype(np.int16)
    return vols
