"""The surface of every lesion of a label volume as a watertight triangle mesh, on the device (T1-T5,
csrc/gts_mesh.hip; definitions: DESIGN.md 4z), with what a mesh gives a measurement: a usable surface area, the mesh
volume, sphericity and surface-to-volume ratio, and a PLY file any viewer opens.

Marching tetrahedra on the six Kuhn tetrahedra of every cell of the region's mask (WT, CT or ET as in gts.measure)
padded by one layer of zeros, so a lesion on the volume's face closes there.  The level set of a piecewise-linear
function on a consistent triangulation is a closed 2-manifold: no ambiguous cases, no holes.  On a binary mask every
vertex is the midpoint of a lattice edge, so the raw mesh is integer geometry in half-index units (2 x the voxel-centre
index).  Vertices come by ascending (owner cell, edge direction), triangles by ascending (cell, tetrahedron, index),
normals pointing out of the tumour: the arrays do not depend on the launch.

A triangle belongs to the lesion (a component of gts.components, connectivity 6 or 26) of the inside corner of its
tetrahedron with the smallest root.  At connectivity 26 every lesion's triangles form closed surfaces disjoint from
every other lesion's.  At connectivity 6 two lesions can meet inside one tetrahedron; their per-lesion triangle sets
are then not closed and the per-lesion volumes are not volumes, while the region's totals are unaffected.

Smoothing is Taubin's lambda | mu scheme on positions in millimetres along the grid axes, so anisotropic voxels are
smoothed in millimetres; a gather in a fixed order, every bit the same on every run.  Everything runs on the current
stream.
"""
import math

import numpy as np
import torch

from . import _lib, _volume
from ._lesions import REGIONS, RegionLesions, grid_arg, table_head
from ._lib import check, current_stream, ptr

HEAD_I64 = _lib.const("GTS_MESH_HEAD_I64")
ROW_I64 = _lib.const("GTS_MESH_ROW_I64")
TAUBIN_LAMBDA, TAUBIN_MU = 0.5, -0.53
LIMITS = "every extent in [1, 4097], (X + 1)(Y + 1)(Z + 1) < 2^31, fewer than 2^31 vertices and 2^31 / 3 triangles"
FEATURE_KEYS = ("mesh_triangles", "mesh_area_mm2", "mesh_volume_ml", "smooth_area_mm2", "smooth_volume_ml",
                "sphericity", "surface_to_volume_per_mm")


def iterations_arg(n):
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 100000:
        raise _lib.GtsError(f"mesh: smooth_iterations {n!r} (0 .. 100000)")
    return n


def region_mesh(labels, region, spacing_mm=(1, 1, 1), connectivity=26, *, smooth_iterations=20, grid_blocks=0,
                mark=None):
    """The mesh of one region's lesions, a dict:

        vertices_half  int32 [V, 3] device    half-index units
        vertices_mm    float64 [V, 3] device  millimetres along the grid axes, half * u_a * s / 2, after
                                              smooth_iterations Taubin iterations (0: the raw mesh)
        faces          int32 [F, 3] device    face_lesion int32 [F] device, the face's lesion in lesion order
        face_area_mm2, face_volume_mm3  float64 [F] device: per face the area and p0 . (p1 x p2) / 6 of vertices_mm
        root, triangles [L], classes [L, 8], v6 [L]   numpy int64 in lesion order (ascending root, as gts.measure):
                       triangles per normal class 1..7 (4|nx| + 2|ny| + |nz|) and an eighth bin that stays 0; v6 / 48
                       is the raw mesh's volume in voxels
        units, scale_mm as gts.metrics.spacing_units gives them, smooth_iterations

    labels: int16 CUDA tensor [X, Y, Z] of internal labels; region "WT", "CT" or "ET" (or 0..2).  The table's head
    comes to the host once, for the sizes of the arrays.  grid_blocks: workgroups of every pass (0: the library's
    choice); no value depends on it.  mark: called with a stage's name once the stage is enqueued."""
    what = "region_mesh"
    grid_blocks, smooth_iterations = grid_arg(grid_blocks, what), iterations_arg(smooth_iterations)
    front = RegionLesions(labels, region, spacing_mm, connectivity, what, LIMITS, mark)
    return _mesh(front, smooth_iterations, grid_blocks)


def _mesh(front, smooth_iterations, grid_blocks=0):
    """region_mesh's own stages, T1-T5, on a front end."""
    what = "region_mesh"
    lib, roots, c_units, (x, y, z), mark = front.lib, front.roots, front.c_units, front.shape, front.mark
    units, scale_mm, dev = front.units, front.scale_mm, roots.device
    workspace, size = _volume.workspace(lib.gts_mesh_workspace, x, y, z, dev, what, LIMITS)
    ints = lib.gts_mesh_table_i64s(x, y, z, front.connectivity)
    table = torch.empty(ints, dtype=torch.int64, device=dev)
    stream = current_stream()
    check(lib.gts_mesh_classify(ptr(roots), x, y, z, front.connectivity, ptr(table), ints, ptr(workspace), size,
                                grid_blocks, stream), "gts_mesh_classify")
    mark("T1-T2 classify, scans")
    head = table_head(table, lambda head: HEAD_I64 + ROW_I64 * int(head[0]))
    n_lesions, n_vertices, n_faces = int(head[0]), int(head[1]), int(head[2])
    if n_vertices >= 2 ** 31 or 3 * n_faces >= 2 ** 31:
        raise _lib.GtsError(f"{what}: {n_vertices} vertices and {n_faces} triangles are outside the kernels' limits "
                            f"({LIMITS})")
    rows = head[HEAD_I64:].reshape(n_lesions, ROW_I64)
    order = np.argsort(rows[:, 0])
    rank = np.empty(n_lesions, dtype=np.int32)
    rank[order] = np.arange(n_lesions, dtype=np.int32)
    rows = rows[order]
    mark("table (copy, host)")
    vertices = torch.empty((n_vertices, 3), dtype=torch.int32, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    face_lesion = torch.empty(n_faces, dtype=torch.int32, device=dev)
    check(lib.gts_mesh_emit(ptr(roots), x, y, z, ptr(workspace), size, ptr(vertices), n_vertices, ptr(faces),
                            ptr(face_lesion), n_faces, grid_blocks, stream), "gts_mesh_emit")
    rank_dev = torch.from_numpy(rank).to(dev)
    check(lib.gts_mesh_relabel(ptr(face_lesion), n_faces, ptr(rank_dev), n_lesions, grid_blocks, stream),
          "gts_mesh_relabel")
    mark("T3 emit")
    positions = torch.empty((n_vertices, 3), dtype=torch.float64, device=dev)
    check(lib.gts_mesh_positions(ptr(vertices), n_vertices, c_units, scale_mm, ptr(positions), grid_blocks, stream),
          "gts_mesh_positions")
    if smooth_iterations:
        adj_size = int(lib.gts_mesh_adjacency_workspace(n_vertices))
        adj_ws = torch.empty(adj_size, dtype=torch.uint8, device=dev)
        row_start = torch.empty(n_vertices + 1, dtype=torch.int32, device=dev)
        neighbours = torch.empty(3 * n_faces, dtype=torch.int32, device=dev)
        check(lib.gts_mesh_adjacency(ptr(faces), n_faces, n_vertices, ptr(row_start), ptr(neighbours), ptr(adj_ws),
                                     adj_size, grid_blocks, stream), "gts_mesh_adjacency")
        mark("T4 adjacency")
        other = torch.empty_like(positions)
        check(lib.gts_mesh_smooth(ptr(row_start), ptr(neighbours), n_vertices, n_faces, ptr(positions), ptr(other),
                                  TAUBIN_LAMBDA, TAUBIN_MU, smooth_iterations, grid_blocks, stream), "gts_mesh_smooth")
        mark("T5 smooth")
    area = torch.empty(n_faces, dtype=torch.float64, device=dev)
    volume = torch.empty(n_faces, dtype=torch.float64, device=dev)
    check(lib.gts_mesh_terms(ptr(positions), ptr(faces), n_vertices, n_faces, ptr(area), ptr(volume), grid_blocks,
                             stream), "gts_mesh_terms")
    mark("T5 terms")
    return dict(vertices_half=vertices, vertices_mm=positions, faces=faces, face_lesion=face_lesion,
                face_area_mm2=area, face_volume_mm3=volume, root=rows[:, 0].copy(), triangles=rows[:, 1].copy(),
                classes=rows[:, 2:10].copy(), v6=rows[:, 10].copy(), units=tuple(units), scale_mm=scale_mm,
                smooth_iterations=smooth_iterations)


def _host(a):
    """A mesh array on the host: device tensors are copied, numpy arrays (a mesh built on the host) pass."""
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def raw_area_mm2(classes, units, scale_mm):
    """sum over the classes k = 1..7 in ascending order, left to right, of count_k * (0.5 * sqrt((n_x u_y u_z)^2 +
    (n_y u_x u_z)^2 + (n_z u_x u_y)^2) / 4.0 * (s * s)), n = (k >> 2 & 1, k >> 1 & 1, k & 1)."""
    ux, uy, uz = units
    total = 0.0
    for k in range(1, 8):
        nx, ny, nz = (k >> 2) & 1, (k >> 1) & 1, k & 1
        norm = math.sqrt(float((nx * uy * uz) ** 2 + (ny * ux * uz) ** 2 + (nz * ux * uy) ** 2))
        total = total + int(classes[k - 1]) * (0.5 * norm / 4.0 * (scale_mm * scale_mm))
    return total


def lesion_sums(mesh):
    """(area_mm2 [L], volume_mm3 [L]) float64: the per-face terms summed per lesion on the host by np.bincount, which
    adds in face order; the faces' order is fixed, so the sums are the same bits on every run."""
    n = len(mesh["root"])
    lesion = _host(mesh["face_lesion"])
    area = np.bincount(lesion, weights=_host(mesh["face_area_mm2"]), minlength=n)
    volume = np.bincount(lesion, weights=_host(mesh["face_volume_mm3"]), minlength=n)
    return area[:n], volume[:n]


def shape_features(mesh):
    """Per lesion (lesion order) a dict of fixed float64 expressions, with s = scale_mm, u = units:

        mesh_triangles            the lesion's triangles
        mesh_area_mm2             raw_area_mm2 of its class counts
        mesh_volume_ml            float(v6 u_x u_y u_z) / 48.0 * (s * s * s) / 1000.0
        smooth_area_mm2           the sum of its faces' areas on vertices_mm (the raw mesh at 0 iterations)
        smooth_volume_ml          the sum of its faces' p0 . (p1 x p2) / 6, / 1000.0
        sphericity                (36 pi V^2)^(1/3) / A             surface_to_volume_per_mm   A / V

    A and V the smooth area and volume in mm (0.0 where V is not positive).  At connectivity 6 a lesion's triangle set
    need not be closed (see the module's docstring)."""
    u, s = mesh["units"], mesh["scale_mm"]
    area, volume = lesion_sums(mesh)
    out = []
    for k in range(len(mesh["root"])):
        a, v = float(area[k]), float(volume[k])
        ok = v > 0.0 and a > 0.0
        out.append(dict(mesh_triangles=int(mesh["triangles"][k]),
                        mesh_area_mm2=raw_area_mm2(mesh["classes"][k], u, s),
                        mesh_volume_ml=float(int(mesh["v6"][k]) * u[0] * u[1] * u[2]) / 48.0 * (s * s * s) / 1000.0,
                        smooth_area_mm2=a, smooth_volume_ml=v / 1000.0,
                        sphericity=(36.0 * math.pi * v * v) ** (1.0 / 3.0) / a if ok else 0.0,
                        surface_to_volume_per_mm=a / v if ok else 0.0))
    return out


def write_ply(path, mesh, affine=None):
    """Binary little-endian PLY: float32 vertices, int32 faces (uchar count 3) and a per-face int32 `lesion`.
    Without an affine the vertices are vertices_mm, millimetres along the grid axes.  With a 4 x 4 voxel-to-world
    affine they go through it: mm / spacing gives the voxel index, the affine NIfTI world coordinates.  A `comment`
    line names the frame.  An empty mesh writes a valid empty file."""
    mm = _host(mesh["vertices_mm"]).reshape(-1, 3)
    frame = "millimetres along the grid axes, origin at the centre of voxel (0, 0, 0)"
    if affine is not None:
        affine = np.asarray(affine, dtype=np.float64)
        if affine.shape != (4, 4):
            raise _lib.GtsError(f"write_ply: affine of shape {affine.shape} (4 x 4)")
        spacing = np.array(mesh["units"], dtype=np.float64) * mesh["scale_mm"]
        mm = (mm / spacing) @ affine[:3, :3].T + affine[:3, 3]
        frame = "NIfTI world coordinates (the file's voxel-to-world affine applied to voxel indices)"
    faces = _host(mesh["faces"]).reshape(-1, 3)
    lesion = _host(mesh["face_lesion"])
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"comment frame: {frame}\n"
              f"comment smoothing: {mesh['smooth_iterations']} Taubin iterations\n"
              f"element vertex {len(mm)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(faces)}\nproperty list uchar int vertex_indices\nproperty int lesion\n"
              "end_header\n")
    record = np.zeros(len(faces), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,)), ("lesion", "<i4")]))
    record["n"], record["v"], record["lesion"] = 3, faces, lesion
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(mm.astype("<f4").tobytes())
        f.write(record.tobytes())


__all__ = ["REGIONS", "FEATURE_KEYS", "region_mesh", "shape_features", "lesion_sums", "raw_area_mm2", "write_ply"]
