// T1-T5: the device half of the tumour surfaces (gts/mesh.py).  A watertight triangle mesh of a
// region's mask by marching tetrahedra, its per-lesion integer table, the vertex adjacency and Taubin smoothing.  The
// region mask comes from L1 (dilation 0) and its components from C1-C3, both unchanged.
//
// Definitions.  roots int32 [X][Y][Z] (Z contiguous): 0 outside the mask, else 1 + the smallest linear index of the
// voxel's lesion.  The mask is padded by one layer of zeros; cell (cx, cy, cz), 0 <= c_a <= N_a, has its minimum corner
// at voxel m = (cx - 1, cy - 1, cz - 1); cells are numbered in C order over (X + 1)(Y + 1)(Z + 1).  Corner d = 4 dx +
// 2 dy + dz of a cell is voxel m + (dx, dy, dz).  Each cell splits into the six Kuhn tetrahedra: tetrahedron t walks
// from corner 0 to corner 7 adding the axes in the order of the t-th permutation of (x, y, z), lexicographic; its
// vertices v0..v3 are in path order.  Coordinates are half-index units, 2 x the voxel-centre index, so the midpoint of
// a lattice edge is the integer sum of its two corners.
//   vertex     the midpoint of a lattice edge with one end inside; its identity is (owner cell, d): the owner's minimum
//              corner is the edge's lower end and d in 1..7 its direction.  Listed by ascending (owner cell, d).
//   triangles  of a tetrahedron with inside vertices I and outside vertices O (ascending path position), m(a, b) the
//              midpoint: |I| = 1: (m(a,o1), m(a,o2), m(a,o3)); |O| = 1: (m(o,i1), m(o,i2), m(o,i3)); |I| = 2, I = {a<b},
//              O = {c<d}: q0 = m(a,c), q1 = m(a,d), q2 = m(b,d), q3 = m(b,c) give (q0,q1,q2) and (q0,q2,q3).  The last two
//              vertices are swapped when the integer normal (p1-p0) x (p2-p0) has a negative dot product with |I| sum(O)
//              - |O| sum(I) (the outward direction).  Listed by ascending (cell, t, index within the tetrahedron).
//   lesion     a triangle belongs to the lesion of the smallest root among its tetrahedron's inside corners.
//   table      per lesion: the number of triangles, their count per normal class (class k = 4|n_x| + 2|n_y| + |n_z| for
//              the seven non-zero normals in {0,1}^3, anything else in an eighth bin that stays 0) and V6 = sum p0.(p1xp2),
//              48 x the enclosed volume in voxels.  V6 is summed modulo 2^64, which is exact whenever |V6| < 2^63: always
//              for a closed surface (every lesion at connectivity 26).
//
//   T1  classify.  One thread per cell, Z fastest: a lane loads the four roots of its cell's upper z face and takes the
//       lower face from the lane before it (lane 0 and row starts load or zero it): 4 loads per cell, not 8.  The
//       8-bit corner mask is stored (the 7-bit mask of owned crossing edges is corner 0's bit xor each other bit);
//       vertex and triangle counts come from the mask; a workgroup writes the totals of its 256 cells.  The same pass
//       adds the table's terms to each lesion's row, lanes of one lesion summed in the wave first.
//   T2  scans.  One workgroup per array turns the per-256-cell totals into exclusive bases (int64), 16 entries per
//       thread and trip; the emit passes redo the scan inside their 256 cells.  Workspace: 1 byte + 4 bytes (vertex
//       base) per cell, 4 bytes per voxel (lesion slot), 16 bytes per 256 cells.
//   T3  emit.  Vertices (int32 half-index triples) with each cell's vertex base; then faces: a vertex's index is
//       base[owner] + the rank of d in the owner's edge mask.
//   T4  adjacency.  Degrees by integer atomics over the 3F directed edges, scan, fill through cursors, every row then
//       sorted ascending by one thread.  A lattice edge has at most 6 tetrahedra around it, each with at most 2
//       triangles at its midpoint, so a degree is at most 12; rows are of any length all the same.
//   T5  smooth and terms.  P' = P + f (mean of the neighbours - P), the sum left to right in ascending neighbour id, a
//       gather with two buffers: float64 without contraction, every bit fixed.  Per triangle then the area and
//       p0.(p1 x p2) / 6.
//
// Integer atomics and plain vector stores only in T1-T4; no float atomics anywhere: identical results on every run and
// at every grid_blocks.  Limits: every extent in [1, 4097], (X+1)(Y+1)(Z+1) < 2^31, vertices and triangles < 2^31 each.
#include "gts_lesions.h"

namespace gts {
namespace {

constexpr int kRow = GTS_MESH_ROW_I64;
constexpr int kHead = GTS_MESH_HEAD_I64;
typedef unsigned long long u64;

enum { fRoot = 0, fTris = 1, fClass = 2, fV6 = 10 };                 // row fields
enum { hLesions = 0, hVertices = 1, hTriangles = 2 };                // header fields
static_assert(hLesions == 0 && fRoot == 0, "the table convention of lesion_rows_kernel");

// ------------------------------------------------------------------ the 16-case rule, at compile time
struct I3 {
  int x, y, z;
};
constexpr I3 corner_offset(int c) { return {(c >> 2) & 1, (c >> 1) & 1, c & 1}; }
constexpr I3 add(I3 a, I3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
constexpr I3 sub(I3 a, I3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
constexpr I3 scale(int k, I3 a) { return {k * a.x, k * a.y, k * a.z}; }
constexpr I3 cross(I3 a, I3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
constexpr int dot(I3 a, I3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
constexpr int iabs(int v) { return v < 0 ? -v : v; }

constexpr int kPerm[6][3] = {{4, 2, 1}, {4, 1, 2}, {2, 4, 1}, {2, 1, 4}, {1, 4, 2}, {1, 2, 4}};  // axis bits, x y z
// the cube corner at path position k of tetrahedron t
constexpr int tet_corner(int t, int k) {
  int c = 0;
  for (int i = 0; i < k; ++i) c |= kPerm[t][i];
  return c;
}

// one (tetrahedron, inside set) case.  A triangle's vertex is its lattice edge, lower corner | upper corner << 3.
struct TetCase {
  int8_t tris;
  uint8_t edge[2][3];
  int8_t cls[2];     // normal class - 1 (0..6), 7 for anything else
  int8_t det;        // sum of p0.(p1 x p2) in the cell's own half-index frame
  int8_t nx, ny, nz; // sum of the oriented integer normals: V6 = det + 2 m.n
  uint8_t path[4];   // the tetrahedron's cube corners in path order
};

constexpr TetCase make_case(int t, int s) {  // bit k of s: path vertex k is inside
  TetCase out = {};
  for (int k = 0; k < 4; ++k) out.path[k] = static_cast<uint8_t>(tet_corner(t, k));
  int in[4] = {}, outv[4] = {}, ni = 0, no = 0;
  for (int k = 0; k < 4; ++k) {
    if ((s >> k) & 1) in[ni++] = k; else outv[no++] = k;
  }
  int pair[2][3][2] = {};
  if (ni == 1) {
    out.tris = 1;
    for (int j = 0; j < 3; ++j) pair[0][j][0] = in[0], pair[0][j][1] = outv[j];
  } else if (no == 1) {
    out.tris = 1;
    for (int j = 0; j < 3; ++j) pair[0][j][0] = outv[0], pair[0][j][1] = in[j];
  } else if (ni == 2) {
    out.tris = 2;
    const int q[4][2] = {{in[0], outv[0]}, {in[0], outv[1]}, {in[1], outv[1]}, {in[1], outv[0]}};
    const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
    for (int r = 0; r < 2; ++r)
      for (int j = 0; j < 3; ++j) pair[r][j][0] = q[pick[r][j]][0], pair[r][j][1] = q[pick[r][j]][1];
  }
  I3 sum_in = {0, 0, 0}, sum_out = {0, 0, 0};
  for (int k = 0; k < ni; ++k) sum_in = add(sum_in, corner_offset(tet_corner(t, in[k])));
  for (int k = 0; k < no; ++k) sum_out = add(sum_out, corner_offset(tet_corner(t, outv[k])));
  const I3 outward = sub(scale(ni, sum_out), scale(no, sum_in));
  int det = 0;
  I3 normals = {0, 0, 0};
  for (int r = 0; r < out.tris; ++r) {
    int lo[3] = {}, hi[3] = {};
    I3 p[3] = {};
    for (int j = 0; j < 3; ++j) {
      const int a = pair[r][j][0], b = pair[r][j][1];
      lo[j] = tet_corner(t, a < b ? a : b), hi[j] = tet_corner(t, a < b ? b : a);
      p[j] = add(corner_offset(lo[j]), corner_offset(hi[j]));
    }
    I3 n = cross(sub(p[1], p[0]), sub(p[2], p[0]));
    if (dot(n, outward) < 0) {
      const int l = lo[1], h = hi[1];
      const I3 pp = p[1];
      lo[1] = lo[2], hi[1] = hi[2], p[1] = p[2];
      lo[2] = l, hi[2] = h, p[2] = pp;
      n = scale(-1, n);
    }
    for (int j = 0; j < 3; ++j) out.edge[r][j] = static_cast<uint8_t>(lo[j] | (hi[j] << 3));
    const int ax = iabs(n.x), ay = iabs(n.y), az = iabs(n.z);
    out.cls[r] = static_cast<int8_t>(ax <= 1 && ay <= 1 && az <= 1 && ax + ay + az > 0 ? 4 * ax + 2 * ay + az - 1 : 7);
    det += dot(p[0], cross(p[1], p[2]));
    normals = add(normals, n);
  }
  out.det = static_cast<int8_t>(det);
  out.nx = static_cast<int8_t>(normals.x), out.ny = static_cast<int8_t>(normals.y);
  out.nz = static_cast<int8_t>(normals.z);
  return out;
}

struct TetTable {
  TetCase c[6][16];
};
constexpr TetTable make_tet_table() {
  TetTable out = {};
  for (int t = 0; t < 6; ++t)
    for (int s = 0; s < 16; ++s) out.c[t][s] = make_case(t, s);
  return out;
}
constexpr TetTable kTetHost = make_tet_table();

// the 4-bit case of tetrahedron t in a cell of corner mask m
constexpr __host__ __device__ int tet_case(int t, unsigned m) {
  // path corners: 0, first axis, first | second, 7
  const int a = t == 0 || t == 1 ? 4 : (t == 2 || t == 3 ? 2 : 1);
  const int b = t == 0 ? 6 : t == 1 ? 5 : t == 2 ? 6 : t == 3 ? 3 : t == 4 ? 5 : 3;
  return static_cast<int>((m & 1u) | (((m >> a) & 1u) << 1) | (((m >> b) & 1u) << 2) | (((m >> 7) & 1u) << 3));
}

struct MaskTable {
  uint8_t tris[256];
};
constexpr MaskTable make_mask_table() {
  MaskTable out = {};
  for (int m = 0; m < 256; ++m) {
    int n = 0;
    for (int t = 0; t < 6; ++t) n += kTetHost.c[t][tet_case(t, static_cast<unsigned>(m))].tris;
    out.tris[m] = static_cast<uint8_t>(n);
  }
  return out;
}
constexpr MaskTable kMaskHost = make_mask_table();

constexpr bool tables_hold() {
  for (int t = 0; t < 6; ++t) {
    if (tet_corner(t, 0) != 0 || tet_corner(t, 3) != 7) return false;
    for (int s = 0; s < 16; ++s) {
      const TetCase& c = kTetHost.c[t][s];
      if (tet_case(t, 0u) != 0 || tet_case(t, 255u) != 15) return false;
      if (tet_case(t, 1u << tet_corner(t, 1)) != 2 || tet_case(t, 1u << tet_corner(t, 2)) != 4) return false;
      for (int r = 0; r < c.tris; ++r)
        if (c.cls[r] == 7) return false;             // only the seven normals of {0,1}^3 occur
      if ((s == 0 || s == 15) != (c.tris == 0)) return false;
    }
  }
  return kMaskHost.tris[0] == 0 && kMaskHost.tris[255] == 0 && kMaskHost.tris[1] == 6 && kMaskHost.tris[128] == 6;
}
static_assert(tables_hold(), "the 16-case rule: path corners, normal classes and triangle counts");

__constant__ TetTable kTet = kTetHost;
__constant__ MaskTable kMask = kMaskHost;

// the 7-bit mask of a cell's owned crossing edges: bit d - 1, corner 0 and corner d differ
__device__ __forceinline__ unsigned edge_mask(unsigned m) { return ((m >> 1) ^ (0u - (m & 1u))) & 127u; }

struct Cells {
  int X, Y, Z, CY, CZ;
  int64_t cells, voxels;
};

__device__ __forceinline__ int root_at(const int* __restrict__ roots, const Cells& g, int x, int y, int z) {
  const bool in = x >= 0 && x < g.X && y >= 0 && y < g.Y && z >= 0 && z < g.Z;
  return in ? roots[(int64_t{x} * g.Y + y) * g.Z + z] : 0;
}

// ------------------------------------------------------------------ T1
// what one tetrahedron adds to its lesion's row (every root took one through gts_lesions.h's lesion_rows_kernel)
struct TetTerms {
  int root;      // the smallest root among the inside corners; 0: no triangle
  int tris;
  u64 cls[2];    // eight 16-bit counters, class - 1 = 4 * word + field
  int64_t v6;
};

template <int T>
__device__ __forceinline__ TetTerms tet_terms(unsigned m, const int (&r)[8], int mx, int my, int mz) {
  const TetCase& c = kTet.c[T][tet_case(T, m)];
  TetTerms out = {0, c.tris, {0, 0}, 0};
  if (c.tris == 0) return out;
  constexpr int corners[4] = {tet_corner(T, 0), tet_corner(T, 1), tet_corner(T, 2), tet_corner(T, 3)};
  int root = INT32_MAX;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = r[corners[k]];
    if (v != 0 && v < root) root = v;
  }
  out.root = root;
  for (int j = 0; j < c.tris; ++j) {  // no indexing by the class: the pair stays in registers
    const u64 one = u64{1} << (16 * (c.cls[j] & 3));
    if (c.cls[j] >> 2) out.cls[1] += one; else out.cls[0] += one;
  }
  out.v6 = c.det + 2 * (int64_t{mx} * c.nx + int64_t{my} * c.ny + int64_t{mz} * c.nz);
  return out;
}

// the terms of the lanes that are `on` go to the rows of their slots, one set of atomics per distinct slot of the wave
__device__ __forceinline__ void add_to_rows(bool on, int s, const TetTerms& t, int64_t* table) {
  wave_for_each_key(on, s, [&](int key, u64, bool mine) {
    const int tris = wave_sum(mine ? t.tris : 0);
    const u64 c0 = wave_sum(mine ? t.cls[0] : u64{0}), c1 = wave_sum(mine ? t.cls[1] : u64{0});  // <= 64 * 12 a field
    const int64_t v6 = wave_sum(mine ? t.v6 : int64_t{0});
    if ((threadIdx.x & (kWave - 1)) == 0) {
      u64* row = reinterpret_cast<u64*>(table + kHead + int64_t{key} * kRow);
      atomicAdd(row + fTris, static_cast<u64>(tris));
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const u64 n = ((k < 4 ? c0 : c1) >> (16 * (k & 3))) & 0xffffu;
        if (n) atomicAdd(row + fClass + k, n);
      }
      atomicAdd(row + fV6, static_cast<u64>(v6));
    }
  });
}

__device__ __forceinline__ void fold(const TetTerms& t, TetTerms* all, bool* uniform) {
  if (t.root == 0) return;
  if (all->root != 0 && all->root != t.root) *uniform = false;
  if (all->root == 0 || t.root < all->root) all->root = t.root;
  all->tris += t.tris, all->cls[0] += t.cls[0], all->cls[1] += t.cls[1], all->v6 += t.v6;
}

__global__ __launch_bounds__(kBlock) void mesh_classify_kernel(const int* __restrict__ roots,
                                                               const int* __restrict__ slot, int64_t* table,
                                                               uint8_t* __restrict__ cmask,
                                                               int64_t* __restrict__ chunk_v,
                                                               int64_t* __restrict__ chunk_t, Cells g, int64_t cap) {
  __shared__ int wave_counts[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t chunks = (g.cells + kBlock - 1) / kBlock;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t c = chunk * kBlock + threadIdx.x;
    const bool valid = c < g.cells;
    const auto [cx, cy, cz] = split_xyz(static_cast<int>(valid ? c : 0), g.CY, g.CZ);
    const int mx = cx - 1, my = cy - 1, mz = cz - 1;
    int r[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // the upper z face: corner 2 k + 1 is voxel (mx + dx, my + dy, cz)
      const int hi = valid ? root_at(roots, g, mx + (k >> 1), my + (k & 1), cz) : 0;
      int lo = __shfl_up(hi, 1, kWave);  // the lane before holds cell c - 1: the same row at cz - 1 when cz > 0
      if (cz == 0) lo = 0;
      else if (lane == 0) lo = valid ? root_at(roots, g, mx + (k >> 1), my + (k & 1), mz) : 0;
      r[2 * k + 1] = hi, r[2 * k] = lo;
    }
    unsigned m = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) m |= (r[d] != 0 ? 1u : 0u) << d;
    if (!valid) m = 0;
    if (valid) cmask[c] = static_cast<uint8_t>(m);
    const int verts = __popc(edge_mask(m)), tris = kMask.tris[m];
    const int both = wave_sum(verts | (tris << 16));  // at most 256 * 7 and 256 * 12: both fit 16 bits
    __syncthreads();                                  // the last chunk's totals have been read
    if (lane == 0) wave_counts[threadIdx.x / kWave] = both;
    __syncthreads();
    if (threadIdx.x == 0) {
      int all = 0;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) all += wave_counts[w];
      chunk_v[chunk] = all & 0xffff, chunk_t[chunk] = all >> 16;
    }
    if (__ballot(tris != 0) == 0) continue;  // uniform over the wave; no barrier below
    TetTerms all = {0, 0, {0, 0}, 0};
    bool uniform = true;
    if (tris != 0) {
      fold(tet_terms<0>(m, r, mx, my, mz), &all, &uniform);
      fold(tet_terms<1>(m, r, mx, my, mz), &all, &uniform);
      fold(tet_terms<2>(m, r, mx, my, mz), &all, &uniform);
      fold(tet_terms<3>(m, r, mx, my, mz), &all, &uniform);
      fold(tet_terms<4>(m, r, mx, my, mz), &all, &uniform);
      fold(tet_terms<5>(m, r, mx, my, mz), &all, &uniform);
    }
    {  // the cells whose triangles are one lesion's: always at connectivity 26
      const bool on = tris != 0 && uniform && all.root >= 1 && all.root <= g.voxels;
      const int s = on ? slot[all.root - 1] : 0;
      add_to_rows(on && s < cap, s, all, table);
    }
    const bool split = tris != 0 && !uniform;  // connectivity 6: two lesions meet in the cell, tetrahedron by tetrahedron
    if (__ballot(split) == 0) continue;
    auto one = [&](const TetTerms& t) {
      const bool on = split && t.root >= 1 && t.root <= g.voxels;
      const int s = on ? slot[t.root - 1] : 0;
      add_to_rows(on && s < cap, s, t, table);
    };
    one(tet_terms<0>(m, r, mx, my, mz));
    one(tet_terms<1>(m, r, mx, my, mz));
    one(tet_terms<2>(m, r, mx, my, mz));
    one(tet_terms<3>(m, r, mx, my, mz));
    one(tet_terms<4>(m, r, mx, my, mz));
    one(tet_terms<5>(m, r, mx, my, mz));
  }
}

// ------------------------------------------------------------------ T2
// one workgroup per array (blockIdx.x picks it): the totals of the chunks become exclusive bases in place and the
// grand total goes to *total.  A thread takes kScanRun consecutive entries, so 35 000 chunks (a BraTS-size volume) are
// nine trips of the workgroup, not 137.
constexpr int kScanRun = 16;
struct ScanJobs {
  int64_t* chunk[2];
  int64_t* total[2];
};

__global__ __launch_bounds__(kBlock) void mesh_scan_chunks_kernel(ScanJobs jobs, int64_t chunks) {
  int64_t* chunk = blockIdx.x == 0 ? jobs.chunk[0] : jobs.chunk[1];
  int64_t* total = blockIdx.x == 0 ? jobs.total[0] : jobs.total[1];
  int64_t carry = 0;
  for (int64_t base = 0; base < chunks; base += int64_t{kBlock} * kScanRun) {
    const int64_t first = base + int64_t{threadIdx.x} * kScanRun;
    int64_t v[kScanRun], mine = 0;
#pragma unroll
    for (int k = 0; k < kScanRun; ++k) {
      v[k] = first + k < chunks ? chunk[first + k] : 0;
      mine += v[k];
    }
    int64_t sum;
    int64_t at = carry + block_scan_exclusive(mine, &sum);
#pragma unroll
    for (int k = 0; k < kScanRun; ++k) {
      if (first + k < chunks) chunk[first + k] = at;
      at += v[k];
    }
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

// ------------------------------------------------------------------ T3
__global__ __launch_bounds__(kBlock) void mesh_vertices_kernel(const uint8_t* __restrict__ cmask,
                                                               const int64_t* __restrict__ chunk_v,
                                                               int* __restrict__ vbase, int* __restrict__ vertices,
                                                               int64_t n_vertices, Cells g) {
  const int64_t chunks = (g.cells + kBlock - 1) / kBlock;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t c = chunk * kBlock + threadIdx.x;
    const bool valid = c < g.cells;
    const unsigned e = valid ? edge_mask(cmask[c]) : 0u;
    int64_t total;
    int64_t at = chunk_v[chunk] + block_scan_exclusive(__popc(e), &total);
    if (!valid) continue;  // after the barriers
    vbase[c] = static_cast<int>(at);
    if (e == 0) continue;
    const auto [cx, cy, cz] = split_xyz(static_cast<int>(c), g.CY, g.CZ);
#pragma unroll
    for (int d = 1; d < 8; ++d) {
      if (!((e >> (d - 1)) & 1u)) continue;
      if (at >= 0 && at < n_vertices) {  // the lower end is the minimum corner: 2 m + the direction
        vertices[3 * at] = 2 * (cx - 1) + ((d >> 2) & 1);
        vertices[3 * at + 1] = 2 * (cy - 1) + ((d >> 1) & 1);
        vertices[3 * at + 2] = 2 * (cz - 1) + (d & 1);
      }
      ++at;
    }
  }
}

__global__ __launch_bounds__(kBlock) void mesh_faces_kernel(const int* __restrict__ roots,
                                                            const int* __restrict__ slot,
                                                            const uint8_t* __restrict__ cmask,
                                                            const int64_t* __restrict__ chunk_t,
                                                            const int* __restrict__ vbase, int* __restrict__ faces,
                                                            int* __restrict__ face_slot, int64_t n_vertices,
                                                            int64_t n_faces, Cells g) {
  const int64_t chunks = (g.cells + kBlock - 1) / kBlock;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t c = chunk * kBlock + threadIdx.x;
    const bool valid = c < g.cells;
    const unsigned m = valid ? cmask[c] : 0u;
    int64_t total;
    int64_t at = chunk_t[chunk] + block_scan_exclusive(kMask.tris[m], &total);
    if (!valid || kMask.tris[m] == 0) continue;  // after the barriers
    const auto [cx, cy, cz] = split_xyz(static_cast<int>(c), g.CY, g.CZ);
    for (int t = 0; t < 6; ++t) {
      const TetCase& tc = kTet.c[t][tet_case(t, m)];
      if (tc.tris == 0) continue;
      int root = INT32_MAX;
      for (int k = 0; k < 4; ++k) {  // surface cells only: their corners' roots straight from memory
        const int corner = tc.path[k];
        if (!((m >> corner) & 1u)) continue;
        const int v = root_at(roots, g, cx - 1 + ((corner >> 2) & 1), cy - 1 + ((corner >> 1) & 1), cz - 1 + (corner & 1));
        if (v != 0 && v < root) root = v;
      }
      const int s = root != INT32_MAX && root >= 1 && root <= g.voxels ? slot[root - 1] : -1;
      for (int j = 0; j < tc.tris; ++j, ++at) {
        if (at < 0 || at >= n_faces) continue;
        for (int i = 0; i < 3; ++i) {
          const int lo = tc.edge[j][i] & 7, d = (tc.edge[j][i] >> 3) ^ lo;
          // the owner: the cell whose minimum corner is the lower end (inside the grid: an end past the volume is outside)
          const int64_t o = c + (int64_t{(lo >> 2) & 1} * g.CY + ((lo >> 1) & 1)) * g.CZ + (lo & 1);
          int64_t v = 0;
          if (o < g.cells && d >= 1) v = int64_t{vbase[o]} + __popc(edge_mask(cmask[o]) & ((1u << (d - 1)) - 1u));
          faces[3 * at + i] = static_cast<int>(v >= 0 && v < n_vertices ? v : 0);
        }
        face_slot[at] = s;
      }
    }
  }
}

// face_slot[f] = rank[face_slot[f]]: the table's arrival order to the caller's lesion order
__global__ __launch_bounds__(kBlock) void mesh_relabel_kernel(int* __restrict__ face_slot, int64_t n_faces,
                                                              const int* __restrict__ rank, int64_t n_rank) {
  for (int64_t f = int64_t{blockIdx.x} * kBlock + threadIdx.x; f < n_faces; f += int64_t{gridDim.x} * kBlock) {
    const int s = face_slot[f];
    face_slot[f] = s >= 0 && s < n_rank ? rank[s] : -1;
  }
}

// ------------------------------------------------------------------ T4
__global__ __launch_bounds__(kBlock) void mesh_degree_kernel(const int* __restrict__ faces, int64_t n_faces,
                                                             int64_t n_vertices, int* degree) {
  for (int64_t e = int64_t{blockIdx.x} * kBlock + threadIdx.x; e < 3 * n_faces; e += int64_t{gridDim.x} * kBlock) {
    const int a = faces[e];
    if (a >= 0 && a < n_vertices) atomicAdd(&degree[a], 1);
  }
}

__global__ __launch_bounds__(kBlock) void mesh_chunk_sums_kernel(const int* __restrict__ v, int64_t n,
                                                                 int64_t* __restrict__ chunk) {
  const int64_t chunks = (n + kBlock - 1) / kBlock;
  for (int64_t k = blockIdx.x; k < chunks; k += gridDim.x) {
    const int64_t i = k * kBlock + threadIdx.x;
    int64_t total;
    block_scan_exclusive(i < n ? v[i] : 0, &total);
    if (threadIdx.x == 0) chunk[k] = total;
  }
}

// cursor holds the degrees: row_start[i] = cursor[i] = their exclusive prefix; row_start[n] = the total
__global__ __launch_bounds__(kBlock) void mesh_row_starts_kernel(int* cursor, int64_t n,
                                                                 const int64_t* __restrict__ chunk,
                                                                 const int64_t* __restrict__ total,
                                                                 int* __restrict__ row_start) {
  const int64_t chunks = (n + kBlock - 1) / kBlock;
  for (int64_t k = blockIdx.x; k < chunks; k += gridDim.x) {
    const int64_t i = k * kBlock + threadIdx.x;
    int64_t sum;
    const int64_t e = chunk[k] + block_scan_exclusive(i < n ? cursor[i] : 0, &sum);
    if (i < n) row_start[i] = cursor[i] = static_cast<int>(e);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) row_start[n] = static_cast<int>(*total);
}

__global__ __launch_bounds__(kBlock) void mesh_fill_kernel(const int* __restrict__ faces, int64_t n_faces,
                                                           int64_t n_vertices, int* cursor, int* __restrict__ nbr) {
  for (int64_t e = int64_t{blockIdx.x} * kBlock + threadIdx.x; e < 3 * n_faces; e += int64_t{gridDim.x} * kBlock) {
    const int64_t f = e / 3;
    const int i = static_cast<int>(e - 3 * f);
    const int a = faces[e], b = faces[3 * f + (i == 2 ? 0 : i + 1)];
    if (a < 0 || a >= n_vertices) continue;
    const int at = atomicAdd(&cursor[a], 1);
    if (at >= 0 && at < 3 * n_faces) nbr[at] = b;
  }
}

// one thread per row: insertion sort, ascending (a row is at most 12 long on a mesh of T3)
__global__ __launch_bounds__(kBlock) void mesh_sort_rows_kernel(const int* __restrict__ row_start, int64_t n_vertices,
                                                                int64_t n_edges, int* __restrict__ nbr) {
  for (int64_t v = int64_t{blockIdx.x} * kBlock + threadIdx.x; v < n_vertices; v += int64_t{gridDim.x} * kBlock) {
    const int64_t begin = row_start[v], end = row_start[v + 1];
    if (begin < 0 || end > n_edges || begin > end) continue;
    for (int64_t i = begin + 1; i < end; ++i) {
      const int key = nbr[i];
      int64_t j = i;
      for (; j > begin && nbr[j - 1] > key; --j) nbr[j] = nbr[j - 1];
      nbr[j] = key;
    }
  }
}

// ------------------------------------------------------------------ T5
__global__ __launch_bounds__(kBlock) void mesh_positions_kernel(const int* __restrict__ half, int64_t n_vertices,
                                                                int64_t ux, int64_t uy, int64_t uz, double scale_mm,
                                                                double* __restrict__ pos) {
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < 3 * n_vertices; i += int64_t{gridDim.x} * kBlock) {
    const int a = static_cast<int>(i % 3);
    const int64_t u = a == 0 ? ux : a == 1 ? uy : uz;
    pos[i] = static_cast<double>(int64_t{half[i]} * u) * scale_mm / 2.0;
  }
}

__global__ __launch_bounds__(kBlock) void mesh_smooth_kernel(const int* __restrict__ row_start,
                                                             const int* __restrict__ nbr, int64_t n_vertices,
                                                             int64_t n_edges, const double* __restrict__ src,
                                                             double* __restrict__ dst, double factor) {
  for (int64_t v = int64_t{blockIdx.x} * kBlock + threadIdx.x; v < n_vertices; v += int64_t{gridDim.x} * kBlock) {
    const int64_t begin = row_start[v], end = row_start[v + 1];
    const double px = src[3 * v], py = src[3 * v + 1], pz = src[3 * v + 2];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int n = 0;
    if (begin >= 0 && end <= n_edges) {
      for (int64_t e = begin; e < end; ++e) {
        const int b = nbr[e];
        if (b < 0 || b >= n_vertices) continue;
        if (n == 0) sx = src[3 * int64_t{b}], sy = src[3 * int64_t{b} + 1], sz = src[3 * int64_t{b} + 2];
        else sx = sx + src[3 * int64_t{b}], sy = sy + src[3 * int64_t{b} + 1], sz = sz + src[3 * int64_t{b} + 2];
        ++n;
      }
    }
    if (n == 0) {
      dst[3 * v] = px, dst[3 * v + 1] = py, dst[3 * v + 2] = pz;
      continue;
    }
    const double k = static_cast<double>(n);
    dst[3 * v] = px + factor * (sx / k - px);
    dst[3 * v + 1] = py + factor * (sy / k - py);
    dst[3 * v + 2] = pz + factor * (sz / k - pz);
  }
}

__global__ __launch_bounds__(kBlock) void mesh_terms_kernel(const double* __restrict__ pos,
                                                            const int* __restrict__ faces, int64_t n_vertices,
                                                            int64_t n_faces, double* __restrict__ area,
                                                            double* __restrict__ volume) {
  for (int64_t f = int64_t{blockIdx.x} * kBlock + threadIdx.x; f < n_faces; f += int64_t{gridDim.x} * kBlock) {
    double p[3][3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int64_t v = faces[3 * f + i];
      ok = ok && v >= 0 && v < n_vertices;
#pragma unroll
      for (int a = 0; a < 3; ++a) p[i][a] = ok ? pos[3 * v + a] : 0.0;
    }
    const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    area[f] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    const double dx = p[1][1] * p[2][2] - p[1][2] * p[2][1], dy = p[1][2] * p[2][0] - p[1][0] * p[2][2],
                 dz = p[1][0] * p[2][1] - p[1][1] * p[2][0];
    volume[f] = ((p[0][0] * dx + p[0][1] * dy) + p[0][2] * dz) / 6.0;
  }
}

// ------------------------------------------------------------------ host
inline bool mesh_cells(int64_t X, int64_t Y, int64_t Z, int64_t* voxels, int64_t* cells) {
  if (!volume_voxels(X, Y, Z, false, voxels) || X > kMmMaxExtent || Y > kMmMaxExtent || Z > kMmMaxExtent) return false;
  return volume_voxels(X + 1, Y + 1, Z + 1, false, cells);
}

inline int64_t chunks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

// corner masks uint8[cells] | vertex bases int32[cells] | slots int32[voxels] | chunk bases int64[2][chunks]
struct MeshBuffers {
  uint8_t* cmask;
  int *vbase, *slot;
  int64_t *chunk_v, *chunk_t;
};

inline int64_t mesh_bytes(int64_t voxels, int64_t cells) {
  return round256(cells) + round256(4 * cells) + round256(4 * voxels) + 2 * round256(8 * chunks_of(cells));
}

inline MeshBuffers mesh_buffers(void* workspace, int64_t voxels, int64_t cells) {
  char* ws = static_cast<char*>(workspace);
  MeshBuffers b;
  b.cmask = reinterpret_cast<uint8_t*>(ws), ws += round256(cells);
  b.vbase = reinterpret_cast<int*>(ws), ws += round256(4 * cells);
  b.slot = reinterpret_cast<int*>(ws), ws += round256(4 * voxels);
  b.chunk_v = reinterpret_cast<int64_t*>(ws), ws += round256(8 * chunks_of(cells));
  b.chunk_t = reinterpret_cast<int64_t*>(ws);
  return b;
}

// cursors int32[V] | chunk bases int64[chunks of V] | the total int64
inline int64_t adjacency_bytes(int64_t V) { return round256(4 * V) + round256(8 * chunks_of(V)) + 256; }

inline bool counts_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V <= INT32_MAX && F <= INT32_MAX / 3; }

}  // namespace
}  // namespace gts

extern "C" int64_t gts_mesh_workspace(int64_t X, int64_t Y, int64_t Z) {
  int64_t voxels, cells;
  return gts::mesh_cells(X, Y, Z, &voxels, &cells) ? gts::mesh_bytes(voxels, cells) : 0;
}

extern "C" int64_t gts_mesh_table_i64s(int64_t X, int64_t Y, int64_t Z, int32_t connectivity) {
  int64_t voxels, cells;
  if (!gts::mesh_cells(X, Y, Z, &voxels, &cells) || (connectivity != 6 && connectivity != 26)) return 0;
  return gts::kHead + gts::kRow * gts::lesion_rows(X, Y, Z, connectivity);
}

extern "C" int64_t gts_mesh_adjacency_workspace(int64_t n_vertices) {
  return n_vertices >= 0 && n_vertices <= INT32_MAX ? gts::adjacency_bytes(n_vertices) : 0;
}

extern "C" int32_t gts_mesh_classify(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, int32_t connectivity,
                                     int64_t* table, int64_t table_i64s, void* workspace, int64_t workspace_bytes,
                                     int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !table || !workspace) return GTS_ERR_NULL;
  int64_t voxels, cells;
  if (!mesh_cells(X, Y, Z, &voxels, &cells) || !grid_ok(grid_blocks) || workspace_bytes < mesh_bytes(voxels, cells))
    return GTS_ERR_SHAPE;
  if (connectivity != 6 && connectivity != 26) return GTS_ERR_ARGKIND;
  const int64_t cap = lesion_rows(X, Y, Z, connectivity);
  if (table_i64s < kHead + kRow * cap) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const MeshBuffers b = mesh_buffers(workspace, voxels, cells);
  const Cells g = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), static_cast<int>(Y + 1),
                   static_cast<int>(Z + 1), cells, voxels};
  if (hipMemsetAsync(table, 0, 8 * kHead, st) != hipSuccess) return launch_status();
  lesion_rows_kernel<kHead, kRow><<<grid_for(voxels, kBlock, grid_blocks), kBlock, 0, st>>>(roots, b.slot, table,
                                                                                            voxels, cap);
  mesh_classify_kernel<<<grid_for(cells, kBlock, grid_blocks), kBlock, 0, st>>>(roots, b.slot, table, b.cmask,
                                                                                 b.chunk_v, b.chunk_t, g, cap);
  const ScanJobs jobs = {{b.chunk_v, b.chunk_t}, {table + hVertices, table + hTriangles}};
  mesh_scan_chunks_kernel<<<2, kBlock, 0, st>>>(jobs, chunks_of(cells));
  return launch_status();
}

extern "C" int32_t gts_mesh_emit(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, void* workspace,
                                 int64_t workspace_bytes, int32_t* vertices, int64_t n_vertices, int32_t* faces,
                                 int32_t* face_slot, int64_t n_faces, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !workspace || (n_vertices > 0 && !vertices) || (n_faces > 0 && (!faces || !face_slot)))
    return GTS_ERR_NULL;
  int64_t voxels, cells;
  if (!mesh_cells(X, Y, Z, &voxels, &cells) || !grid_ok(grid_blocks) || workspace_bytes < mesh_bytes(voxels, cells) ||
      !counts_ok(n_vertices, n_faces))
    return GTS_ERR_SHAPE;
  if (n_vertices == 0 || n_faces == 0) return GTS_OK;  // an empty region: nothing to write, nothing launched
  hipStream_t st = static_cast<hipStream_t>(stream);
  const MeshBuffers b = mesh_buffers(workspace, voxels, cells);
  const Cells g = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), static_cast<int>(Y + 1),
                   static_cast<int>(Z + 1), cells, voxels};
  const int grid = grid_for(cells, kBlock, grid_blocks);
  mesh_vertices_kernel<<<grid, kBlock, 0, st>>>(b.cmask, b.chunk_v, b.vbase, vertices, n_vertices, g);
  mesh_faces_kernel<<<grid, kBlock, 0, st>>>(roots, b.slot, b.cmask, b.chunk_t, b.vbase, faces, face_slot, n_vertices,
                                             n_faces, g);
  return launch_status();
}

extern "C" int32_t gts_mesh_relabel(int32_t* face_slot, int64_t n_faces, const int32_t* rank, int64_t n_rank,
                                    int64_t grid_blocks, void* stream) {
  using namespace gts;
  if ((n_faces > 0 && !face_slot) || (n_rank > 0 && !rank)) return GTS_ERR_NULL;
  if (!grid_ok(grid_blocks) || !counts_ok(n_rank, n_faces)) return GTS_ERR_SHAPE;
  if (n_faces == 0) return GTS_OK;
  mesh_relabel_kernel<<<grid_for(n_faces, kBlock, grid_blocks), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      face_slot, n_faces, rank, n_rank);
  return launch_status();
}

extern "C" int32_t gts_mesh_adjacency(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* row_start,
                                      int32_t* neighbours, void* workspace, int64_t workspace_bytes,
                                      int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!row_start || !workspace || (n_faces > 0 && (!faces || !neighbours))) return GTS_ERR_NULL;
  if (!grid_ok(grid_blocks) || !counts_ok(n_vertices, n_faces) || workspace_bytes < adjacency_bytes(n_vertices))
    return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  int* cursor = reinterpret_cast<int*>(ws);
  int64_t* chunk = reinterpret_cast<int64_t*>(ws + round256(4 * n_vertices));
  int64_t* total = reinterpret_cast<int64_t*>(ws + round256(4 * n_vertices) + round256(8 * chunks_of(n_vertices)));
  if (hipMemsetAsync(row_start, 0, 4 * (n_vertices + 1), st) != hipSuccess) return launch_status();
  if (n_vertices == 0 || n_faces == 0) return launch_status();
  const int grid_e = grid_for(3 * n_faces, kBlock, grid_blocks), grid_v = grid_for(n_vertices, kBlock, grid_blocks);
  int* degree = cursor;  // the degrees are counted where the cursors will stand; the starts are written from them
  if (hipMemsetAsync(degree, 0, 4 * n_vertices, st) != hipSuccess) return launch_status();
  mesh_degree_kernel<<<grid_e, kBlock, 0, st>>>(faces, n_faces, n_vertices, degree);
  mesh_chunk_sums_kernel<<<grid_v, kBlock, 0, st>>>(degree, n_vertices, chunk);
  const ScanJobs jobs = {{chunk, chunk}, {total, total}};
  mesh_scan_chunks_kernel<<<1, kBlock, 0, st>>>(jobs, chunks_of(n_vertices));
  mesh_row_starts_kernel<<<grid_v, kBlock, 0, st>>>(cursor, n_vertices, chunk, total, row_start);
  mesh_fill_kernel<<<grid_e, kBlock, 0, st>>>(faces, n_faces, n_vertices, cursor, neighbours);
  mesh_sort_rows_kernel<<<grid_v, kBlock, 0, st>>>(row_start, n_vertices, 3 * n_faces, neighbours);
  return launch_status();
}

extern "C" int32_t gts_mesh_positions(const int32_t* vertices, int64_t n_vertices, const int64_t* units,
                                      double scale_mm, double* positions, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!units || (n_vertices > 0 && (!vertices || !positions))) return GTS_ERR_NULL;
  if (!grid_ok(grid_blocks) || !counts_ok(n_vertices, 0)) return GTS_ERR_SHAPE;
  if (!units_ok(units) || !(scale_mm > 0.0) || !(scale_mm <= 1.0e6)) return GTS_ERR_ARGKIND;
  if (n_vertices == 0) return GTS_OK;
  mesh_positions_kernel<<<grid_for(3 * n_vertices, kBlock, grid_blocks), kBlock, 0,
                          static_cast<hipStream_t>(stream)>>>(vertices, n_vertices, units[0], units[1], units[2],
                                                              scale_mm, positions);
  return launch_status();
}

extern "C" int32_t gts_mesh_smooth(const int32_t* row_start, const int32_t* neighbours, int64_t n_vertices,
                                   int64_t n_faces, double* positions, double* scratch, double lambda, double mu,
                                   int64_t iterations, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!row_start || (n_vertices > 0 && (!positions || !scratch)) || (n_faces > 0 && !neighbours)) return GTS_ERR_NULL;
  if (!grid_ok(grid_blocks) || !counts_ok(n_vertices, n_faces) || iterations < 0 || iterations > 100000)
    return GTS_ERR_SHAPE;
  if (!(lambda == lambda) || !(mu == mu) || lambda - lambda != 0.0 || mu - mu != 0.0) return GTS_ERR_ARGKIND;
  if (n_vertices == 0) return GTS_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = grid_for(n_vertices, kBlock, grid_blocks);
  for (int64_t it = 0; it < iterations; ++it) {
    mesh_smooth_kernel<<<grid, kBlock, 0, st>>>(row_start, neighbours, n_vertices, 3 * n_faces, positions, scratch,
                                                lambda);
    mesh_smooth_kernel<<<grid, kBlock, 0, st>>>(row_start, neighbours, n_vertices, 3 * n_faces, scratch, positions, mu);
  }
  return launch_status();
}

extern "C" int32_t gts_mesh_terms(const double* positions, const int32_t* faces, int64_t n_vertices, int64_t n_faces,
                                  double* area, double* volume, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (n_faces > 0 && (!positions || !faces || !area || !volume)) return GTS_ERR_NULL;
  if (!grid_ok(grid_blocks) || !counts_ok(n_vertices, n_faces)) return GTS_ERR_SHAPE;
  if (n_faces == 0) return GTS_OK;
  mesh_terms_kernel<<<grid_for(n_faces, kBlock, grid_blocks), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      positions, faces, n_vertices, n_faces, area, volume);
  return launch_status();
}
