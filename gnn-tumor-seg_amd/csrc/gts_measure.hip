// M1-M4: the device half of the per-lesion measurements (gts/measure.py).  What a user otherwise does
// on the host with scipy's label, one mask per lesion and a brute-force pairwise distance in numpy.  The region mask
// comes from L1 (dilation 0) and its components from C1-C3, both unchanged.
//
// Definitions.  An int16 label volume [X][Y][Z] (Z contiguous), a region (0 WT, 1 CT, 2 ET) and units (u_x, u_y, u_z),
// the voxel spacing as positive integers (gts.metrics.spacing_units).  A lesion L is a connected component of the
// region mask; points are voxel centres; every quantity is an exact int64.
//   counts   n, n_class[1..3] (voxels of L per label), the box, S_a = the sum of coordinate a over L.
//   faces    F_a = the number of (voxel of L, direction +a or -a) whose neighbour across that face is outside the
//            region mask or outside the volume (an axis of extent 1 exposes both faces).  The face-count area
//            F_x u_y u_z + F_y u_x u_z + F_z u_x u_y overestimates a smooth surface (a staircase, not a tangent plane).
//   D3       max over pairs of voxels of L of sum_a u_a^2 d_a^2; 0 for a single voxel.
//   in-plane on every plane of constant z in which L has a footprint (its whole cross-section, connected or not):
//            D2_z = max over footprint pairs of u_x^2 dx^2 + u_y^2 dy^2, and W_z = max over the pairs (a, b) that
//            reach D2_z of the caliper width max_r p.P_r - min_r p.P_r over the footprint, p = (-d_y, d_x), d = P_b -
//            P_a in integer physical units; W_z = 0 when D2_z = 0.  W_z is exactly (major diameter) x (width
//            perpendicular to it) in units^2.  Ties take the maximum width, which mirroring the volume leaves alone.
//            The lesion reports (z*, D2_z*, W_z*), z* the smallest z with maximal W_z.  Distances are centre to
//            centre, so a one-pixel footprint measures 0.
//
//   M1  table pass.  Every root voxel takes a row (gts_lesions.h: lesion_rows_kernel, at most lesion_rows of them);
//       one pass over labels and roots then adds every voxel's counts, box, coordinate sums, face counts and whether
//       it is a 3-D candidate to its lesion's row, the lanes of one lesion summed in the wave first.  A single
//       workgroup then scans the rows: the first slice row of every lesion (one row per z of its box) and the start
//       of its candidate list.
//   M2  candidate lists.  A diameter endpoint and a caliper extreme are vertices of the convex hull, and a hull
//       vertex cannot have lesion voxels on both sides along an axis (it would be their midpoint).  So the 3-D
//       candidates are the voxels that lack one of their two neighbours along x, along y and along z, the in-plane
//       candidates of a slice those that do along x and along y; a face neighbour in the mask is in the lesion at
//       either connectivity.  Count per slice row, exclusive scan, fill through atomic cursors: the order inside a
//       list is arrival order and no result depends on it.
//   M3  pairwise 3-D diameter.  Work units (lesion row, tile i, tile j >= i) of the candidate list; both tiles in LDS
//       as int32 triples already multiplied by the units; per-thread running max, wave reduce, one 64-bit atomic max
//       per workgroup and unit.
//   M4  in-plane.  Work units (lesion row, slice).  Pass A: max D2 over candidate pairs.  Pass B: every pair that
//       reaches it takes the projection range over the slice's candidates.  A planar set of n points has at most n
//       diameter pairs, so B costs no more than A.  One thread per lesion then resolves (z*, D2, W) from its slice
//       rows in ascending z.
//
// Integer arithmetic, integer atomics (add, max) and plain vector stores only: identical results on every run and at
// every grid_blocks.  Limits: every extent in [1, 4097], X * Y * Z < 2^31, units in [1, 10^6], and with
// B = sum_a u_a^2 (N_a - 1)^2, 2 B < 2^62: u_a (N_a - 1) then fits an int32, every squared distance is at most B and
// |p.P_r| <= 2 u_x (N_x - 1) u_y (N_y - 1) <= B, so a projection range is at most 2 B.
#include "gts_lesions.h"

namespace gts {
namespace {

constexpr int kRow = GTS_MEASURE_ROW_I64;
constexpr int kHead = GTS_MEASURE_HEAD_I64;
constexpr int kPairTile = GTS_MEASURE_PAIR_TILE;
constexpr int kPlaneTile = GTS_MEASURE_PLANE_TILE;
typedef unsigned long long u64;

static_assert(kPairTile == kBlock && kPlaneTile == kBlock, "one thread stages one point of a tile");

// row fields
enum { fRoot = 0, fN = 1, fClass = 2, fBox = 5, fSum = 11, fFace = 14, fCand = 17, fCandEnd = 18, fSlice = 19,
       fD3 = 20, fPlaneZ = 21, fPlaneD2 = 22, fPlaneW = 23 };
// header fields
enum { hLesions = 0, hSlices = 1, hCand3 = 2, hCand2 = 3 };
static_assert(hLesions == 0 && fRoot == 0, "the table convention of lesion_rows_kernel");

struct Vol {
  int X, Y, Z;
  int64_t n;
};

// which of the six face neighbours of voxel i = (x, y, z) are in the mask: bit 2a for -a, bit 2a + 1 for +a
__device__ __forceinline__ unsigned face_neighbours(const int* __restrict__ roots, int64_t i, int x, int y, int z,
                                                    const Vol& v) {
  const int64_t yz = int64_t{v.Y} * v.Z;
  unsigned m = 0;
  if (x > 0 && roots[i - yz] != 0) m |= 1u;
  if (x + 1 < v.X && roots[i + yz] != 0) m |= 2u;
  if (y > 0 && roots[i - v.Z] != 0) m |= 4u;
  if (y + 1 < v.Y && roots[i + v.Z] != 0) m |= 8u;
  if (z > 0 && roots[i - 1] != 0) m |= 16u;
  if (z + 1 < v.Z && roots[i + 1] != 0) m |= 32u;
  return m;
}

// lacks one of its two neighbours along every axis below `axes` (3: x, y, z; 2: x, y)
__device__ __forceinline__ bool is_candidate(unsigned m, int axes) {
  bool c = true;
  for (int a = 0; a < axes; ++a) c = c && ((m >> (2 * a)) & 3u) != 3u;
  return c;
}

// the maximum of v over the workgroup, in every thread; every thread calls it
__device__ __forceinline__ int64_t block_max(int64_t v) {
  __shared__ int64_t wave_top[kWavesPerBlock];
  v = wave_reduce(v, [](int64_t a, int64_t b) { return a > b ? a : b; });
  if ((threadIdx.x & (kWave - 1)) == 0) wave_top[threadIdx.x / kWave] = v;
  __syncthreads();
  int64_t top = wave_top[0];
#pragma unroll
  for (int k = 1; k < kWavesPerBlock; ++k) top = wave_top[k] > top ? wave_top[k] : top;
  __syncthreads();
  return top;
}

// ------------------------------------------------------------------ M1
__global__ __launch_bounds__(kBlock) void measure_tables_kernel(const int16_t* __restrict__ labels,
                                                                const int* __restrict__ roots,
                                                                const int* __restrict__ slot, int64_t* table, Vol v,
                                                                int region, int64_t cap) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t base = int64_t{blockIdx.x} * kBlock; base < v.n; base += int64_t{gridDim.x} * kBlock) {
    const int64_t i = base + threadIdx.x;  // the trip count is the workgroup's: every lane reaches the wave loop
    const bool inside = i < v.n;
    const auto [x, y, z] = split_xyz(static_cast<int>(inside ? i : 0), v.Y, v.Z);
    const int r = inside ? roots[i] : 0;
    const int label = inside ? labels[i] : 0;
    bool g = r != 0 && in_region(label, region);
    const int s = g ? slot[r - 1] : 0;
    g = g && s < cap;
    const unsigned m = g ? face_neighbours(roots, i, x, y, z, v) : 0u;
    const bool cand = g && is_candidate(m, 3);
    const int vals[12] = {x + 1, v.X - x, y + 1, v.Y - y, z + 1, v.Z - z, x, y, z,
                          2 - static_cast<int>(__popc(m & 3u)), 2 - static_cast<int>(__popc(m & 12u)),
                          2 - static_cast<int>(__popc(m & 48u))};
    wave_for_each_key(g, s, [&](int key, u64 same, bool mine) {
      const int count = __popcll(same);
      int cls[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) cls[c] = __popcll(__ballot(mine && label == c + 1));
      const int cands = __popcll(__ballot(mine && cand));
      int red[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const int mv = mine ? vals[k] : 0;
        red[k] = k < 6 ? wave_reduce(mv, [](int a, int b) { return a > b ? a : b; }) : wave_sum(mv);
      }
      if (lane == 0) {
        u64* row = reinterpret_cast<u64*>(table + kHead + int64_t{key} * kRow);
        atomicAdd(row + fN, static_cast<u64>(count));
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (cls[c]) atomicAdd(row + fClass + c, static_cast<u64>(cls[c]));
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicMax(row + fBox + k, static_cast<u64>(red[k]));
#pragma unroll
        for (int k = 6; k < 12; ++k)
          if (red[k]) atomicAdd(row + fSum + (k - 6), static_cast<u64>(red[k]));
        if (cands) atomicAdd(row + fCand, static_cast<u64>(cands));
      }
    });
  }
}

// one workgroup: per row the first slice row (exclusive sum of the boxes' z extents) and the start of the 3-D
// candidate list (exclusive sum of the candidate counts); the totals go to the header
__global__ __launch_bounds__(kBlock) void measure_scan_rows_kernel(int64_t* table, int Z, int64_t cap) {
  const int64_t rows = table[hLesions] < cap ? table[hLesions] : cap;
  int64_t slices = 0, cands = 0;
  for (int64_t base = 0; base < rows; base += kBlock) {
    const int64_t s = base + threadIdx.x;
    int64_t* row = table + kHead + s * kRow;
    const int64_t zext = s < rows ? row[fBox + 4] + row[fBox + 5] - Z : 0;
    const int64_t c = s < rows ? row[fCand] : 0;
    int64_t t0, t1;
    const int64_t e0 = block_scan_exclusive(zext, &t0), e1 = block_scan_exclusive(c, &t1);
    if (s < rows) {
      row[fSlice] = slices + e0;
      row[fCandEnd] = cands + e1;
    }
    slices += t0;
    cands += t1;
  }
  if (threadIdx.x == 0) {
    table[hSlices] = slices;
    table[hCand3] = cands;
  }
}

// ------------------------------------------------------------------ M2
__global__ __launch_bounds__(kBlock) void measure_clear_slices_kernel(const int64_t* __restrict__ table,
                                                                      int* __restrict__ slice_end, int64_t n) {
  const int64_t rows = table[hSlices] < n ? table[hSlices] : n;
  for (int64_t r = int64_t{blockIdx.x} * kBlock + threadIdx.x; r < rows; r += int64_t{gridDim.x} * kBlock)
    slice_end[r] = 0;
}

// FILL false: count the in-plane candidates per slice row.  FILL true: write both lists through the cursors.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void measure_candidates_kernel(const int* __restrict__ roots,
                                                                    const int* __restrict__ slot, int64_t* table,
                                                                    int* slice_end, int* __restrict__ cand3,
                                                                    int* __restrict__ cand2, Vol v, int64_t cap) {
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < v.n; i += int64_t{gridDim.x} * kBlock) {
    const int r = roots[i];
    if (r == 0) continue;
    const int s = slot[r - 1];
    if (s >= cap) continue;
    const auto [x, y, z] = split_xyz(static_cast<int>(i), v.Y, v.Z);
    const unsigned m = face_neighbours(roots, i, x, y, z, v);
    if (!is_candidate(m, 2)) continue;  // a 3-D candidate is an in-plane one too
    int64_t* row = table + kHead + int64_t{s} * kRow;
    const int64_t sr = row[fSlice] + (z - (v.Z - row[fBox + 5]));  // fBox + 5: the maximum of Z - z
    if (sr < 0 || sr >= v.n) continue;                             // cannot happen; keeps the stores inside
    if (!FILL) {
      atomicAdd(&slice_end[sr], 1);
    } else {
      const int at = atomicAdd(&slice_end[sr], 1);
      if (at >= 0 && at < v.n) cand2[at] = static_cast<int>(i);
      if (is_candidate(m, 3)) {
        const u64 at3 = atomicAdd(reinterpret_cast<u64*>(row + fCandEnd), u64{1});
        if (at3 < static_cast<u64>(v.n)) cand3[at3] = static_cast<int>(i);
      }
    }
  }
}

// one workgroup: the slice rows' counts become exclusive offsets in place, the cursors of the fill; after the fill
// entry r is the end of row r, which is the start of row r + 1
__global__ __launch_bounds__(kBlock) void measure_scan_slices_kernel(int64_t* table, int* slice_end, int64_t n) {
  const int64_t rows = table[hSlices] < n ? table[hSlices] : n;
  int64_t carry = 0;
  for (int64_t base = 0; base < rows; base += kBlock) {
    const int64_t r = base + threadIdx.x;
    const int64_t c = r < rows ? slice_end[r] : 0;
    int64_t total;
    const int64_t e = block_scan_exclusive(c, &total);
    if (r < rows) slice_end[r] = static_cast<int>(carry + e);
    carry += total;
  }
  if (threadIdx.x == 0) table[hCand2] = carry;
}

// ------------------------------------------------------------------ M3
struct Units {
  int x, y, z;
};

__global__ __launch_bounds__(kBlock) void measure_diameter_kernel(const int* __restrict__ work, int64_t n_work,
                                                                  int64_t* table, const int* __restrict__ cand3,
                                                                  Vol v, Units u, int64_t cap) {
  __shared__ int tile_i[3][kPairTile];
  __shared__ int tile_j[3][kPairTile];
  const int64_t rows = table[hLesions] < cap ? table[hLesions] : cap;
  const int t = threadIdx.x;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t s = work[3 * w], ti = work[3 * w + 1], tj = work[3 * w + 2];
    if (s < 0 || s >= rows || ti < 0 || tj < ti) continue;  // uniform over the workgroup
    int64_t* row = table + kHead + s * kRow;
    const int64_t count = row[fCand], begin = row[fCandEnd] - count;  // after the fill the cursor is the end
    if (begin < 0 || count < 0 || begin + count > v.n || tj * kPairTile >= count) continue;
    const int64_t at_i = ti * kPairTile + t, at_j = tj * kPairTile + t;
    const bool on_i = at_i < count, on_j = at_j < count;
    const auto pi = split_xyz(on_i ? cand3[begin + at_i] : 0, v.Y, v.Z);
    const auto pj = split_xyz(on_j ? cand3[begin + at_j] : 0, v.Y, v.Z);
    tile_i[0][t] = pi.x * u.x, tile_i[1][t] = pi.y * u.y, tile_i[2][t] = pi.z * u.z;
    tile_j[0][t] = pj.x * u.x, tile_j[1][t] = pj.y * u.y, tile_j[2][t] = pj.z * u.z;
    __syncthreads();
    const int in_i = static_cast<int>(count - ti * kPairTile < kPairTile ? count - ti * kPairTile : kPairTile);
    int64_t top = 0;
    if (on_j) {
      const int ax = tile_j[0][t], ay = tile_j[1][t], az = tile_j[2][t];
      for (int k = 0; k < in_i; ++k) {  // every lane reads one address: a broadcast
        const int dx = tile_i[0][k] - ax, dy = tile_i[1][k] - ay, dz = tile_i[2][k] - az;
        const int64_t d = int64_t{dx} * dx + int64_t{dy} * dy + int64_t{dz} * dz;
        top = d > top ? d : top;
      }
    }
    top = block_max(top);  // its barriers also free the tiles for the next unit
    if (t == 0 && top > 0) atomicMax(reinterpret_cast<u64*>(row + fD3), static_cast<u64>(top));
  }
}

// ------------------------------------------------------------------ M4
struct Point2 {
  int x, y;
};

__device__ __forceinline__ Point2 plane_point(const int* __restrict__ cand2, int64_t at, const Vol& v, const Units& u) {
  const auto p = split_xyz(cand2[at], v.Y, v.Z);
  return {p.x * u.x, p.y * u.y};
}

__global__ __launch_bounds__(kBlock) void measure_plane_kernel(const int* __restrict__ work, int64_t n_work,
                                                               const int64_t* __restrict__ table,
                                                               const int* __restrict__ slice_end,
                                                               const int* __restrict__ cand2,
                                                               int64_t* __restrict__ slices, int64_t n_slices, Vol v,
                                                               Units u, int64_t cap) {
  __shared__ int tile[2][kPlaneTile];
  const int64_t rows = table[hLesions] < cap ? table[hLesions] : cap;
  const int t = threadIdx.x;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t s = work[2 * w], dz = work[2 * w + 1];
    if (s < 0 || s >= rows) continue;  // uniform over the workgroup, like every `continue` below
    const int64_t* row = table + kHead + s * kRow;
    const int64_t zext = row[fBox + 4] + row[fBox + 5] - v.Z, sr = row[fSlice] + dz;
    if (dz < 0 || dz >= zext || sr < 0 || sr >= n_slices || sr >= v.n) continue;
    const int64_t begin = sr > 0 ? slice_end[sr - 1] : 0, end = slice_end[sr], count = end - begin;
    if (begin < 0 || count < 0 || end > v.n) continue;
    const int64_t tiles = (count + kPlaneTile - 1) / kPlaneTile;
    int64_t d2 = 0, width = 0;
    for (int pass = 0; pass < 2; ++pass) {  // A: the largest squared distance; B: the widest caliper among its pairs
      int64_t top = 0;
      for (int64_t ti = 0; ti < tiles; ++ti) {
        const int64_t at = ti * kPlaneTile + t;
        const Point2 p = at < count ? plane_point(cand2, begin + at, v, u) : Point2{0, 0};
        tile[0][t] = p.x, tile[1][t] = p.y;
        __syncthreads();
        const int64_t left = count - ti * kPlaneTile;
        const int in_tile = static_cast<int>(left < kPlaneTile ? left : kPlaneTile);
        for (int64_t j = t; j < count; j += kBlock) {
          const Point2 a = plane_point(cand2, begin + j, v, u);
          for (int k = 0; k < in_tile && ti * kPlaneTile + k < j; ++k) {  // unordered pairs: the earlier one in LDS
            const int dx = tile[0][k] - a.x, dy = tile[1][k] - a.y;
            const int64_t d = int64_t{dx} * dx + int64_t{dy} * dy;
            if (pass == 0) {
              top = d > top ? d : top;
            } else if (d == d2) {
              int64_t lo = INT64_MAX, hi = INT64_MIN;
              for (int64_t r = 0; r < count; ++r) {
                const Point2 q = plane_point(cand2, begin + r, v, u);
                const int64_t proj = int64_t{-dy} * q.x + int64_t{dx} * q.y;
                lo = proj < lo ? proj : lo;
                hi = proj > hi ? proj : hi;
              }
              top = hi - lo > top ? hi - lo : top;
            }
          }
        }
        __syncthreads();
      }
      top = block_max(top);
      if (pass == 0) {
        d2 = top;
        if (d2 == 0) break;  // one point, or none: both measures are 0
      } else {
        width = top;
      }
    }
    if (t == 0) {
      slices[2 * sr] = d2;
      slices[2 * sr + 1] = width;
    }
  }
}

// one thread per lesion: the smallest z with the largest W
__global__ __launch_bounds__(kBlock) void measure_resolve_kernel(int64_t* table, const int64_t* __restrict__ slices,
                                                                 int64_t n_slices, int Z, int64_t cap) {
  const int64_t rows = table[hLesions] < cap ? table[hLesions] : cap;
  for (int64_t s = int64_t{blockIdx.x} * kBlock + threadIdx.x; s < rows; s += int64_t{gridDim.x} * kBlock) {
    int64_t* row = table + kHead + s * kRow;
    const int64_t z0 = Z - row[fBox + 5], zext = row[fBox + 4] - z0, first = row[fSlice];
    int64_t best_z = z0, best_d2 = 0, best_w = -1;
    for (int64_t dz = 0; dz < zext && first + dz < n_slices; ++dz) {
      const int64_t d2 = slices[2 * (first + dz)], w = slices[2 * (first + dz) + 1];
      if (w > best_w) best_z = z0 + dz, best_d2 = d2, best_w = w;
    }
    row[fPlaneZ] = best_z;
    row[fPlaneD2] = best_d2;
    row[fPlaneW] = best_w < 0 ? 0 : best_w;
  }
}

// ------------------------------------------------------------------ host
inline bool measure_voxels(int64_t X, int64_t Y, int64_t Z, int64_t* n) {
  return volume_voxels(X, Y, Z, false, n) && X <= kMmMaxExtent && Y <= kMmMaxExtent && Z <= kMmMaxExtent;
}

inline int64_t measure_table_i64s(int64_t X, int64_t Y, int64_t Z, int connectivity) {
  return kHead + kRow * lesion_rows(X, Y, Z, connectivity);
}

// header | slot int32[n] | slice ends int32[n] | 3-D candidates int32[n] | in-plane candidates int32[n]
inline int64_t measure_bytes(int64_t n) { return kHeaderBytes + 4 * round256(4 * n); }

struct MeasureBuffers {
  int *slot, *slice_end, *cand3, *cand2;
};

inline MeasureBuffers measure_buffers(void* workspace, int64_t n) {
  char* ws = static_cast<char*>(workspace) + kHeaderBytes;
  const int64_t part = round256(4 * n);
  return {reinterpret_cast<int*>(ws), reinterpret_cast<int*>(ws + part), reinterpret_cast<int*>(ws + 2 * part),
          reinterpret_cast<int*>(ws + 3 * part)};
}

// 2 * sum_a u_a^2 (N_a - 1)^2 < 2^62, for units that passed units_ok and extents that passed measure_voxels
inline bool bound_ok(int64_t X, int64_t Y, int64_t Z, const int64_t* units) {
  const int64_t extent[3] = {X, Y, Z};
  unsigned __int128 bound = 0;
  for (int a = 0; a < 3; ++a) {
    const unsigned __int128 d =
        static_cast<unsigned __int128>(units[a]) * static_cast<unsigned __int128>(extent[a] - 1);
    bound += d * d;
  }
  return 2 * bound < (static_cast<unsigned __int128>(1) << 62);
}

inline int check_measure(int64_t X, int64_t Y, int64_t Z, const int64_t* units) {
  int64_t n;
  if (!measure_voxels(X, Y, Z, &n)) return GTS_ERR_SHAPE;
  if (!units_ok(units)) return GTS_ERR_ARGKIND;
  return bound_ok(X, Y, Z, units) ? GTS_OK : GTS_ERR_SHAPE;
}

// the connectivity a table of table_i64s rows was sized for decides its capacity: the smaller one always fits
inline int64_t table_rows(int64_t table_i64s) { return (table_i64s - kHead) / kRow; }

}  // namespace
}  // namespace gts

extern "C" int64_t gts_measure_workspace(int64_t X, int64_t Y, int64_t Z) {
  int64_t n;
  return gts::measure_voxels(X, Y, Z, &n) ? gts::measure_bytes(n) : 0;
}

extern "C" int64_t gts_measure_table_i64s(int64_t X, int64_t Y, int64_t Z, int32_t connectivity) {
  int64_t n;
  if (!gts::measure_voxels(X, Y, Z, &n) || (connectivity != 6 && connectivity != 26)) return 0;
  return gts::measure_table_i64s(X, Y, Z, connectivity);
}

extern "C" int32_t gts_measure_check(int64_t X, int64_t Y, int64_t Z, const int64_t* units) {
  if (!units) return GTS_ERR_NULL;
  return gts::check_measure(X, Y, Z, units);
}

extern "C" int32_t gts_measure_tables_i16(const int16_t* labels, const int32_t* roots, int64_t X, int64_t Y, int64_t Z,
                                          int32_t region, int32_t connectivity, int64_t* table, int64_t table_i64s,
                                          void* workspace, int64_t workspace_bytes, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!labels || !roots || !table || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!measure_voxels(X, Y, Z, &n) || !grid_ok(grid_blocks) || workspace_bytes < measure_bytes(n))
    return GTS_ERR_SHAPE;
  if (region < 0 || region > 2 || (connectivity != 6 && connectivity != 26)) return GTS_ERR_ARGKIND;
  if (table_i64s < measure_table_i64s(X, Y, Z, connectivity)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const MeasureBuffers b = measure_buffers(workspace, n);
  const int64_t cap = lesion_rows(X, Y, Z, connectivity);
  const Vol v = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), n};
  if (hipMemsetAsync(table, 0, 8 * kHead, st) != hipSuccess) return launch_status();
  const int grid = grid_for(n, kBlock, grid_blocks);
  lesion_rows_kernel<kHead, kRow><<<grid, kBlock, 0, st>>>(roots, b.slot, table, n, cap);
  measure_tables_kernel<<<grid, kBlock, 0, st>>>(labels, roots, b.slot, table, v, region, cap);
  measure_scan_rows_kernel<<<1, kBlock, 0, st>>>(table, v.Z, cap);
  return launch_status();
}

extern "C" int32_t gts_measure_candidates(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, int64_t* table,
                                          int64_t table_i64s, void* workspace, int64_t workspace_bytes,
                                          int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !table || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!measure_voxels(X, Y, Z, &n) || !grid_ok(grid_blocks) || workspace_bytes < measure_bytes(n) ||
      table_i64s < measure_table_i64s(X, Y, Z, 26))
    return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const MeasureBuffers b = measure_buffers(workspace, n);
  const int64_t cap = table_rows(table_i64s);
  const Vol v = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), n};
  const int grid = grid_for(n, kBlock, grid_blocks);
  measure_clear_slices_kernel<<<grid, kBlock, 0, st>>>(table, b.slice_end, n);
  measure_candidates_kernel<false><<<grid, kBlock, 0, st>>>(roots, b.slot, table, b.slice_end, b.cand3, b.cand2, v,
                                                            cap);
  measure_scan_slices_kernel<<<1, kBlock, 0, st>>>(table, b.slice_end, n);
  measure_candidates_kernel<true><<<grid, kBlock, 0, st>>>(roots, b.slot, table, b.slice_end, b.cand3, b.cand2, v, cap);
  return launch_status();
}

extern "C" int32_t gts_measure_diameters(int64_t X, int64_t Y, int64_t Z, const int64_t* units, const int32_t* work,
                                         int64_t n_work, int64_t* table, int64_t table_i64s, const void* workspace,
                                         int64_t workspace_bytes, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!units || !table || !workspace || (n_work > 0 && !work)) return GTS_ERR_NULL;
  int64_t n;
  if (!measure_voxels(X, Y, Z, &n) || !grid_ok(grid_blocks) || workspace_bytes < measure_bytes(n) ||
      table_i64s < measure_table_i64s(X, Y, Z, 26) || n_work < 0 || n_work > INT32_MAX)
    return GTS_ERR_SHAPE;
  const int status = check_measure(X, Y, Z, units);
  if (status != GTS_OK) return status;
  if (n_work == 0) return GTS_OK;  // no lesion of two voxels: no pair kernel
  const MeasureBuffers b = measure_buffers(const_cast<void*>(workspace), n);
  const Vol v = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), n};
  const Units u = {static_cast<int>(units[0]), static_cast<int>(units[1]), static_cast<int>(units[2])};
  measure_diameter_kernel<<<grid_for(n_work, 1, grid_blocks), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      work, n_work, table, b.cand3, v, u, table_rows(table_i64s));
  return launch_status();
}

extern "C" int32_t gts_measure_planes(int64_t X, int64_t Y, int64_t Z, const int64_t* units, const int32_t* work,
                                      int64_t n_work, int64_t* slices, int64_t n_slices, int64_t* table,
                                      int64_t table_i64s, const void* workspace, int64_t workspace_bytes,
                                      int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!units || !table || !workspace || (n_work > 0 && !work) || (n_slices > 0 && !slices)) return GTS_ERR_NULL;
  int64_t n;
  if (!measure_voxels(X, Y, Z, &n) || !grid_ok(grid_blocks) || workspace_bytes < measure_bytes(n) ||
      table_i64s < measure_table_i64s(X, Y, Z, 26) || n_work < 0 || n_work > INT32_MAX || n_slices < 0 || n_slices > n)
    return GTS_ERR_SHAPE;
  const int status = check_measure(X, Y, Z, units);
  if (status != GTS_OK) return status;
  if (n_work == 0 || n_slices == 0) return GTS_OK;  // an empty region: nothing to measure, nothing launched
  hipStream_t st = static_cast<hipStream_t>(stream);
  const MeasureBuffers b = measure_buffers(const_cast<void*>(workspace), n);
  const Vol v = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), n};
  const Units u = {static_cast<int>(units[0]), static_cast<int>(units[1]), static_cast<int>(units[2])};
  const int64_t cap = table_rows(table_i64s);
  if (hipMemsetAsync(slices, 0, 16 * n_slices, st) != hipSuccess) return launch_status();
  measure_plane_kernel<<<grid_for(n_work, 1, grid_blocks), kBlock, 0, st>>>(work, n_work, table, b.slice_end, b.cand2,
                                                                          slices, n_slices, v, u, cap);
  measure_resolve_kernel<<<grid_for(cap < n_work ? cap : n_work, kBlock, grid_blocks), kBlock, 0, st>>>(
      table, slices, n_slices, v.Z, cap);
  return launch_status();
}
