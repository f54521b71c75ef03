// What the per-lesion features share on top of gts_volume.h: scoring (L1-L3, gts_lesionwise.hip), measuring (M1-M4,
// gts_measure.hip) and meshing (T1-T5, gts_mesh.hip) each give every lesion, a component of C1-C3, a row of a table.
// The Python half is gts/_lesions.py.  A new per-lesion feature includes this instead of copying a neighbour.
#pragma once
#include "gts_volume.h"

namespace gts {

// The most lesions (and so the most roots) a volume [X][Y][Z] can hold.  Connectivity 26: two voxels of one
// 2 x 2 x 2 cell are 26-adjacent, so no two lesions meet a cell: ceil(X/2) ceil(Y/2) ceil(Z/2).  Connectivity 6: one
// voxel per lesion gives voxels that are pairwise not face-adjacent, an independent set of the bipartite grid graph:
// ceil(n / 2).  Both are reached (a lattice of lone voxels, a checkerboard): a table of this many rows cannot overflow.
inline int64_t lesion_rows(int64_t X, int64_t Y, int64_t Z, int connectivity) {
  return connectivity == 26 ? ((X + 1) / 2) * ((Y + 1) / 2) * ((Z + 1) / 2) : (X * Y * Z + 1) / 2;
}

// The convention of the int64 tables: HEAD words of header, then rows of ROW fields.  Head word 0 counts the lesions
// (the caller clears the head); every root voxel i (roots[i] == i + 1) takes the next slot from it, writes the slot to
// slot[i] and its root to field 0 of that row, and clears the row's other fields: only the rows in use are cleared, not
// a table sized for the worst case.  Slot order is arrival order; the host sorts by root.  A slot at or beyond `cap`
// gets no row and is stored as `cap` (cannot happen for the roots of C1-C3 at a cap of lesion_rows).
template <int HEAD, int ROW>
__global__ __launch_bounds__(kBlock) void lesion_rows_kernel(const int* __restrict__ roots, int* __restrict__ slot,
                                                             int64_t* table, int64_t n, int64_t cap) {
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    if (roots[i] != i + 1) continue;
    const int64_t s = static_cast<int64_t>(atomicAdd(reinterpret_cast<unsigned long long*>(table), 1ull));
    slot[i] = static_cast<int>(s < cap ? s : cap);
    if (s >= cap) continue;
    int64_t* row = table + HEAD + s * ROW;
    row[0] = i + 1;
#pragma unroll
    for (int f = 1; f < ROW; ++f) row[f] = 0;
  }
}

// The grid rule: a grid_blocks of 0 leaves the choice to the library, one workgroup per `per_block` items and at
// most 65 536; any other is taken as it is (the kernels stride, so no value depends on it).
constexpr int64_t kLesionMaxGrid = 1 << 16;

inline bool grid_ok(int64_t grid_blocks) { return grid_blocks >= 0 && grid_blocks <= INT32_MAX; }

inline int grid_for(int64_t items, int64_t per_block, int64_t grid_blocks) {
  const int64_t need = items > 0 ? (items + per_block - 1) / per_block : 1;
  return static_cast<int>(grid_blocks > 0 ? grid_blocks : (need < kLesionMaxGrid ? need : kLesionMaxGrid));
}

}  // namespace gts
