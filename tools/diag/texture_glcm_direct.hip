// The form of X3 (csrc/gts_texture.hip) that lost: the same work units, the same neighbour test, but every add goes
// straight to the global folded matrix, no LDS tile.  Same arguments as gts_texture_glcm, so tools/measure_texture.py
// can put it in the library's place for one timed run.  Not part of the library; built by the tool:
//   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Iinclude -Ignn-tumor-seg_amd/csrc -shared
//         tools/diag/texture_glcm_direct.hip -o tools/diag/texture_glcm_direct.so
#include "gts_lesions.h"

namespace {

using namespace gts;

constexpr int kChunk = GTS_TEXTURE_CHUNK;
constexpr int kDirections = GTS_TEXTURE_DIRECTIONS;
constexpr int kPlanRow = GTS_TEXTURE_PLAN_I64;

__constant__ int kOffsets[kDirections][3] = {{0, 0, 1},  {0, 1, -1}, {0, 1, 0},  {0, 1, 1}, {1, -1, -1},
                                             {1, -1, 0}, {1, -1, 1}, {1, 0, -1}, {1, 0, 0}, {1, 0, 1},
                                             {1, 1, -1}, {1, 1, 0},  {1, 1, 1}};

__global__ __launch_bounds__(kBlock) void glcm_direct_kernel(const int* __restrict__ roots,
                                                             const int* __restrict__ work, int64_t n_work,
                                                             const int* __restrict__ segments,
                                                             const int64_t* __restrict__ plan, int L,
                                                             const int* __restrict__ list,
                                                             const uint8_t* __restrict__ levels, int64_t n_listed,
                                                             const uint8_t* __restrict__ level_volume, int* glcm,
                                                             int G, int X, int Y, int Z, int64_t n) {
  const int64_t stride = int64_t{G} * (G + 1) / 2;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int l = work[3 * w], d = work[3 * w + 1], c = work[3 * w + 2];
    if (l < 0 || l >= L || d < 0 || d >= kDirections || c < 0) continue;
    const int64_t begin = segments[l], end = segments[l + 1], first = begin + int64_t{c} * kChunk;
    const int64_t* row = plan + int64_t{l} * kPlanRow;
    const int n_levels = static_cast<int>(row[2]), root = static_cast<int>(row[3]);
    if (begin < 0 || end > n_listed || first >= end || n_levels < 1 || n_levels > G) continue;
    const int dx = kOffsets[d][0], dy = kOffsets[d][1], dz = kOffsets[d][2];
    const int64_t step = (int64_t{dx} * Y + dy) * Z + dz;
    const int64_t last = first + kChunk < end ? first + kChunk : end;
    int* out = glcm + (int64_t{l} * kDirections + d) * stride;
    for (int64_t k = first + threadIdx.x; k < last; k += kBlock) {
      const int p = list[k];
      if (p < 0 || p >= n) continue;
      const auto [x, y, z] = split_xyz(p, Y, Z);
      const int qx = x + dx, qy = y + dy, qz = z + dz;
      if (qx < 0 || qx >= X || qy < 0 || qy >= Y || qz < 0 || qz >= Z) continue;
      const int64_t q = p + step;
      if (roots[q] != root) continue;
      const int gp = levels[k], gq = level_volume[q];
      if (gp >= n_levels || gq >= n_levels) continue;
      const int i = gp < gq ? gp : gq, j = gp < gq ? gq : gp;
      atomicAdd(&out[j * (j + 1) / 2 + i], 1);
    }
  }
}

}  // namespace

extern "C" int32_t diag_texture_glcm_direct(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, const int32_t* work,
                                            int64_t n_work, const int32_t* segments, const int64_t* plan,
                                            int64_t lesions, const int32_t* list, const uint8_t* levels,
                                            int64_t n_listed, int32_t* table, int64_t table_words, int64_t max_levels,
                                            const void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                                            void* stream) {
  // the library's own checks have passed on the same arguments in the run before; only what indexing needs is here
  int64_t n;
  if (!roots || !work || !segments || !plan || !list || !levels || !table || !workspace) return GTS_ERR_NULL;
  if (!volume_voxels(X, Y, Z, false, &n) || n_work < 1 || lesions < 1 || max_levels < 1 ||
      max_levels > GTS_TEXTURE_MAX_LEVELS || workspace_bytes < kHeaderBytes + round256(4 * n) + round256(n) ||
      table_words < lesions * (max_levels + kDirections * (max_levels * (max_levels + 1) / 2)))
    return GTS_ERR_SHAPE;
  const uint8_t* level_volume = static_cast<const uint8_t*>(workspace) + kHeaderBytes + round256(4 * n);
  glcm_direct_kernel<<<grid_for(n_work, 1, grid_blocks), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      roots, work, n_work, segments, plan, static_cast<int>(lesions), list, levels, n_listed, level_volume,
      table + lesions * max_levels, static_cast<int>(max_levels), static_cast<int>(X), static_cast<int>(Y),
      static_cast<int>(Z), n);
  return hipGetLastError() == hipSuccess ? GTS_OK : GTS_ERR_SHAPE;
}
