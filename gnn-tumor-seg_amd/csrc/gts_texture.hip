// X1-X3: the device half of the per-lesion intensity and texture tables (gts/texture.py): per selected
// lesion the range of a scan's values, the grey levels, their histogram and the grey-level co-occurrence matrix (GLCM)
// over the 13 directions at distance 1.  What a user otherwise does on the host with one mask per lesion and shifted
// array comparisons in numpy.  The lesions are the components of C1-C3 over the region's mask, unchanged.
//
// Definitions.  roots int32 [X][Y][Z] (Z contiguous) and a scan of the same shape, int16 or float32.  A lesion is the
// set of voxels of one root; the host selects lesions (by size) and numbers them 0 .. L - 1 by ascending root.
//   range    lo, hi = the smallest and largest value over the lesion, by comparison only: integer atomics on an
//            order-preserving encoding (int16: v + 32768; float32: the bits of v + 0.0f, all flipped when the sign is
//            set, else the sign flipped).  A float32 NaN or Inf is counted, per lesion and in the head, and takes part
//            in nothing else.
//   levels   one rounded float64 operation each, no contraction.  Fixed bin number N: g = min(N - 1, floor((double(v)
//            - lo) * double(N) / (hi - lo))), 0 when hi == lo.  Fixed bin width w: g = floor(double(v) / w) -
//            floor(lo / w).  The host derives `levels` per lesion from (lo, hi) and refuses more than 128.
//   hist     hist[l][g] = voxels of lesion l at level g.
//   GLCM     directions d = 0 .. 12: the offsets (dx, dy, dz) in {-1, 0, 1}^3 whose first non-zero component is
//            positive, in ascending (dx, dy, dz).  fold[l][d][j (j + 1) / 2 + i], i <= j, = the number of voxels p of
//            lesion l whose neighbour q = p + delta_d is inside the volume and has the same root, with {g(p), g(q)} =
//            {i, j}: every unordered neighbouring pair once.  The public symmetric matrix is fold off the diagonal
//            and 2 fold on it.  The index does not depend on the lesion's number of levels.
//
//   X1  counts: every root takes a row (gts_lesions.h) and one pass adds every voxel to its root's count; the host
//       selects from them.  ranges: one pass over roots and the scan for the selected lesions, the lanes of one
//       lesion reduced in the wave first; the same pass writes each lesion's voxel indices into its segment of a
//       compact list through an atomic cursor (the order inside a segment is arrival order; only sums follow).
//   X2  per listed voxel the grey level, stored beside the list and scattered into a level volume, and the histogram,
//       a workgroup's 256 voxels counted in LDS first.
//   X3  work units (lesion, direction, chunk of GTS_TEXTURE_CHUNK listed voxels).  A workgroup counts a unit in an
//       LDS tile of the folded triangle (128 levels: 8256 int32, 33 KiB) with LDS atomics and flushes the entries that
//       are not zero with global atomics.
//
// Integer atomics (add, min, max), float64 level arithmetic that is one rounded operation per step, and plain vector
// stores only: identical results on every run and at every grid_blocks.  What X4-X6 (gts_texture_matrices.hip, the
// run, zone and neighbourhood tables) share with these passes is in gts_texture.h.  Limits: those of gts_measure_check's shape
// (every extent in [1, 4097], X * Y * Z < 2^31).  A count is at most the lesion's voxels, so int32 holds it.
#include <type_traits>

#include "gts_texture.h"

namespace gts {
namespace {

constexpr int kTriangle = kMaxLevels * (kMaxLevels + 1) / 2;

static_assert(kTriangle * 4 <= 48 * 1024, "the folded tile leaves LDS for a second workgroup per CU");

// range row fields; head word 0 counts the non-finite voxels of all selected lesions
enum { rLo = 0, rHi = 1, rCursor = 2, rNonFinite = 3 };

__host__ __device__ constexpr int64_t triangle(int64_t levels) { return levels * (levels + 1) / 2; }

// a < b as values  <=>  encode(a) < encode(b) as unsigned
__device__ __forceinline__ unsigned encode(int16_t v) { return static_cast<unsigned>(static_cast<int>(v) + 32768); }
__device__ __forceinline__ unsigned encode(float v) {
  const unsigned b = __float_as_uint(v + 0.0f);  // -0.0 becomes +0.0: they compare equal
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename T>
__device__ __forceinline__ bool finite_value(T v) {
  if constexpr (std::is_same<T, float>::value) return is_finite(v);
  return true;
}

// ------------------------------------------------------------------ X1: counts
__global__ __launch_bounds__(kBlock) void texture_count_kernel(const int* __restrict__ roots,
                                                               const int* __restrict__ slot, int64_t* counts,
                                                               int64_t n, int64_t cap) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t base = int64_t{blockIdx.x} * kBlock; base < n; base += int64_t{gridDim.x} * kBlock) {
    const int64_t i = base + threadIdx.x;  // the trip count is the workgroup's: every lane reaches the wave loop
    const int r = i < n ? roots[i] : 0;
    bool on = r > 0 && r <= n;
    const int s = on ? slot[r - 1] : 0;
    on = on && s >= 0 && s < cap;
    wave_for_each_key(on, s, [&](int key, u64 same, bool) {
      if (lane == 0)
        atomicAdd(reinterpret_cast<u64*>(counts + kHead + int64_t{key} * kCountRow + 1),
                  static_cast<u64>(__popcll(same)));
    });
  }
}

// ------------------------------------------------------------------ X1: ranges and the compact list
__global__ __launch_bounds__(kBlock) void texture_init_ranges_kernel(int64_t* ranges,
                                                                     const int* __restrict__ segments, int64_t L) {
  for (int64_t l = int64_t{blockIdx.x} * kBlock + threadIdx.x; l < L; l += int64_t{gridDim.x} * kBlock) {
    int64_t* row = ranges + kHead + l * kRangeRow;
    row[rLo] = int64_t{0xFFFFFFFF};
    row[rHi] = 0;
    row[rCursor] = segments[l];
    row[rNonFinite] = 0;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void texture_range_kernel(const int* __restrict__ roots,
                                                               const T* __restrict__ image,
                                                               const int* __restrict__ slot,
                                                               const int* __restrict__ select, int64_t n_rows,
                                                               const int* __restrict__ segments, int64_t L,
                                                               int64_t* ranges, int* __restrict__ list,
                                                               int64_t n_listed, int64_t n) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t base = int64_t{blockIdx.x} * kBlock; base < n; base += int64_t{gridDim.x} * kBlock) {
    const int64_t i = base + threadIdx.x;
    const int r = i < n ? roots[i] : 0;
    bool on = r > 0 && r <= n;
    const int s = on ? slot[r - 1] : -1;
    on = on && s >= 0 && s < n_rows;
    const int l = on ? select[s] : -1;
    on = on && l >= 0 && l < L;
    // only a selected lesion's voxel is read as a number
    const T v = on ? image[i] : T(0);
    const bool finite = finite_value(v);
    const unsigned enc = encode(finite ? v : T(0));
    wave_for_each_key(on, l, [&](int key, u64 same, bool mine) {
      const bool use = mine && finite;
      const unsigned lo = wave_reduce(use ? enc : 0xFFFFFFFFu, [](unsigned a, unsigned b) { return a < b ? a : b; });
      const unsigned hi = wave_reduce(use ? enc : 0u, [](unsigned a, unsigned b) { return a > b ? a : b; });
      const int bad = __popcll(__ballot(mine && !finite));
      u64* row = reinterpret_cast<u64*>(ranges + kHead + int64_t{key} * kRangeRow);
      u64 at = 0;
      if (lane == 0) {
        if (__popcll(same) > bad) {
          atomicMin(row + rLo, static_cast<u64>(lo));
          atomicMax(row + rHi, static_cast<u64>(hi));
        }
        if (bad) {
          atomicAdd(row + rNonFinite, static_cast<u64>(bad));
          atomicAdd(reinterpret_cast<u64*>(ranges), static_cast<u64>(bad));
        }
        at = atomicAdd(row + rCursor, static_cast<u64>(__popcll(same)));
      }
      at = __shfl(at, 0, kWave);
      if (mine) {
        const u64 mine_at = at + static_cast<u64>(__popcll(same & ((u64{1} << lane) - 1)));
        // inside the lesion's own segment when the plan's counts are the volume's; the test keeps the store inside
        if (mine_at < static_cast<u64>(segments[key + 1]) && mine_at < static_cast<u64>(n_listed))
          list[mine_at] = static_cast<int>(i);
      }
    });
  }
}

// ------------------------------------------------------------------ X2: levels and histogram
template <typename T>
__global__ __launch_bounds__(kBlock) void texture_levels_kernel(const T* __restrict__ image, int bins, double width,
                                                                const int* __restrict__ segments,
                                                                const int64_t* __restrict__ plan, int L,
                                                                const int* __restrict__ list, int64_t n_listed,
                                                                uint8_t* __restrict__ levels,
                                                                uint8_t* __restrict__ level_volume, int* hist, int G,
                                                                int64_t n) {
  // A workgroup's 256 listed voxels are almost always one lesion's, the lesion of its first: that lesion counts in
  // LDS and flushes the levels in use; a voxel of a later lesion (a segment ends inside the 256) adds globally.
  __shared__ unsigned block_hist[kMaxLevels];
  for (int64_t base = int64_t{blockIdx.x} * kBlock; base < n_listed; base += int64_t{gridDim.x} * kBlock) {
    const int home = lesion_of(segments, L, base);  // uniform over the workgroup, like the trip count
    block_hist_clear(block_hist, G);
    const int64_t k = base + threadIdx.x;
    const int l = k < n_listed ? lesion_of(segments, L, k) : home;
    const int p = k < n_listed ? list[k] : -1;
    const int64_t* row = plan + int64_t{l} * kPlanRow;
    const int top = static_cast<int>(row[pLevels]) - 1;
    // false only beyond the list, or for a plan that is not the volume's
    if (p >= 0 && p < n && k < segments[l + 1] && top >= 0 && top < G) {
      const double lo = __longlong_as_double(row[pLo]), hi = __longlong_as_double(row[pHi]);
      const double v = static_cast<double>(image[p]);
      double g;
      if (width > 0.0) {
        g = floor(v / width) - floor(lo / width);
      } else if (hi == lo) {
        g = 0.0;
      } else {
        g = floor((v - lo) * static_cast<double>(bins) / (hi - lo));
      }
      // g lies in [0, top + 1] for lo <= v <= hi (rounding is monotone); top + 1 is v == hi under a bin number
      const int level = g >= static_cast<double>(top) ? top : (g > 0.0 ? static_cast<int>(g) : 0);
      levels[k] = static_cast<uint8_t>(level);
      level_volume[p] = static_cast<uint8_t>(level);
      if (l == home) {
        atomicAdd(&block_hist[level], 1u);
      } else {
        atomicAdd(&hist[int64_t{l} * G + level], 1);
      }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += kBlock)
      if (block_hist[g]) atomicAdd(&hist[int64_t{home} * G + g], static_cast<int>(block_hist[g]));
    __syncthreads();  // the counters are free for the next 256
  }
}

// ------------------------------------------------------------------ X3: co-occurrence
__global__ __launch_bounds__(kBlock) void texture_glcm_kernel(const int* __restrict__ roots,
                                                              const int* __restrict__ work, int64_t n_work,
                                                              const int* __restrict__ segments,
                                                              const int64_t* __restrict__ plan, int L,
                                                              const int* __restrict__ list,
                                                              const uint8_t* __restrict__ levels, int64_t n_listed,
                                                              const uint8_t* __restrict__ level_volume, int* glcm,
                                                              int G, Vol v) {
  __shared__ unsigned tile[kTriangle];
  const int64_t stride = triangle(G);
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int l = work[3 * w], d = work[3 * w + 1], c = work[3 * w + 2];
    if (l < 0 || l >= L || d < 0 || d >= kDirections || c < 0) continue;  // uniform over the workgroup
    const int64_t begin = segments[l], end = segments[l + 1], first = begin + int64_t{c} * kChunk;
    const int64_t* row = plan + int64_t{l} * kPlanRow;
    const int n_levels = static_cast<int>(row[pLevels]), root = static_cast<int>(row[pRoot]);
    if (begin < 0 || end > n_listed || first >= end || n_levels < 1 || n_levels > G) continue;
    const int cells = static_cast<int>(triangle(n_levels));
    for (int e = threadIdx.x; e < cells; e += kBlock) tile[e] = 0;
    __syncthreads();
    const int dx = kOffsets[d][0], dy = kOffsets[d][1], dz = kOffsets[d][2];
    const int64_t step = (int64_t{dx} * v.Y + dy) * v.Z + dz;
    const int64_t last = first + kChunk < end ? first + kChunk : end;
    for (int64_t k = first + threadIdx.x; k < last; k += kBlock) {
      const int p = list[k];
      if (p < 0 || p >= v.n) continue;
      const auto [x, y, z] = split_xyz(p, v.Y, v.Z);
      const int qx = x + dx, qy = y + dy, qz = z + dz;
      if (qx < 0 || qx >= v.X || qy < 0 || qy >= v.Y || qz < 0 || qz >= v.Z) continue;
      const int64_t q = p + step;
      if (roots[q] != root) continue;  // the same root, not merely the same mask
      const int gp = levels[k], gq = level_volume[q];
      if (gp >= n_levels || gq >= n_levels) continue;  // cannot happen after X2; keeps the add inside the tile
      const int i = gp < gq ? gp : gq, j = gp < gq ? gq : gp;
      atomicAdd(&tile[j * (j + 1) / 2 + i], 1u);
    }
    __syncthreads();
    int* out = glcm + (int64_t{l} * kDirections + d) * stride;
    for (int e = threadIdx.x; e < cells; e += kBlock)
      if (tile[e]) atomicAdd(&out[e], static_cast<int>(tile[e]));
    __syncthreads();  // the tile is free for the next unit
  }
}

// ------------------------------------------------------------------ host
// int32 words of hist [L][G] and the folded glcm [L][13][G (G + 1) / 2]; 0 outside the limits or above the byte cap
inline int64_t table_words(int64_t lesions, int64_t levels) {
  if (lesions < 0 || lesions > INT32_MAX || levels < 1 || levels > kMaxLevels) return 0;
  const int64_t words = lesions * (levels + kDirections * triangle(levels));
  return 4 * words <= int64_t{GTS_TEXTURE_MAX_TABLE_BYTES} ? words : 0;
}

inline bool bins_ok(int32_t bins, double width) {
  if (!(width >= 0.0) || !is_finite(width)) return false;
  return width > 0.0 || (bins >= 1 && bins <= kMaxLevels);
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_texture_workspace(int64_t X, int64_t Y, int64_t Z) {
  int64_t n;
  return gts::texture_voxels(X, Y, Z, &n) ? gts::texture_bytes(n) : 0;
}

extern "C" int64_t gts_texture_count_i64s(int64_t X, int64_t Y, int64_t Z, int32_t connectivity) {
  int64_t n;
  if (!gts::texture_voxels(X, Y, Z, &n) || (connectivity != 6 && connectivity != 26)) return 0;
  return gts::kHead + gts::kCountRow * gts::lesion_rows(X, Y, Z, connectivity);
}

extern "C" int64_t gts_texture_table_words(int64_t lesions, int64_t levels) {
  return gts::table_words(lesions, levels);
}

extern "C" int32_t gts_texture_counts(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, int32_t connectivity,
                                      int64_t* counts, int64_t counts_i64s, void* workspace, int64_t workspace_bytes,
                                      int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !counts || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!texture_voxels(X, Y, Z, &n)) return GTS_ERR_SHAPE;
  if (connectivity != 6 && connectivity != 26) return GTS_ERR_ARGKIND;
  if (!grid_ok(grid_blocks)) return GTS_ERR_SHAPE;
  const int64_t cap = lesion_rows(X, Y, Z, connectivity);
  if (workspace_bytes < texture_bytes(n) || counts_i64s < kHead + kCountRow * cap) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TextureBuffers b = texture_buffers(workspace, n);
  if (hipMemsetAsync(counts, 0, 8 * kHead, st) != hipSuccess) return launch_status();
  const int grid = grid_for(n, kBlock, grid_blocks);
  lesion_rows_kernel<kHead, kCountRow><<<grid, kBlock, 0, st>>>(roots, b.slot, counts, n, cap);
  texture_count_kernel<<<grid, kBlock, 0, st>>>(roots, b.slot, counts, n, cap);
  return launch_status();
}

extern "C" int32_t gts_texture_ranges(const int32_t* roots, const void* image, int32_t dtype, int64_t X, int64_t Y,
                                      int64_t Z, const int32_t* select, int64_t n_rows, const int32_t* segments,
                                      int64_t lesions, int64_t* ranges, int64_t ranges_i64s, int32_t* list,
                                      int64_t n_listed, const void* workspace, int64_t workspace_bytes,
                                      int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !image || !select || !segments || !ranges || !list || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!texture_voxels(X, Y, Z, &n) || n_rows < 1 || n_rows > n || lesions < 1 || lesions > n_rows || n_listed < 1 ||
      n_listed > n)
    return GTS_ERR_SHAPE;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  if (!grid_ok(grid_blocks)) return GTS_ERR_SHAPE;
  if (workspace_bytes < texture_bytes(n) || ranges_i64s < kHead + kRangeRow * lesions) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TextureBuffers b = texture_buffers(const_cast<void*>(workspace), n);
  if (hipMemsetAsync(ranges, 0, 8 * kHead, st) != hipSuccess) return launch_status();
  texture_init_ranges_kernel<<<grid_for(lesions, kBlock, grid_blocks), kBlock, 0, st>>>(ranges, segments, lesions);
  const int grid = grid_for(n, kBlock, grid_blocks);
  return with_scan_type(dtype, image, [&](auto* src) {
    texture_range_kernel<<<grid, kBlock, 0, st>>>(roots, src, b.slot, select, n_rows, segments, lesions, ranges, list,
                                                  n_listed, n);
    return launch_status();
  });
}

extern "C" int32_t gts_texture_levels(const void* image, int32_t dtype, int64_t X, int64_t Y, int64_t Z, int32_t bins,
                                      double bin_width, const int32_t* segments, const int64_t* plan, int64_t lesions,
                                      const int32_t* list, int64_t n_listed, uint8_t* levels, int32_t* table,
                                      int64_t table_words, int64_t max_levels, void* workspace,
                                      int64_t workspace_bytes, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!image || !segments || !plan || !list || !levels || !table || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!texture_voxels(X, Y, Z, &n) || lesions < 1 || lesions > n || n_listed < 1 || n_listed > n)
    return GTS_ERR_SHAPE;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  if (!bins_ok(bins, bin_width)) return GTS_ERR_ARGKIND;
  if (!grid_ok(grid_blocks)) return GTS_ERR_SHAPE;
  const int64_t words = gts::table_words(lesions, max_levels);
  if (workspace_bytes < texture_bytes(n) || words == 0 || table_words < words) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TextureBuffers b = texture_buffers(workspace, n);
  if (hipMemsetAsync(table, 0, 4 * words, st) != hipSuccess) return launch_status();
  const int grid = grid_for(n_listed, kBlock, grid_blocks);
  return with_scan_type(dtype, image, [&](auto* src) {
    texture_levels_kernel<<<grid, kBlock, 0, st>>>(src, bins, bin_width, segments, plan, static_cast<int>(lesions),
                                                   list, n_listed, levels, b.level_volume, table,
                                                   static_cast<int>(max_levels), n);
    return launch_status();
  });
}

extern "C" int32_t gts_texture_glcm(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, const int32_t* work,
                                    int64_t n_work, const int32_t* segments, const int64_t* plan, int64_t lesions,
                                    const int32_t* list, const uint8_t* levels, int64_t n_listed, int32_t* table,
                                    int64_t table_words, int64_t max_levels, const void* workspace,
                                    int64_t workspace_bytes, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !segments || !plan || !list || !levels || !table || !workspace || (n_work > 0 && !work))
    return GTS_ERR_NULL;
  int64_t n;
  if (!texture_voxels(X, Y, Z, &n) || lesions < 1 || lesions > n || n_listed < 1 || n_listed > n || n_work < 0 ||
      n_work > INT32_MAX)
    return GTS_ERR_SHAPE;
  if (!grid_ok(grid_blocks)) return GTS_ERR_SHAPE;
  const int64_t words = gts::table_words(lesions, max_levels);
  if (workspace_bytes < texture_bytes(n) || words == 0 || table_words < words) return GTS_ERR_SHAPE;
  if (n_work == 0) return GTS_OK;
  const TextureBuffers b = texture_buffers(const_cast<void*>(workspace), n);
  const Vol v = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), n};
  texture_glcm_kernel<<<grid_for(n_work, 1, grid_blocks), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      roots, work, n_work, segments, plan, static_cast<int>(lesions), list, levels, n_listed, b.level_volume,
      table + lesions * max_levels, static_cast<int>(max_levels), v);
  return launch_status();
}
