// S1-S6: morphological brain extraction of one MRI volume: threshold, erode, keep the largest
// component, dilate, close, fill holes, apply.  What a user otherwise does on the host with scipy.ndimage.
//
// A volume has three axes [X][Y][Z] with Z contiguous (the definition is symmetric in the axes, so the caller hands a
// tensor's shape over as it is); masks are int16 0/1 volumes, so C1-C3 of gts_components.hip serve unchanged.
//
//   S1  range: n = the voxels that are finite and > 0, hi = their maximum.  The maximum is taken over the float32
//       bit patterns, which order like the values for positive floats: one integer atomicMax per wave and workgroup;
//   S2  histogram: 4096 bins over (0, hi] in a 16 KB LDS table of uint32 per workgroup, one global atomic per non-empty
//       bin and workgroup; then the threshold mask M0 = (v finite, v > 0, float64(v) >= t) and its count;
//   S3  ball erosion / dilation as an exact squared-distance test with a window bounded by r = floor(sqrt(R2)) <= 15:
//       along Z the 1-D distance to the nearest target, capped at r + 1, one byte (lines staged in LDS); along Y the
//       minimum of g^2 + d^2 over |d| <= r, capped at R2 + 1, two bytes; along X the same minimum compared with R2.
//       A cap only replaces values that are above R2 already, so the comparison is exact;
//   S4  largest component: sizes by root with integer atomics (one per wave and root), the winner by one 64-bit
//       atomicMax over (size << 32) | (0xFFFFFFFF - root), so that a tie goes to the smaller root, then the runner-up;
//   S5  hole fill: roots of the complement at connectivity 6, every root that owns a voxel on a face flagged,
//       B = C or (complement voxel whose root is not flagged);
//   S6  apply: every modality keeps its value where B is set and becomes 0 elsewhere, dtype preserved.
//
// Every result is an integer (or a copy of an input value) that does not depend on scheduling or on the grid.
#include "gts_scan.h"

namespace gts {
namespace {

constexpr int kBins = GTS_BRAIN_BINS;
constexpr int kMaxR2 = GTS_BRAIN_MAX_R2;
constexpr int kMaxRadius = 15;                     // floor(sqrt(kMaxR2))
constexpr int kLineTile = 4 * kBlock;              // S3, along Z: voxels one workgroup stages at a time
constexpr int kMaxGrid = 2048;                     // the library's choice of workgroups at the most
constexpr int kMaxChannels = 64;
static_assert(kMaxRadius * kMaxRadius <= kMaxR2 && (kMaxRadius + 1) * (kMaxRadius + 1) > kMaxR2, "radius of R2");

template <typename T>
__device__ __forceinline__ bool positive_finite(T v) {
  const float f = static_cast<float>(v);
  return is_finite(f) && f > 0.f;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  return wave_reduce(v, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
}

// ------------------------------------------------------------------ S1
// out[0] += members, out[1] = max(out[1], float32 bits of the largest member); out is cleared before the launch
template <typename T>
__global__ __launch_bounds__(kBlock) void brain_range_kernel(const T* __restrict__ src, int64_t n,
                                                             unsigned long long* __restrict__ out) {
  __shared__ unsigned block_best;
  if (threadIdx.x == 0) block_best = 0;
  __syncthreads();
  unsigned mine[1] = {0};
  unsigned best = 0;
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const T v = src[i];
    if (positive_finite(v)) {
      const unsigned bits = __float_as_uint(static_cast<float>(v));
      best = bits > best ? bits : best;
      ++mine[0];
    }
  }
  best = static_cast<unsigned>(wave_max_u64(best));
  if ((threadIdx.x & (kWave - 1)) == 0 && best) atomicMax(&block_best, best);
  __syncthreads();
  if (threadIdx.x == 0 && block_best) atomicMax(&out[1], static_cast<unsigned long long>(block_best));
  block_add_counters(mine, out);
}

// ------------------------------------------------------------------ S2
template <typename T>
__global__ __launch_bounds__(kBlock) void brain_histogram_kernel(const T* __restrict__ src, int64_t n, double hi,
                                                                 unsigned long long* __restrict__ counts) {
  __shared__ unsigned hist[kBins];
  block_hist_clear(hist, kBins);
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const T v = src[i];
    if (positive_finite(v)) {
      const double q = floor(static_cast<double>(v) / hi * static_cast<double>(kBins));
      atomicAdd(&hist[q < static_cast<double>(kBins - 1) ? static_cast<int>(q) : kBins - 1], 1u);
    }
  }
  block_hist_flush(hist, kBins, counts);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void brain_threshold_kernel(const T* __restrict__ src, int64_t n, double t,
                                                                 int16_t* __restrict__ mask,
                                                                 unsigned long long* __restrict__ count) {
  unsigned mine[1] = {0};
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const T v = src[i];
    const bool member = positive_finite(v) && static_cast<double>(v) >= t;
    mask[i] = member ? 1 : 0;
    mine[0] += member ? 1u : 0u;
  }
  block_add_counters(mine, count);
}

// ------------------------------------------------------------------ S3
// Along Z.  A workgroup stages the target bits of kLineTile consecutive voxels and kMaxRadius + 1 on either side
// (lines follow one another in memory; where a line ends is the index's business, not the tile's).
__global__ __launch_bounds__(kBlock) void morph_z_kernel(const int16_t* __restrict__ mask, int64_t n, int Z, int r,
                                                         int target, int outside, uint8_t* __restrict__ g) {
  constexpr int kHalo = kMaxRadius + 1;
  __shared__ uint8_t hit[kLineTile + 2 * kHalo];
  const int64_t tiles = (n + kLineTile - 1) / kLineTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kLineTile;
    __syncthreads();  // the previous tile has been read
    for (int j = threadIdx.x; j < kLineTile + 2 * kHalo; j += kBlock) {
      const int64_t i = base - kHalo + j;
      hit[j] = (i >= 0 && i < n) ? ((mask[i] != 0) == (target != 0)) : 0;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < kLineTile && base + j < n; j += kBlock) {
      const int z = static_cast<int>((base + j) % Z);
      const uint8_t* at = hit + kHalo + j;
      int d = 0;
      for (; d <= r; ++d) {
        const bool below = z - d >= 0 ? at[-d] != 0 : outside != 0;
        const bool above = z + d < Z ? at[d] != 0 : outside != 0;
        if (below || above) break;
      }
      g[base + j] = static_cast<uint8_t>(d);  // r + 1: nothing within r
    }
  }
}

// Along Y: h = min(R2 + 1, min over |d| <= r of g(y + d)^2 + d^2); a position outside counts as a target or not at all.
__global__ __launch_bounds__(kBlock) void morph_y_kernel(const uint8_t* __restrict__ g, int64_t n, int Y, int Z, int r,
                                                         int R2, int outside, uint16_t* __restrict__ h) {
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const int y = static_cast<int>((i / Z) % Y);
    int best = R2 + 1;
    for (int d = -r; d <= r; ++d) {
      const int yy = y + d;
      int v;
      if (yy >= 0 && yy < Y) {
        const int gg = g[i + int64_t{d} * Z];
        v = gg * gg + d * d;
      } else if (outside) {
        v = d * d;
      } else {
        continue;
      }
      best = v < best ? v : best;
    }
    h[i] = static_cast<uint16_t>(best);
  }
}

// Along X: out = (min over |d| <= r of h(x + d) + d^2 <= R2) != invert.
__global__ __launch_bounds__(kBlock) void morph_x_kernel(const uint16_t* __restrict__ h, int64_t n, int X, int64_t YZ,
                                                         int r, int R2, int outside, int invert,
                                                         int16_t* __restrict__ out) {
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const int x = static_cast<int>(i / YZ);
    int best = R2 + 1;
    for (int d = -r; d <= r; ++d) {
      const int xx = x + d;
      int v;
      if (xx >= 0 && xx < X)
        v = h[i + d * YZ] + d * d;
      else if (outside)
        v = d * d;
      else
        continue;
      best = v < best ? v : best;
    }
    out[i] = ((best <= R2) != (invert != 0)) ? 1 : 0;
  }
}

// ------------------------------------------------------------------ S4
// header words of the workspace
enum { kBestKey = 0, kSecond = 1, kComponents = 2, kMaskVoxels = 3, kVoxels = 4, kFilled = 5 };

// One wave per 64 consecutive voxels: one atomic per distinct root among them.
__global__ __launch_bounds__(kBlock) void largest_sizes_kernel(const int* __restrict__ roots, int64_t n,
                                                               int* __restrict__ sizes) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t base = (int64_t{blockIdx.x} * kWavesPerBlock + threadIdx.x / kWave) * kWave; base < n;
       base += int64_t{gridDim.x} * kBlock) {
    const int64_t i = base + lane;
    const int r = i < n ? roots[i] : 0;
    wave_for_each_key(r != 0, r, [&](int key, unsigned long long same, bool mine) {
      if (mine && lane == __ffsll(static_cast<long long>(same)) - 1) atomicAdd(&sizes[key - 1], __popcll(same));
    });
  }
}

// kSecondPass = false: the winner's key, the component count and the mask's voxels; true: the largest size among the other roots.
template <bool kSecondPass>
__global__ __launch_bounds__(kBlock) void largest_select_kernel(const int* __restrict__ roots,
                                                                const int* __restrict__ sizes, int64_t n,
                                                                unsigned long long* __restrict__ header) {
  const unsigned winner = kSecondPass ? 0xFFFFFFFFu - static_cast<unsigned>(header[kBestKey] & 0xFFFFFFFFull) : 0u;
  unsigned mine[2] = {0, 0};  // components, voxels: below 2^31 in all
  unsigned long long best = 0;
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const int r = roots[i];
    if (r == 0 || r != i + 1) continue;
    const unsigned long long size = static_cast<unsigned long long>(sizes[i]);
    if (kSecondPass) {
      if (static_cast<unsigned>(r) != winner && size > best) best = size;
    } else {
      const unsigned long long key = (size << 32) | (0xFFFFFFFFull - static_cast<unsigned long long>(r));
      best = key > best ? key : best;
      ++mine[0];
      mine[1] += static_cast<unsigned>(size);
    }
  }
  best = wave_max_u64(best);
  if ((threadIdx.x & (kWave - 1)) == 0 && best) atomicMax(&header[kSecondPass ? kSecond : kBestKey], best);
  if (!kSecondPass) block_add_counters(mine, header + kComponents);
}

// stats = {components, the largest size, the second-largest size, the winner's root, the mask's voxels}
__global__ __launch_bounds__(kBlock) void largest_keep_kernel(const int* __restrict__ roots, int64_t n,
                                                              const unsigned long long* __restrict__ header,
                                                              int16_t* __restrict__ keep,
                                                              long long* __restrict__ stats) {
  const unsigned long long key = header[kBestKey];
  const int winner = key ? static_cast<int>(0xFFFFFFFFu - static_cast<unsigned>(key & 0xFFFFFFFFull)) : -1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = static_cast<long long>(header[kComponents]);
    stats[1] = static_cast<long long>(key >> 32);
    stats[2] = static_cast<long long>(header[kSecond]);
    stats[3] = key ? winner : 0;
    stats[4] = static_cast<long long>(header[kMaskVoxels]);
  }
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock)
    keep[i] = roots[i] == winner ? 1 : 0;
}

// ------------------------------------------------------------------ S5
__global__ __launch_bounds__(kBlock) void fill_complement_kernel(const int16_t* __restrict__ mask, int64_t n,
                                                                 int16_t* __restrict__ comp,
                                                                 uint8_t* __restrict__ open) {
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    comp[i] = mask[i] == 0 ? 1 : 0;
    open[i] = 0;
  }
}

// every lane that flags a root stores the same byte: no atomic is needed
__global__ __launch_bounds__(kBlock) void fill_flag_kernel(const int* __restrict__ roots, int64_t n, int X, int Y, int Z,
                                                           uint8_t* open) {
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const int r = roots[i];
    if (r == 0) continue;
    const auto [x, y, z] = split_xyz(i, Y, Z);
    if (x == 0 || x == X - 1 || y == 0 || y == Y - 1 || z == 0 || z == Z - 1) open[r - 1] = 1;
  }
}

// stats = {|B|, voxels filled}
__global__ __launch_bounds__(kBlock) void fill_apply_kernel(const int16_t* __restrict__ mask,
                                                            const int* __restrict__ roots,
                                                            const uint8_t* __restrict__ open, int64_t n,
                                                            int16_t* __restrict__ out,
                                                            unsigned long long* __restrict__ counters) {
  unsigned mine[2] = {0, 0};
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const int r = roots[i];
    const bool set = mask[i] != 0;
    const bool filled = !set && r != 0 && !open[r - 1];
    out[i] = (set || filled) ? 1 : 0;
    mine[0] += (set || filled) ? 1u : 0u;
    mine[1] += filled ? 1u : 0u;
  }
  block_add_counters(mine, counters);
}

__global__ void copy_counters_kernel(const unsigned long long* __restrict__ counters, long long* __restrict__ stats,
                                     int count) {
  if (static_cast<int>(threadIdx.x) < count) stats[threadIdx.x] = static_cast<long long>(counters[threadIdx.x]);
}

// ------------------------------------------------------------------ S6
template <typename T>
__global__ __launch_bounds__(kBlock) void apply_mask_kernel(const T* __restrict__ src, const int16_t* __restrict__ mask,
                                                            int channels, int64_t n, T* __restrict__ dst,
                                                            unsigned long long* __restrict__ count) {
  unsigned mine[1] = {0};
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const bool set = mask[i] != 0;
    mine[0] += set ? 1u : 0u;
    for (int c = 0; c < channels; ++c) dst[c * n + i] = set ? src[c * n + i] : T(0);
  }
  block_add_counters(mine, count);
}

// ------------------------------------------------------------------ host
inline bool brain_voxels(int64_t X, int64_t Y, int64_t Z, int64_t* n) { return volume_voxels(X, Y, Z, false, n); }

// workgroups of a pass over `items` at `per_block` each: the caller's count or the library's, never more than needed
inline int grid_for(int64_t items, int64_t per_block, int64_t grid_blocks) {
  return blocks_for(items, per_block, grid_blocks > 0 ? grid_blocks : kMaxGrid);
}

// header | a: int32[n] (roots; S3's bytes) | b: int32[n] (sizes; S3's shorts; S5's complement) | open: uint8[n] |
// the workspace of C1-C3
struct Layout {
  int64_t a, b, open, components, bytes;
};
inline Layout layout(int64_t X, int64_t Y, int64_t Z, int64_t n) {
  Layout l;
  l.a = kHeaderBytes;
  l.b = l.a + round256(4 * n);
  l.open = l.b + round256(4 * n);
  l.components = l.open + round256(n);
  l.bytes = l.components + gts_components_workspace(X, Y, Z);
  return l;
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_brainmask_workspace(int64_t X, int64_t Y, int64_t Z) {
  int64_t n;
  if (!gts::brain_voxels(X, Y, Z, &n)) return 0;
  return gts::layout(X, Y, Z, n).bytes;
}

extern "C" int32_t gts_brain_range(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, uint64_t* out,
                                   int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!src || !out) return GTS_ERR_NULL;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  int64_t n;
  if (!brain_voxels(X, Y, Z, &n) || !grid_blocks_ok(grid_blocks)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(out, 0, 2 * sizeof(uint64_t), st) != hipSuccess) return launch_status();
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  const int grid = grid_for(n, kBlock, grid_blocks);
  return with_scan_type(dtype, src, [&](auto* s) {
    brain_range_kernel<<<grid, kBlock, 0, st>>>(s, n, o);
    return launch_status();
  });
}

extern "C" int32_t gts_brain_histogram(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, double hi,
                                       int64_t* counts, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!src || !counts) return GTS_ERR_NULL;
  if (!scan_type_ok(dtype) || !is_finite(hi) || !(hi > 0.0)) return GTS_ERR_ARGKIND;
  int64_t n;
  if (!brain_voxels(X, Y, Z, &n) || !grid_blocks_ok(grid_blocks)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, kBins * sizeof(int64_t), st) != hipSuccess) return launch_status();
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  const int grid = grid_for(n, kBlock, grid_blocks);
  return with_scan_type(dtype, src, [&](auto* s) {
    brain_histogram_kernel<<<grid, kBlock, 0, st>>>(s, n, hi, c);
    return launch_status();
  });
}

extern "C" int32_t gts_brain_threshold(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, double t,
                                       int16_t* mask, uint64_t* count, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!src || !mask || !count) return GTS_ERR_NULL;
  if (!scan_type_ok(dtype) || !is_finite(t) || t < 0.0) return GTS_ERR_ARGKIND;
  int64_t n;
  if (!brain_voxels(X, Y, Z, &n) || !grid_blocks_ok(grid_blocks)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(count, 0, sizeof(uint64_t), st) != hipSuccess) return launch_status();
  unsigned long long* c = reinterpret_cast<unsigned long long*>(count);
  const int grid = grid_for(n, kBlock, grid_blocks);
  return with_scan_type(dtype, src, [&](auto* s) {
    brain_threshold_kernel<<<grid, kBlock, 0, st>>>(s, n, t, mask, c);
    return launch_status();
  });
}

extern "C" int32_t gts_ball_morph_i16(const int16_t* mask_in, int64_t X, int64_t Y, int64_t Z, int32_t R2,
                                      int32_t target, int32_t outside, int16_t* mask_out, void* workspace,
                                      int64_t workspace_bytes, int32_t invert, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!mask_in || !mask_out || !workspace) return GTS_ERR_NULL;
  if (R2 < 0 || R2 > kMaxR2 || (target | 1) != 1 || (outside | 1) != 1 || (invert | 1) != 1) return GTS_ERR_ARGKIND;
  int64_t n;
  if (!brain_voxels(X, Y, Z, &n) || !grid_blocks_ok(grid_blocks)) return GTS_ERR_SHAPE;
  const Layout l = layout(X, Y, Z, n);
  if (workspace_bytes < l.bytes) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  uint8_t* g = reinterpret_cast<uint8_t*>(ws + l.a);
  uint16_t* h = reinterpret_cast<uint16_t*>(ws + l.b);
  int r = 0;
  while ((r + 1) * (r + 1) <= R2) ++r;
  morph_z_kernel<<<grid_for(n, kLineTile, grid_blocks), kBlock, 0, st>>>(mask_in, n, static_cast<int>(Z), r, target,
                                                                         outside, g);
  const int grid = grid_for(n, kBlock, grid_blocks);
  morph_y_kernel<<<grid, kBlock, 0, st>>>(g, n, static_cast<int>(Y), static_cast<int>(Z), r, R2, outside, h);
  morph_x_kernel<<<grid, kBlock, 0, st>>>(h, n, static_cast<int>(X), Y * Z, r, R2, outside, invert, mask_out);
  return launch_status();
}

extern "C" int32_t gts_largest_component_i16(const int16_t* mask, int64_t X, int64_t Y, int64_t Z,
                                             int32_t connectivity, int16_t* keep_out, int64_t* stats, void* workspace,
                                             int64_t workspace_bytes, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!mask || !keep_out || !stats || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!brain_voxels(X, Y, Z, &n) || (connectivity != 6 && connectivity != 26) || !grid_blocks_ok(grid_blocks))
    return GTS_ERR_SHAPE;
  const Layout l = layout(X, Y, Z, n);
  if (workspace_bytes < l.bytes) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  unsigned long long* header = reinterpret_cast<unsigned long long*>(ws);
  int* roots = reinterpret_cast<int*>(ws + l.a);
  int* sizes = reinterpret_cast<int*>(ws + l.b);
  if (hipMemsetAsync(ws, 0, kHeaderBytes, st) != hipSuccess) return launch_status();
  if (hipMemsetAsync(sizes, 0, 4 * n, st) != hipSuccess) return launch_status();
  const int status = gts_components_roots_i16(mask, X, Y, Z, connectivity, roots, ws + l.components,
                                              l.bytes - l.components, stream);
  if (status != GTS_OK) return status;
  const int grid = grid_for(n, kBlock, grid_blocks);
  largest_sizes_kernel<<<grid, kBlock, 0, st>>>(roots, n, sizes);
  largest_select_kernel<false><<<grid, kBlock, 0, st>>>(roots, sizes, n, header);
  largest_select_kernel<true><<<grid, kBlock, 0, st>>>(roots, sizes, n, header);
  largest_keep_kernel<<<grid, kBlock, 0, st>>>(roots, n, header, keep_out, reinterpret_cast<long long*>(stats));
  return launch_status();
}

extern "C" int32_t gts_fill_holes_i16(const int16_t* mask, int64_t X, int64_t Y, int64_t Z, int16_t* mask_out,
                                      int64_t* stats, void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                                      void* stream) {
  using namespace gts;
  if (!mask || !mask_out || !stats || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!brain_voxels(X, Y, Z, &n) || !grid_blocks_ok(grid_blocks)) return GTS_ERR_SHAPE;
  const Layout l = layout(X, Y, Z, n);
  if (workspace_bytes < l.bytes) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  unsigned long long* header = reinterpret_cast<unsigned long long*>(ws);
  int* roots = reinterpret_cast<int*>(ws + l.a);
  int16_t* comp = reinterpret_cast<int16_t*>(ws + l.b);
  uint8_t* open = reinterpret_cast<uint8_t*>(ws + l.open);
  if (hipMemsetAsync(ws, 0, kHeaderBytes, st) != hipSuccess) return launch_status();
  const int grid = grid_for(n, kBlock, grid_blocks);
  fill_complement_kernel<<<grid, kBlock, 0, st>>>(mask, n, comp, open);
  const int status = gts_components_roots_i16(comp, X, Y, Z, 6, roots, ws + l.components, l.bytes - l.components, stream);
  if (status != GTS_OK) return status;
  fill_flag_kernel<<<grid, kBlock, 0, st>>>(roots, n, static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), open);
  fill_apply_kernel<<<grid, kBlock, 0, st>>>(mask, roots, open, n, mask_out, header + kVoxels);
  copy_counters_kernel<<<1, kWave, 0, st>>>(header + kVoxels, reinterpret_cast<long long*>(stats), 2);
  return launch_status();
}

extern "C" int32_t gts_apply_mask(const void* src, int32_t dtype, int64_t C, int64_t X, int64_t Y, int64_t Z,
                                  const int16_t* mask, void* dst, uint64_t* count, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!src || !mask || !dst || !count) return GTS_ERR_NULL;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  int64_t n;
  if (!brain_voxels(X, Y, Z, &n) || C < 1 || C > kMaxChannels || !grid_blocks_ok(grid_blocks)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(count, 0, sizeof(uint64_t), st) != hipSuccess) return launch_status();
  unsigned long long* c = reinterpret_cast<unsigned long long*>(count);
  const int grid = grid_for(n, kBlock, grid_blocks);
  return with_scan_type(dtype, src, [&](auto* s) {
    using T = std::remove_const_t<std::remove_pointer_t<decltype(s)>>;
    apply_mask_kernel<<<grid, kBlock, 0, st>>>(s, mask, static_cast<int>(C), n, static_cast<T*>(dst), c);
    return launch_status();
  });
}
