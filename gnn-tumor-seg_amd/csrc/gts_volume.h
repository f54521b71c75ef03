// What the kernels over a volume of three axes share, int16 labels and scan intensities alike: the workspace
// arithmetic and the volume limit of their entry points, the BraTS region rule, and the wave and workgroup idioms
// of their counting passes.  One copy of each; a new volume feature includes this instead of copying a
// neighbour.  What only the scan (intensity) kernels share is in gts_scan.h, which includes this.
#pragma once
#include "gts_common.h"

namespace gts {

// ------------------------------------------------------------------ host: workspaces, limits, grids
constexpr int64_t kHeaderBytes = 256;  // counters and cursors at the front of a workspace, cleared by one memset

inline int64_t round256(int64_t b) { return (b + 255) & ~int64_t{255}; }

// true: the kernels can index the volume, *n = X * Y * Z < 2^31 (no product overflows on the way).  An extent
// of 0 gives *n = 0 where allow_empty says so and false otherwise; a negative extent is always false.
inline bool volume_voxels(int64_t X, int64_t Y, int64_t Z, bool allow_empty, int64_t* n) {
  constexpr int64_t kLimit = int64_t{1} << 31;
  if (X < 0 || Y < 0 || Z < 0) return false;
  *n = 0;
  if (X == 0 || Y == 0 || Z == 0) return allow_empty;
  if (X >= kLimit || Y >= kLimit || Z >= kLimit || X * Y >= kLimit || X * Y * Z >= kLimit) return false;
  *n = X * Y * Z;
  return true;
}

// The kernels that work in millimetres (H3w-H5w, M1-M4, T1-T5) take the voxel spacing as integer units, each in
// [1, kMmMaxUnit] (100 mm in steps of 1e-4 mm), on extents up to kMmMaxExtent (H2's uint16 distances):
// u_a (N_a - 1) then fits an int32.  (gts_select.h's kMaxExtent and gts_scan.h's kScanMaxExtent have other reasons.)
constexpr int64_t kMmMaxExtent = 4097;
constexpr int64_t kMmMaxUnit = 1000000;
inline bool units_ok(const int64_t* units) {
  for (int a = 0; a < 3; ++a)
    if (units[a] < 1 || units[a] > kMmMaxUnit) return false;
  return true;
}

// workgroups for `items` at `per_block` each, at most `cap` (the kernel strides over the rest)
inline int blocks_for(int64_t items, int64_t per_block, int64_t cap = INT32_MAX) {
  const int64_t b = (items + per_block - 1) / per_block;
  return static_cast<int>(b < cap ? b : cap);
}

// ------------------------------------------------------------------ the three BraTS regions
// Bit r of region_bits(v): label v lies in region r, 0 whole tumour (v != 0), 1 tumour core (v in {2, 3}),
// 2 enhancing tumour (v == 3).  A label outside 0..3 is whole tumour only.
constexpr __host__ __device__ unsigned region_bits(int v) {
  return (v != 0 ? 1u : 0u) | ((v == 2 || v == 3) ? 2u : 0u) | (v == 3 ? 4u : 0u);
}
constexpr __host__ __device__ bool in_region(int v, int region) { return (region_bits(v) >> region) & 1u; }

constexpr bool region_rule_holds(int v) {
  return in_region(v, 0) == (v != 0) && in_region(v, 1) == (v == 2 || v == 3) && in_region(v, 2) == (v == 3);
}
static_assert(region_rule_holds(-1) && region_rule_holds(0) && region_rule_holds(1) && region_rule_holds(2) &&
                  region_rule_holds(3) && region_rule_holds(4),
              "bit r of region_bits is region r");

// ------------------------------------------------------------------ device: indices, waves, counters
template <typename I>
struct Xyz {
  I x, y, z;
};

// (x, y, z) of linear index i = (x * Y + y) * Z + z; I is the caller's index type, so its arithmetic stays its own
template <typename I>
__device__ __forceinline__ Xyz<I> split_xyz(I i, int Y, int Z) {
  const I z = i % static_cast<I>(Z), row = i / static_cast<I>(Z);
  return {row / static_cast<I>(Y), row % static_cast<I>(Y), z};
}

// the xor tree over the wave's lanes: v = op(v, the partner's v) at distances 32, 16, ... 1
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, kWave));
  return v;  // in every lane
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  return wave_reduce(v, [](T a, T b) { return a + b; });
}

// body(k, same, mine) once per distinct key k among the lanes that are `on`: same is the lane mask of the
// group, mine says whether the calling lane is in it.  A body then needs one atomic per group, not per lane.
// Every lane of the wave must call it; keys are taken in the order of their first lane.
template <typename Body>
__device__ __forceinline__ void wave_for_each_key(bool on, int key, Body&& body) {
  unsigned long long todo = __ballot(on);
  while (todo) {
    const int k = __shfl(key, __ffsll(static_cast<long long>(todo)) - 1, kWave);
    const bool mine = on && key == k;
    const unsigned long long same = __ballot(mine);
    body(k, same, mine);
    todo &= ~same;
  }
}

// global[c] += the sum of mine[c] over the workgroup: wave sums, LDS counters, then one global atomic per
// counter that is not zero.  Every thread of the workgroup must call it, once per kernel.
template <int N, typename Global>
__device__ __forceinline__ void block_add_counters(const unsigned (&mine)[N], Global* __restrict__ global) {
  __shared__ unsigned block_counts[N];
  if (threadIdx.x < N) block_counts[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const unsigned s = wave_sum(mine[c]);
    if ((threadIdx.x & (kWave - 1)) == 0 && s) atomicAdd(&block_counts[c], s);
  }
  __syncthreads();
  if (threadIdx.x < N && block_counts[threadIdx.x])
    atomicAdd(&global[threadIdx.x], static_cast<Global>(block_counts[threadIdx.x]));
}

// the exclusive prefix of v over the workgroup's threads and, in *total, the sum; every thread calls it
__device__ __forceinline__ int64_t block_scan_exclusive(int64_t v, int64_t* total) {
  __shared__ int64_t wave_total[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  int64_t inc = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int64_t t = __shfl_up(inc, off, kWave);
    if (lane >= off) inc += t;
  }
  if (lane == kWave - 1) wave_total[w] = inc;
  __syncthreads();
  int64_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kWavesPerBlock; ++k) {
    if (k < w) before += wave_total[k];
    all += wave_total[k];
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

}  // namespace gts
