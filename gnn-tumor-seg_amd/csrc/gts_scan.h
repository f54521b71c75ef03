// What the kernels over a scan (intensity) volume share, on top of gts_volume.h: the NIfTI dtype codes and the
// two-armed launch over them, the extent limit of the resampling entry points, the finiteness test, THE trilinear
// sampler (conform, co-registration), the 64 x 64 LDS tile crossing of their tiled kernels and the two halves of
// a workgroup's LDS histogram.  One copy of each; a new scan feature includes this instead of copying a neighbour.
#pragma once
#include "gts_volume.h"

namespace gts {

// ------------------------------------------------------------------ host: dtypes, limits
constexpr int32_t kI16 = 4, kF32 = 16;  // NIfTI datatype codes: what a scan volume may hold

constexpr bool scan_type_ok(int32_t dtype) { return dtype == kI16 || dtype == kF32; }

// f(typed src) for the dtype's element type, GTS_ERR_ARGKIND for any other code.  An entry point that reports
// another error between its dtype check and its launch keeps scan_type_ok in that place.
template <typename F>
int with_scan_type(int32_t dtype, const void* src, F&& f) {
  if (dtype == kI16) return f(static_cast<const int16_t*>(src));
  if (dtype == kF32) return f(static_cast<const float*>(src));
  return GTS_ERR_ARGKIND;
}

// What include/gts_hip.h promises for conform, co-registration and bias correction: every extent in 1 ..
// kScanMaxExtent and fewer than 2^31 voxels.  (The 4096 of gts_select.h and HD95's limit have their own reasons.)
constexpr int64_t kScanMaxExtent = 65535;

constexpr bool scan_extent_ok(int64_t n) { return n >= 1 && n <= kScanMaxExtent; }

inline bool scan_extents_ok(int64_t X, int64_t Y, int64_t Z) {
  int64_t n;
  return scan_extent_ok(X) && scan_extent_ok(Y) && scan_extent_ok(Z) && volume_voxels(X, Y, Z, false, &n);
}

// a caller's grid_blocks: 0 leaves the choice to the library
constexpr bool grid_blocks_ok(int64_t grid_blocks) { return grid_blocks >= 0 && grid_blocks <= INT32_MAX; }

// false for NaN, +Inf and -Inf
template <typename T>
constexpr __host__ __device__ bool is_finite(T v) {
  static_assert(static_cast<T>(0.5) != T(0), "a floating-point type");
  return v - v == T(0);
}

// ------------------------------------------------------------------ device: the trilinear sampler
// A sample that lies on a voxel (t == 0) IS that voxel: the sign of a -0.0 survives and a non-finite neighbour
// that carries no weight does not turn the result into a NaN.  For finite values a + (b - a) * 0 is a anyway.
__device__ __forceinline__ double lerp64(double a, double b, double t) { return t == 0.0 ? a : a + (b - a) * t; }

// The eight neighbours (x0 | x1, y0 | y1, z0 | z1, all inside vol[Z][Y][X]) as float64, lerped along x, then y,
// then z with the weights of the second index; the library is built without contraction.  The bits of every
// resampled voxel come from here: how a caller gets its indices and weights is its own business.
template <typename In>
__device__ __forceinline__ double trilinear8(const In* __restrict__ vol, int X, int Y, int x0, int x1, int y0, int y1,
                                             int z0, int z1, double tx, double ty, double tz) {
  const In* r00 = vol + (static_cast<int64_t>(z0) * Y + y0) * X;
  const In* r01 = vol + (static_cast<int64_t>(z0) * Y + y1) * X;
  const In* r10 = vol + (static_cast<int64_t>(z1) * Y + y0) * X;
  const In* r11 = vol + (static_cast<int64_t>(z1) * Y + y1) * X;
  const double v00 = lerp64(static_cast<double>(r00[x0]), static_cast<double>(r00[x1]), tx);
  const double v01 = lerp64(static_cast<double>(r01[x0]), static_cast<double>(r01[x1]), tx);
  const double v10 = lerp64(static_cast<double>(r10[x0]), static_cast<double>(r10[x1]), tx);
  const double v11 = lerp64(static_cast<double>(r11[x0]), static_cast<double>(r11[x1]), tx);
  return lerp64(lerp64(v00, v01, ty), lerp64(v10, v11, ty), tz);
}

// ------------------------------------------------------------------ device: the tile crossing
// A resampling kernel whose output x reads the input's y or z: the reads of neighbouring voxels along the
// INPUT's x are the coalesced ones, the writes along the OUTPUT's x.  A workgroup of kBlock threads takes a
// 64 x 64 tile over (output x, the output axis a that runs along the input's x) starting at (tx0, ta0):
//   value(ox, oa)      with a wave's lanes along a, the result through LDS;
//   store(ox, oa, w)   with the lanes along x.
// LDS holds one 32-bit Word per value with a pitch of 65 words, 16640 bytes: the row writes and the column reads
// (ds_write_b32 / ds_read_b32, 32 banks per 32-lane group) both touch 32 distinct banks.  Every thread of the
// workgroup must call it, once per kernel.
constexpr int kTile = 64;
constexpr int kPitch = kTile + 1;

template <typename Word, typename Value, typename Store>
__device__ __forceinline__ void cross_tile64(int tx0, int ta0, int OX, int OA, Value&& value, Store&& store) {
  static_assert(sizeof(Word) == 4, "the bank arithmetic is for 32-bit words");
  __shared__ Word tile[kTile * kPitch];
  const int lane = threadIdx.x & (kTile - 1), wave_row = threadIdx.x / kTile;
  {
    const int oa = ta0 + lane;
    for (int r = wave_row; r < kTile; r += kBlock / kTile) {
      const int ox = tx0 + r;
      if (oa < OA && ox < OX) tile[r * kPitch + lane] = value(ox, oa);
    }
  }
  __syncthreads();
  {
    const int ox = tx0 + lane;
    for (int r = wave_row; r < kTile; r += kBlock / kTile) {
      const int oa = ta0 + r;
      if (oa < OA && ox < OX) store(ox, oa, tile[lane * kPitch + r]);
    }
  }
}

// ------------------------------------------------------------------ device: a workgroup's LDS histogram
// hist[0 .. n) = 0, visible to the workgroup
__device__ __forceinline__ void block_hist_clear(unsigned* hist, int n) {
  for (int i = threadIdx.x; i < n; i += kBlock) hist[i] = 0;
  __syncthreads();
}

// counts[i] += hist[i] once the workgroup has finished counting: one 64-bit atomic per bin that is not empty
__device__ __forceinline__ void block_hist_flush(const unsigned* hist, int n, unsigned long long* __restrict__ counts) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += kBlock)
    if (hist[i]) atomicAdd(&counts[i], static_cast<unsigned long long>(hist[i]));
}

}  // namespace gts
