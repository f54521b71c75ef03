// R1/R2: co-register the modalities of a study that lie on different grids (no counterpart in
// the reference, which reads studies that the BraTS organisers registered already).
//
// Both kernels sample a MOVING volume ([Z][Y][X], x fastest, int16 or float32, on its own grid) at the points a
// 3 x 4 float64 matrix T sends the voxel indices (x, y, z) of another grid to:
//   u = ((T00 x + T01 y) + T02 z) + T03, v and w likewise from rows 1 and 2: float64, nothing contracted;
//   inside  <=>  0 <= u <= X-1 && 0 <= v <= Y-1 && 0 <= w <= Z-1 (a NaN coordinate fails every comparison: outside);
//   i0 = min(floor(u), X-1), i1 = min(i0 + 1, X-1), t = u - i0 per axis; the eight neighbours through
//   gts_scan.h's trilinear8 (float64, along x, then y, then z; t == 0 returns the voxel itself).
//
//   R1 gts_affine_resample   out[z][y][x] = float32(that value), 0.0f outside.  One value per lane, and two maps
//        of lanes to voxels that compute the same bits:
//          plain  lane = output voxel in linear order.  Neighbouring lanes read input addresses that step by
//                 (T00, T10, T20): coalesced when the output's x runs along the input's x (|T00| dominant), and
//                 correct for every T;
//          tiled  |T10| or |T20| dominant: the output's x runs along the input's y or z, and the output axis
//                 ka with the larger |T0ka| runs along the input's x.  A 64 x 64 tile over (output x, output ka):
//                 computing, a wave's lanes run along ka (input rows); the values cross a padded LDS tile;
//                 storing, the lanes run along output x (gts_scan.h's cross_tile64).
//   R2 gts_joint_histogram   for every voxel of a FIXED float32 volume with x, y, z all multiples of `stride`
//        and each of K matrices: the moving value m (float64, not rounded), then one count in row k of an int64
//        table [K][B*B + 1]: entry B*B when the sample is outside, entry bin(f) * B + bin(m) otherwise.
//        bin(v) = 0 when v is not finite (NaN and +-Inf), else q = floor((v - lo) *
//        scale), q >= 1 ? (q < B-1 ? int(q) : B-1) : 0 (a NaN q fails q >= 1: bin 0).
//        Counts are integers, summed in LDS (uint32, one B*B table per matrix) and flushed with one 64-bit
//        integer global atomic per non-zero cell and workgroup: no float atomics, no dependence on the grid or
//        on arrival order.  The fixed value and its bin are read once for all K matrices.  Contention: most
//        voxels of a head scan are background and share one cell, so a wave first counts, by a ballot, the
//        lanes whose cell equals its first active lane's and adds that count once; only the other lanes add
//        one by one.  16384 cells (64 KiB) per pass: 64 matrices at B = 16, 16 at B = 32, 4 at B = 64; more
//        matrices than that take further passes over the fixed volume.
#include <math.h>
#include <stddef.h>

#include <algorithm>

#include "gts_scan.h"

namespace gts {
namespace {

constexpr int kMaxMatrices = 16;
constexpr int kPassCells = 16384;                                            // uint32 cells of one pass's tables
constexpr int kHistLdsBytes = (kPassCells + kMaxMatrices) * 4;               // + one outside counter per matrix
constexpr int kMaxLdsPerCu = 160 * 1024;
constexpr int kPathAuto = 0, kPathPlain = 1, kPathTiled = 2;

struct Coord {
  double u, v, w;
};

// T is row-major 3 x 4
__device__ __forceinline__ Coord transform(const double (&T)[12], int x, int y, int z) {
  const double xd = x, yd = y, zd = z;
  return {((T[0] * xd + T[1] * yd) + T[2] * zd) + T[3], ((T[4] * xd + T[5] * yd) + T[6] * zd) + T[7],
          ((T[8] * xd + T[9] * yd) + T[10] * zd) + T[11]};
}

__device__ __forceinline__ bool inside(const Coord& c, int X, int Y, int Z) {
  return c.u >= 0.0 && c.u <= static_cast<double>(X - 1) && c.v >= 0.0 && c.v <= static_cast<double>(Y - 1) &&
         c.w >= 0.0 && c.w <= static_cast<double>(Z - 1);
}

// The trilinear value at an INSIDE coordinate: every index below lies in the volume because inside() held.
template <typename In>
__device__ __forceinline__ double sample(const In* __restrict__ vol, int X, int Y, int Z, const Coord& c) {
  const int x0 = min(static_cast<int>(c.u), X - 1), x1 = min(x0 + 1, X - 1);   // u >= 0: the cast is the floor
  const int y0 = min(static_cast<int>(c.v), Y - 1), y1 = min(y0 + 1, Y - 1);
  const int z0 = min(static_cast<int>(c.w), Z - 1), z1 = min(z0 + 1, Z - 1);
  const double tx = c.u - static_cast<double>(x0), ty = c.v - static_cast<double>(y0), tz = c.w - static_cast<double>(z0);
  return trilinear8(vol, X, Y, x0, x1, y0, y1, z0, z1, tx, ty, tz);
}

// ------------------------------------------------------------------ R1
struct ResampleArgs {
  double T[12];
  int in[3];   // X, Y, Z
  int out[3];  // OX, OY, OZ
};

template <typename In>
__device__ __forceinline__ float resampled(const In* __restrict__ src, const ResampleArgs& p, int ox, int oy, int oz) {
  const Coord c = transform(p.T, ox, oy, oz);
  if (!inside(c, p.in[0], p.in[1], p.in[2])) return 0.0f;
  return static_cast<float>(sample(src, p.in[0], p.in[1], p.in[2], c));
}

template <typename In>
__global__ __launch_bounds__(kBlock) void resample_plain_kernel(const In* __restrict__ src, float* __restrict__ dst,
                                                                const ResampleArgs p, int64_t total) {
  const int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  if (i >= total) return;
  const int ox = static_cast<int>(i % p.out[0]);
  const int64_t row = i / p.out[0];
  dst[i] = resampled(src, p, ox, static_cast<int>(row % p.out[1]), static_cast<int>(row / p.out[1]));
}

// Block = one 64 x 64 tile over (output x, output axis ka) at one coordinate of the third output axis.
template <typename In>
__global__ __launch_bounds__(kBlock) void resample_tiled_kernel(const In* __restrict__ src, float* __restrict__ dst,
                                                                const ResampleArgs p, int ka, int tiles_x, int tiles_a) {
  int64_t b = blockIdx.x;
  const int tx0 = static_cast<int>(b % tiles_x) * kTile;
  b /= tiles_x;
  const int ta0 = static_cast<int>(b % tiles_a) * kTile;
  const int ob = static_cast<int>(b / tiles_a);
  cross_tile64<float>(
      tx0, ta0, p.out[0], ka == 1 ? p.out[1] : p.out[2],
      [&](int ox, int oa) { return resampled(src, p, ox, ka == 1 ? oa : ob, ka == 1 ? ob : oa); },
      [&](int ox, int oa, float v) {
        const int oy = ka == 1 ? oa : ob, oz = ka == 1 ? ob : oa;
        dst[(static_cast<int64_t>(oz) * p.out[1] + oy) * p.out[0] + ox] = v;
      });
}

template <typename In>
int launch_resample(const In* s, float* dst, const ResampleArgs& p, int path, hipStream_t st) {
  const double ax = fabs(p.T[0]), ay = fabs(p.T[4]), az = fabs(p.T[8]);
  const bool x_leads = ax >= ay && ax >= az;   // neighbouring output voxels along x step along the input's x
  if (path == kPathPlain || (path == kPathAuto && x_leads)) {
    const int64_t total = int64_t{p.out[0]} * p.out[1] * p.out[2];
    resample_plain_kernel<In><<<blocks_for(total, kBlock), kBlock, 0, st>>>(s, dst, p, total);
    return launch_status();
  }
  const int ka = fabs(p.T[2]) > fabs(p.T[1]) ? 2 : 1, kb = 3 - ka;   // the output axis that runs along the input's x
  const int tiles_x = (p.out[0] + kTile - 1) / kTile, tiles_a = (p.out[ka] + kTile - 1) / kTile;
  const int64_t blocks = int64_t{tiles_x} * tiles_a * p.out[kb];     // <= OX OY OZ < 2^31
  resample_tiled_kernel<In><<<static_cast<unsigned>(blocks), kBlock, 0, st>>>(s, dst, p, ka, tiles_x, tiles_a);
  return launch_status();
}

// ------------------------------------------------------------------ R2
struct HistArgs {
  double T[kMaxMatrices * 12];  // read with kernarg_entry: the struct is the kernel's only argument
  const float* fixed;
  const void* moving;
  unsigned long long* counts;   // row 0 of this pass
  int64_t total;                // strided samples
  int in[3];                    // moving X, Y, Z
  int fix[3];                   // fixed FX, FY, FZ
  int nsx, nsy;                 // strided samples along x and y
  int stride, bins, K;
  double lo_f, scale_f, lo_m, scale_m;
};

__device__ __forceinline__ int bin_of(double v, double lo, double scale, int bins) {
  if (!is_finite(v)) return 0;
  const double q = floor((v - lo) * scale);
  return q >= 1.0 ? (q < static_cast<double>(bins - 1) ? static_cast<int>(q) : bins - 1) : 0;
}

template <typename In>
__global__ __launch_bounds__(kBlock) void joint_histogram_kernel(const HistArgs p) {
  extern __shared__ unsigned lds[];
  const int cells_per = p.bins * p.bins, n_cells = p.K * cells_per;
  unsigned* cells = lds;
  unsigned* outside = lds + n_cells;  // [K]
  for (int i = threadIdx.x; i < n_cells + p.K; i += kBlock) lds[i] = 0;
  __syncthreads();
  const In* __restrict__ moving = static_cast<const In*>(p.moving);
  const int lane = threadIdx.x & (kWave - 1);
  // every lane of a wave runs every iteration and every k, so the ballots below see the whole wave
  for (int64_t base = int64_t{blockIdx.x} * kBlock; base < p.total; base += int64_t{gridDim.x} * kBlock) {
    const int64_t i = base + threadIdx.x;
    const bool on = i < p.total;
    int x = 0, y = 0, z = 0, bf = 0;
    if (on) {
      x = static_cast<int>(i % p.nsx) * p.stride;
      const int64_t row = i / p.nsx;
      y = static_cast<int>(row % p.nsy) * p.stride;
      z = static_cast<int>(row / p.nsy) * p.stride;
      const float f = p.fixed[(static_cast<int64_t>(z) * p.fix[1] + y) * p.fix[0] + x];
      bf = bin_of(static_cast<double>(f), p.lo_f, p.scale_f, p.bins);
    }
    for (int k = 0; k < p.K; ++k) {
      double T[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) T[j] = kernarg_entry<double>(offsetof(HistArgs, T), k * 12 + j);
      const Coord c = transform(T, x, y, z);
      const bool in = on && inside(c, p.in[0], p.in[1], p.in[2]);
      int cell = 0;
      if (in) cell = bf * p.bins + bin_of(sample(moving, p.in[0], p.in[1], p.in[2], c), p.lo_m, p.scale_m, p.bins);
      const unsigned long long out_lanes = __ballot(on && !in);
      if (lane == 0 && out_lanes) atomicAdd(&outside[k], static_cast<unsigned>(__popcll(out_lanes)));
      const unsigned long long in_lanes = __ballot(in);
      if (in_lanes) {
        const int lead = __ffsll(static_cast<long long>(in_lanes)) - 1;
        const int lead_cell = __shfl(cell, lead, kWave);
        const bool same = in && cell == lead_cell;
        const unsigned long long same_lanes = __ballot(same);
        unsigned* table = cells + k * cells_per;
        if (lane == lead) atomicAdd(&table[lead_cell], static_cast<unsigned>(__popcll(same_lanes)));
        if (in && !same) atomicAdd(&table[cell], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_cells; i += kBlock) {
    const unsigned n = cells[i];
    if (n) {
      const int k = i / cells_per;
      atomicAdd(&p.counts[static_cast<int64_t>(k) * (cells_per + 1) + (i - k * cells_per)], static_cast<unsigned long long>(n));
    }
  }
  if (threadIdx.x < p.K && outside[threadIdx.x])
    atomicAdd(&p.counts[static_cast<int64_t>(threadIdx.x) * (cells_per + 1) + cells_per],
              static_cast<unsigned long long>(outside[threadIdx.x]));
}

int device_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      n <= 0)
    n = 256;
  return n;
}

template <typename In>
int launch_histogram(const In* moving, HistArgs p, const double* matrices, int K, int64_t grid_blocks, hipStream_t st) {
  p.moving = moving;
  static const hipError_t allowed = hipFuncSetAttribute(reinterpret_cast<const void*>(&joint_histogram_kernel<In>),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, kHistLdsBytes);
  if (allowed != hipSuccess) return static_cast<int>(allowed);
  const int cells_per = p.bins * p.bins;
  const int per_pass = std::min(kMaxMatrices, kPassCells / cells_per);
  unsigned long long* counts = p.counts;
  for (int k0 = 0; k0 < K; k0 += per_pass) {
    p.K = std::min(per_pass, K - k0);
    for (int j = 0; j < p.K * 12; ++j) p.T[j] = matrices[k0 * 12 + j];
    p.counts = counts + static_cast<int64_t>(k0) * (cells_per + 1);
    const int lds_bytes = (p.K * cells_per + p.K) * 4;
    int64_t blocks = grid_blocks;
    if (blocks <= 0) {  // as many workgroups as stay resident: each one flushes its tables once
      const int per_cu = std::max(1, std::min(8, kMaxLdsPerCu / lds_bytes));
      blocks = blocks_for(p.total, kBlock, int64_t{device_cus()} * per_cu);
    }
    joint_histogram_kernel<In><<<static_cast<unsigned>(blocks), kBlock, lds_bytes, st>>>(p);
    const int status = launch_status();
    if (status != GTS_OK) return status;
  }
  return GTS_OK;
}

bool finite_all(const double* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!is_finite(v[i])) return false;
  return true;
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_affine_resample(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, const double* matrix,
                                       int64_t OX, int64_t OY, int64_t OZ, float* dst, int32_t path, void* stream) {
  using namespace gts;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  if (path != kPathAuto && path != kPathPlain && path != kPathTiled) return GTS_ERR_ARGKIND;
  if (!src || !dst || !matrix) return GTS_ERR_NULL;
  if (!scan_extents_ok(X, Y, Z) || !scan_extents_ok(OX, OY, OZ)) return GTS_ERR_SHAPE;
  const int64_t in_dims[3] = {X, Y, Z}, out_dims[3] = {OX, OY, OZ};
  if (!finite_all(matrix, 12)) return GTS_ERR_ARGKIND;
  ResampleArgs p;
  for (int j = 0; j < 12; ++j) p.T[j] = matrix[j];
  for (int k = 0; k < 3; ++k) {
    p.in[k] = static_cast<int>(in_dims[k]);
    p.out[k] = static_cast<int>(out_dims[k]);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  return with_scan_type(dtype, src, [&](auto* s) { return launch_resample(s, dst, p, path, st); });
}

extern "C" int32_t gts_joint_histogram(const float* fixed, int64_t FX, int64_t FY, int64_t FZ, const void* moving,
                                       int32_t dtype, int64_t X, int64_t Y, int64_t Z, const double* matrices, int64_t K,
                                       int64_t stride, int64_t bins, double lo_f, double scale_f, double lo_m,
                                       double scale_m, int64_t* counts, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  if (bins != 16 && bins != 32 && bins != 64) return GTS_ERR_ARGKIND;
  if (!fixed || !moving || !matrices || !counts) return GTS_ERR_NULL;
  if (K < 1 || K > kMaxMatrices || stride < 1 || !grid_blocks_ok(grid_blocks)) return GTS_ERR_SHAPE;
  if (!scan_extents_ok(X, Y, Z) || !scan_extents_ok(FX, FY, FZ)) return GTS_ERR_SHAPE;
  const int64_t in_dims[3] = {X, Y, Z}, fix_dims[3] = {FX, FY, FZ};
  const double ranges[4] = {lo_f, scale_f, lo_m, scale_m};
  if (!finite_all(matrices, K * 12) || !finite_all(ranges, 4)) return GTS_ERR_ARGKIND;
  HistArgs p;
  p.fixed = fixed;
  p.counts = reinterpret_cast<unsigned long long*>(counts);
  for (int k = 0; k < 3; ++k) {
    p.in[k] = static_cast<int>(in_dims[k]);
    p.fix[k] = static_cast<int>(fix_dims[k]);
  }
  const int64_t s = stride < kScanMaxExtent ? stride : kScanMaxExtent;  // a stride beyond every extent samples index 0 only
  p.stride = static_cast<int>(s);
  p.nsx = static_cast<int>((FX + s - 1) / s);
  p.nsy = static_cast<int>((FY + s - 1) / s);
  p.total = int64_t{p.nsx} * p.nsy * ((FZ + s - 1) / s);
  p.bins = static_cast<int>(bins);
  p.K = 0;
  p.lo_f = lo_f, p.scale_f = scale_f, p.lo_m = lo_m, p.scale_m = scale_m;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t cleared = hipMemsetAsync(counts, 0, static_cast<size_t>(K) * (bins * bins + 1) * sizeof(int64_t), st);
  if (cleared != hipSuccess) return static_cast<int>(cleared);
  return with_scan_type(dtype, moving, [&](auto* m) {
    return launch_histogram(m, p, matrices, static_cast<int>(K), grid_blocks, st);
  });
}
