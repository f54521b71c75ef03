// U1/U1n/U2: voxel-wise uncertainty maps of the ensemble and their QU-BraTS style counts (gts/uncertainty.py,
// DESIGN.md §4u).
//
//   region_uncertainty_rows   (U1)  the three region maps (WT, CT, ET) of the class sums E1 leaves, scattered at
//                             the crop box: out[r, xs[i], ys[j], zs[k]] = u_r(sums[(i * cy + j) * cz + k, :]).
//   region_uncertainty_nodes  (U1n) the GNN-only form: out[r, v] = u_r(sums[svs[v]]), 0 for a background voxel.
//   uncertainty_histogram     (U2)  per region the counts of TP, FP, FN and TN voxels at every map value.
//
// u_r is one sequence of IEEE float64 operations (region_uncertainty below); the library is built with
// -ffp-contract=off, so none of them fuses, and the maps equal the numpy expression bit for bit.
// U1 and U1n stream: one thread per row / voxel, 16 B in and 3 B out (U1), 2 B in and 3 B out (U1n; the node
// table stays in L2).  U2 reads 7 B per voxel and counts in per-workgroup LDS tables; integer sums, so the result
// does not depend on the launch geometry or on the order of the atomics.
#include "gts_volume.h"

namespace gts {
namespace {

constexpr int kRegions = 3;
constexpr int kOutcomes = 4;                                // TP, FP, FN, TN
constexpr int kBins = GTS_UNCERTAINTY_BINS;                 // 0..100, and 101 for anything above
constexpr int kRegionWords = kOutcomes * kBins;             // 408
constexpr int kCounted = kRegions * kRegionWords;           // 1224 counters, then the bad-label counter
constexpr int kTables = kCounted + 1;                       // LDS words of a workgroup (4900 B)
static_assert(GTS_UNCERTAINTY_HIST_WORDS == (kRegions + 1) * kRegionWords, "hist is [4][4][102]");
static_assert(kTables <= GTS_UNCERTAINTY_HIST_WORDS, "the bad-label counter is hist[3][0][0]");

// u of one region: S the float64 sum of the region's class sums, t the number of terms
__device__ __forceinline__ unsigned uncertainty_of(double S, double t) {
  double p = S / t;
  if (!(p == p)) return 100u;  // NaN
  p = p < 0.0 ? 0.0 : p;
  p = p > 1.0 ? 1.0 : p;
  const double q = 1.0 - p;
  const double m = p < q ? p : q;
  return static_cast<unsigned>(static_cast<int>(rint(200.0 * m)));  // round-half-to-even, 0..100
}

// (u_WT, u_CT, u_ET) of a row of fp32 class sums s[0..3]: the classes of a region are added in ascending order
__device__ __forceinline__ void region_uncertainty(const float (&s)[4], double t, unsigned (&u)[kRegions]) {
  const double d1 = static_cast<double>(s[1]), d2 = static_cast<double>(s[2]), d3 = static_cast<double>(s[3]);
  u[0] = uncertainty_of((d1 + d2) + d3, t);
  u[1] = uncertainty_of(d2 + d3, t);
  u[2] = uncertainty_of(d3, t);
}

struct UncBox {
  const int32_t* xs;
  const int32_t* ys;
  const int32_t* zs;
  int cx, cy, cz;    // cropped extents
  int dim_y, dim_z;  // full extents of the two inner axes
  int64_t n_vol;     // voxels of the full volume: the stride between two region maps
};

template <bool WIDE>  // WIDE: sums 16-byte aligned
__global__ __launch_bounds__(kBlock) void region_uncertainty_rows_kernel(const float* __restrict__ sums,
                                                                         uint8_t* __restrict__ out, UncBox box,
                                                                         double terms) {
  // the crop has fewer than 2^31 rows (the entry point refuses more), so the row index and its split into
  // (i, j, k) stay 32-bit: two 32-bit divisions per row instead of 64-bit ones; t + the stride (< 2^21) cannot wrap
  const unsigned n_crop = static_cast<unsigned>(box.cx) * box.cy * box.cz;
  for (unsigned t = blockIdx.x * kBlock + threadIdx.x; t < n_crop; t += gridDim.x * kBlock) {
    const float* row = sums + 4 * static_cast<int64_t>(t);
    float s[4];
    if constexpr (WIDE) {
      const Vec<4> v = Vec<4>::load_nt(row);
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = v.v[c];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = row[c];
    }
    unsigned u[kRegions];
    region_uncertainty(s, terms, u);
    const Xyz<unsigned> ijk = split_xyz<unsigned>(t, box.cy, box.cz);
    const int64_t at =
        (static_cast<int64_t>(box.xs[ijk.x]) * box.dim_y + box.ys[ijk.y]) * box.dim_z + box.zs[ijk.z];
#pragma unroll
    for (int r = 0; r < kRegions; ++r) out[r * box.n_vol + at] = static_cast<uint8_t>(u[r]);
  }
}

template <bool WIDE>  // WIDE: sums 16-byte aligned
__global__ __launch_bounds__(kBlock) void region_uncertainty_nodes_kernel(const int16_t* __restrict__ svs,
                                                                          const float* __restrict__ sums,
                                                                          uint8_t* __restrict__ out, int64_t n_vox,
                                                                          int n_rows, double terms) {
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; v < n_vox;
       v += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int r = resolve_row(svs[v], n_rows);
    unsigned u[kRegions] = {0u, 0u, 0u};  // background voxels are healthy and certain
    if (r != n_rows) {
      float s[4];
      if constexpr (WIDE) {
        const float4 row = reinterpret_cast<const float4*>(sums)[r];
        s[0] = row.x, s[1] = row.y, s[2] = row.z, s[3] = row.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = sums[4 * static_cast<int64_t>(r) + c];
      }
      region_uncertainty(s, terms, u);
    }
#pragma unroll
    for (int g = 0; g < kRegions; ++g) out[g * n_vox + v] = static_cast<uint8_t>(u[g]);
  }
}

// One voxel into the tables.  Every lane of the wave calls it (`on` false: nothing to count).  Nearly every voxel
// of a scan is healthy on both sides with u = 0 in all three regions; those would make a wave's lanes hit the
// same three LDS words, so they are counted per wave (ballot + popcount into `quiet`, the same value in every
// lane) and only the others go through LDS atomics.
__device__ __forceinline__ void count_voxel(bool on, int p, int g, unsigned u0, unsigned u1, unsigned u2,
                                            unsigned* __restrict__ tables, unsigned& quiet) {
  const bool bad = on && (static_cast<unsigned>(p) > 3u || static_cast<unsigned>(g) > 3u);
  const bool calm = on && !bad && (p | g) == 0 && (u0 | u1 | u2) == 0u;
  quiet += static_cast<unsigned>(__popcll(__ballot(calm)));
  if (bad) atomicAdd(&tables[kCounted], 1u);
  if (on && !bad && !calm) {
    const unsigned pb = region_bits(p), gb = region_bits(g);
    const unsigned u[kRegions] = {u0, u1, u2};
#pragma unroll
    for (int r = 0; r < kRegions; ++r) {
      const unsigned outcome = ((pb >> r) & 1u ? 0u : 2u) + ((gb >> r) & 1u ? 0u : 1u);  // TP, FP, FN, TN
      const unsigned bin = u[r] > 100u ? 101u : u[r];
      atomicAdd(&tables[r * kRegionWords + outcome * kBins + bin], 1u);
    }
  }
}

// hist[c] += the counts of this workgroup's share of the n voxels.  Both loops run a wave-uniform number of
// times (the bound is on the wave's first item), so `quiet` stays the same in every lane.
__global__ __launch_bounds__(kBlock) void uncertainty_histogram_kernel(const int16_t* __restrict__ pred,
                                                                       const int16_t* __restrict__ truth,
                                                                       const uint8_t* __restrict__ unc,
                                                                       unsigned long long* __restrict__ hist,
                                                                       int64_t n, int vector_ok) {
  __shared__ unsigned tables[kTables];
  for (int c = threadIdx.x; c < kTables; c += kBlock) tables[c] = 0u;
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave_first = static_cast<int64_t>(blockIdx.x) * kBlock + (threadIdx.x - lane);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  unsigned quiet = 0u;

  const int64_t n_groups = vector_ok ? n / 8 : 0;  // groups of 8 voxels: 16 B of each label array, 8 B of each map
  for (int64_t g0 = wave_first; g0 < n_groups; g0 += stride) {
    const int64_t g = g0 + lane;
    const bool on = g < n_groups;
    uint4 p = make_uint4(0u, 0u, 0u, 0u), t = p;
    uint2 m[kRegions] = {make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u)};
    if (on) {
      p = reinterpret_cast<const uint4*>(pred)[g];
      t = reinterpret_cast<const uint4*>(truth)[g];
#pragma unroll
      for (int r = 0; r < kRegions; ++r) m[r] = *reinterpret_cast<const uint2*>(unc + r * n + 8 * g);
    }
    const unsigned pw[4] = {p.x, p.y, p.z, p.w}, tw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int sh16 = (e & 1) * 16, sh8 = (e & 3) * 8;
      const int pv = static_cast<int16_t>((pw[e >> 1] >> sh16) & 0xffffu);
      const int tv = static_cast<int16_t>((tw[e >> 1] >> sh16) & 0xffffu);
      const unsigned u0 = ((e < 4 ? m[0].x : m[0].y) >> sh8) & 0xffu;
      const unsigned u1 = ((e < 4 ? m[1].x : m[1].y) >> sh8) & 0xffu;
      const unsigned u2 = ((e < 4 ? m[2].x : m[2].y) >> sh8) & 0xffu;
      count_voxel(on, pv, tv, u0, u1, u2, tables, quiet);
    }
  }
  // one voxel per lane: everything, when the groups above do not apply (a pointer or n not aligned for them)
  for (int64_t i0 = n_groups * 8 + wave_first; i0 < n; i0 += stride) {
    const int64_t i = i0 + lane;
    const bool on = i < n;
    int pv = 0, tv = 0;
    unsigned u0 = 0u, u1 = 0u, u2 = 0u;
    if (on) pv = pred[i], tv = truth[i], u0 = unc[i], u1 = unc[n + i], u2 = unc[2 * n + i];
    count_voxel(on, pv, tv, u0, u1, u2, tables, quiet);
  }
  if (lane == 0 && quiet) {
#pragma unroll
    for (int r = 0; r < kRegions; ++r) atomicAdd(&tables[r * kRegionWords + 3 * kBins], quiet);  // TN at u = 0
  }
  __syncthreads();
  for (int c = threadIdx.x; c < kTables; c += kBlock) {
    const unsigned v = tables[c];
    if (v) atomicAdd(&hist[c], static_cast<unsigned long long>(v));
  }
}

constexpr int64_t kMaxVoxels = INT64_C(1) << 40;
constexpr int kMaxHistogramGroups = 2048;
// The tables are 32-bit.  Fewer than kMaxHistogramGroups workgroups are launched only when each has at most 8192
// voxels; otherwise a workgroup's share is about n / kMaxHistogramGroups, below 2^32 for every n allowed.
static_assert(kMaxVoxels / kMaxHistogramGroups + 8 * kBlock < (INT64_C(1) << 32), "a share fits its counters");

inline unsigned histogram_groups(int64_t n) {
  // 32 voxels per thread before a second workgroup pays for its flush; all of them when n is large
  const int64_t per_block = static_cast<int64_t>(kBlock) * 32;
  const int64_t blocks = (n + per_block - 1) / per_block;
  return static_cast<unsigned>(blocks > kMaxHistogramGroups ? kMaxHistogramGroups : blocks);
}

inline unsigned row_grid(int64_t rows) {
  const int64_t blocks = (rows + kBlock - 1) / kBlock;
  return static_cast<unsigned>(blocks > 8192 ? 8192 : blocks);
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_region_uncertainty_rows_u8(const float* sums, const int32_t* xs, const int32_t* ys,
                                                  const int32_t* zs, uint8_t* out, int64_t cx, int64_t cy,
                                                  int64_t cz, int64_t dim_x, int64_t dim_y, int64_t dim_z,
                                                  int64_t n_classes, int64_t terms, void* stream) {
  using namespace gts;
  if (cx < 0 || cy < 0 || cz < 0 || dim_x < 1 || dim_y < 1 || dim_z < 1 || dim_x > 32768 || dim_y > 32768 ||
      dim_z > 32768 || cx > dim_x || cy > dim_y || cz > dim_z || n_classes != 4 || terms < 1 ||
      terms > (INT64_C(1) << 31))
    return GTS_ERR_SHAPE;
  const int64_t n_crop = cx * cy * cz;
  if (n_crop >= (INT64_C(1) << 31)) return GTS_ERR_SHAPE;  // the kernel's row arithmetic is 32-bit
  if (n_crop == 0) return GTS_OK;
  if (!sums || !xs || !ys || !zs || !out) return GTS_ERR_NULL;
  const UncBox box{xs, ys, zs, static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(cz),
                   static_cast<int>(dim_y), static_cast<int>(dim_z), dim_x * dim_y * dim_z};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double t = static_cast<double>(terms);
  if ((reinterpret_cast<uintptr_t>(sums) & 15) == 0)
    region_uncertainty_rows_kernel<true><<<row_grid(n_crop), kBlock, 0, st>>>(sums, out, box, t);
  else
    region_uncertainty_rows_kernel<false><<<row_grid(n_crop), kBlock, 0, st>>>(sums, out, box, t);
  return launch_status();
}

extern "C" int32_t gts_region_uncertainty_nodes_u8(const int16_t* svs, const float* sums, uint8_t* out,
                                                   int64_t n_vox, int64_t n_rows, int64_t n_classes, int64_t terms,
                                                   void* stream) {
  using namespace gts;
  if (n_vox < 0 || n_vox > kMaxVoxels || n_rows < 0 || n_rows > 32768 || n_classes != 4 || terms < 1 ||
      terms > (INT64_C(1) << 31))
    return GTS_ERR_SHAPE;
  if (n_vox == 0) return GTS_OK;
  if (!svs || !out || (n_rows > 0 && !sums)) return GTS_ERR_NULL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double t = static_cast<double>(terms);
  if ((reinterpret_cast<uintptr_t>(sums) & 15) == 0)
    region_uncertainty_nodes_kernel<true><<<row_grid(n_vox), kBlock, 0, st>>>(svs, sums, out, n_vox,
                                                                              static_cast<int>(n_rows), t);
  else
    region_uncertainty_nodes_kernel<false><<<row_grid(n_vox), kBlock, 0, st>>>(svs, sums, out, n_vox,
                                                                               static_cast<int>(n_rows), t);
  return launch_status();
}

extern "C" int32_t gts_uncertainty_histogram(const int16_t* pred, const int16_t* truth, const uint8_t* unc,
                                             int64_t* hist, int64_t n, void* stream) {
  using namespace gts;
  if (n < 0 || n > kMaxVoxels) return GTS_ERR_SHAPE;
  if (n == 0) return GTS_OK;
  if (!pred || !truth || !unc || !hist) return GTS_ERR_NULL;
  // 16-byte groups of the label arrays and 8-byte groups of each of the three maps (which lie n bytes apart)
  const int vector_ok = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(truth)) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(unc) & 7) == 0 && (n & 7) == 0;
  uncertainty_histogram_kernel<<<histogram_groups(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      pred, truth, unc, reinterpret_cast<unsigned long long*>(hist), n, vector_ok);
  return launch_status();
}
