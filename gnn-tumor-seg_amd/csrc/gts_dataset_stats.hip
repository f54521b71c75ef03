// D1-D3: one scan's share of DataPreprocessor.compute_dataset_stats (scripts/preprocess_dataset.py:93-115)
// on the device:
//
//   healthy = np.logical_and(img[:, :, :, 0] > 0.001, lab == 0)      # over the WHOLE volume, no crop
//   img     = normalize_img(img[healthy], is_flat=True)              # x / q995_c (image_processing.py:45-51)
//   mu, sigma = np.mean(img, axis=0), np.std(img, axis=0)
//
// Source: the four volumes as I1-I3 take them, [4][Z][Y][X] (x fastest), int16 or float32, and the label
// volume [Z][Y][X] int16 in raw BraTS coding.
//
//   D1  membership float32(ch0) > float32(0.001) && label == 0 as a bit mask, one 64-bit word per wave
//       (__ballot; wave w of the grid-stride loop always covers voxels 64 k .. 64 k + 63), the member count
//       and the number of members with a non-finite value in some channel (integer atomics);
//   D2  I2's radix select (gts_select.h) with the mask as element source;
//   D3  per channel the sums of y = float32(x) / top_c (IEEE float32 division) and of y * y over the members,
//       accumulated in float64.  The volume is cut into units of kUnit voxels; a workgroup sums a unit in a
//       fixed pattern (thread t takes voxels t, t + 256, ... of the unit in ascending order, then a xor-shuffle
//       tree per wave, then the four waves in order) and writes one partial per unit; a one-block kernel adds
//       the partials in a fixed pattern.  Which workgroup takes which unit is the only thing the grid size
//       decides, so the sums have the same bits for every grid size and on every run.  No float atomics.
//       y * y is exact in float64 (24 + 24 significand bits), so the one-pass variance
//       sum(y^2) / n - mean^2 only pays the cancellation of the final subtraction.
#include "gts_select.h"

namespace gts {
namespace {

constexpr int kUnit = 8192;                           // voxels per D3 partial: 32 per thread
constexpr int kSums = 2 * kChannels;                  // sum y [4], sum y^2 [4]
constexpr int kFinalGroups = kBlock / kSums;          // threads that share one of the 8 sums in the final kernel

struct StatsLayout {
  int64_t mask, partial, total;
  int64_t words, units;
};

inline StatsLayout stats_layout(int64_t vol) {
  StatsLayout l;
  l.words = (vol + 63) / 64;
  l.units = (vol + kUnit - 1) / kUnit;
  l.mask = kLayout.total;                             // after the select's histogram and state, 8-byte aligned
  l.partial = l.mask + l.words * 8;
  l.total = l.partial + l.units * kSums * 8;
  return l;
}

// D1.
template <typename T>
__global__ __launch_bounds__(kBlock) void dstats_mask_kernel(const T* __restrict__ src,
                                                             const int16_t* __restrict__ lab, unsigned vol,
                                                             unsigned long long* __restrict__ bits,
                                                             unsigned long long* __restrict__ counts) {
  const unsigned padded = (vol + 63u) & ~63u;         // whole waves: every lane of a wave takes the same trips
  unsigned mine[2] = {0, 0};  // members, members with a non-finite value
  for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < padded; i += gridDim.x * kBlock) {
    bool member = false;
    if (i < vol) {
      member = load_f32(src, i) > 0.001f && lab[i] == 0;
      if (member) {
        bool finite = true;
#pragma unroll
        for (int c = 0; c < kChannels; ++c) finite &= __builtin_isfinite(load_f32(src, static_cast<size_t>(c) * vol + i));
        mine[1] += finite ? 0u : 1u;
      }
    }
    const unsigned long long word = __ballot(member);
    if ((threadIdx.x & (kWave - 1)) == 0) bits[i >> 6] = word;
    mine[0] += member ? 1u : 0u;
  }
  block_add_counters(mine, counts);
}

struct Tops {
  float top[kChannels];
};

// D3, partials: partial[unit][0..3] = sum y_c, [4..7] = sum y_c^2 over the unit's members.
template <typename T>
__global__ __launch_bounds__(kBlock) void dstats_moments_kernel(const T* __restrict__ src, unsigned vol,
                                                                const unsigned long long* __restrict__ bits,
                                                                unsigned words, Tops p, unsigned units,
                                                                double* __restrict__ partial) {
  __shared__ double red[kWavesPerBlock][kSums];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
    double acc[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) acc[j] = 0.0;
    const unsigned base = u * kUnit;
    for (int k = 0; k < kUnit / kBlock; ++k) {
      const unsigned i = base + k * kBlock + threadIdx.x;      // i >> 6 is the same for the whole wave
      const unsigned w = i >> 6;
      const unsigned long long word = w < words ? bits[w] : 0ull;
      if (word == 0ull) continue;
      if ((word >> lane) & 1ull) {                            // a set bit implies i < vol (D1 sets none beyond)
#pragma unroll
        for (int c = 0; c < kChannels; ++c) {
          const float y = load_f32(src, static_cast<size_t>(c) * vol + i) / p.top[c];
          const double yd = static_cast<double>(y);
          acc[c] += yd;
          acc[kChannels + c] += yd * yd;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kSums; ++j) acc[j] = wave_sum(acc[j]);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < kSums; ++j) red[wave][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
      double s = red[0][threadIdx.x];
      for (int w = 1; w < kWavesPerBlock; ++w) s += red[w][threadIdx.x];
      partial[static_cast<size_t>(u) * kSums + threadIdx.x] = s;
    }
    __syncthreads();
  }
}

// D3, final: out[0..3] = sum y, [4..7] = sum y^2, [8..11] = mean, [12..15] = standard deviation (ddof 0).
__global__ __launch_bounds__(kBlock) void dstats_final_kernel(const double* __restrict__ partial, unsigned units,
                                                              unsigned long long n, double* __restrict__ out) {
  __shared__ double red[kFinalGroups][kSums];
  __shared__ double total[kSums];
  const unsigned j = threadIdx.x % kSums, g = threadIdx.x / kSums;
  double s = 0.0;
  for (unsigned u = g; u < units; u += kFinalGroups) s += partial[static_cast<size_t>(u) * kSums + j];
  red[g][j] = s;
  __syncthreads();
  if (threadIdx.x < kSums) {
    double t = red[0][threadIdx.x];
    for (int k = 1; k < kFinalGroups; ++k) t += red[k][threadIdx.x];
    total[threadIdx.x] = t;
    out[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x < kChannels) {
    const double count = static_cast<double>(n);
    const double mean = total[threadIdx.x] / count;
    const double var = total[kChannels + threadIdx.x] / count - mean * mean;
    out[kSums + threadIdx.x] = mean;
    out[kSums + kChannels + threadIdx.x] = sqrt(var > 0.0 ? var : 0.0);
  }
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_dataset_stats_workspace(int64_t X, int64_t Y, int64_t Z) {
  using namespace gts;
  if (!volume_ok(X, Y, Z)) return GTS_ERR_SHAPE;
  return stats_layout(X * Y * Z).total;
}

extern "C" int32_t gts_dataset_stats_mask(const void* src, int32_t dtype, const int16_t* labels, int64_t X, int64_t Y,
                                          int64_t Z, uint64_t* counts, void* workspace, int64_t workspace_bytes,
                                          void* stream) {
  using namespace gts;
  if (!src || !labels || !counts || !workspace) return GTS_ERR_NULL;
  if (!volume_ok(X, Y, Z)) return GTS_ERR_SHAPE;
  const int64_t vol = X * Y * Z;
  const StatsLayout l = stats_layout(vol);
  if (workspace_bytes < l.total) return GTS_ERR_SHAPE;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, 16, st) != hipSuccess) return launch_status();
  auto* bits = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + l.mask);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const int grid = blocks_for(vol, kBlock, kMaxBlocks);
  return with_scan_type(dtype, src, [&](auto* s) {
    dstats_mask_kernel<<<grid, kBlock, 0, st>>>(s, labels, static_cast<unsigned>(vol), bits, cnt);
    return launch_status();
  });
}

extern "C" int32_t gts_dataset_stats_order_stats(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                                                 int64_t n, int64_t rank_lo, int64_t rank_hi, float* out,
                                                 void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!src || !out || !workspace) return GTS_ERR_NULL;
  if (!volume_ok(X, Y, Z)) return GTS_ERR_SHAPE;
  const int64_t vol = X * Y * Z;
  const StatsLayout l = stats_layout(vol);
  if (workspace_bytes < l.total || n < 1 || n > vol) return GTS_ERR_SHAPE;
  if (rank_lo < 0 || rank_hi < rank_lo || rank_hi >= n) return GTS_ERR_SHAPE;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const MaskSource source{reinterpret_cast<const unsigned long long*>(static_cast<char*>(workspace) + l.mask)};
  return with_scan_type(dtype, src, [&](auto* s) {
    run_select(s, static_cast<size_t>(vol), source, vol, rank_lo, rank_hi, out, workspace, st);
    return launch_status();
  });
}

extern "C" int32_t gts_dataset_stats_moments(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                                             int64_t n, const float* top, double* out, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!src || !top || !out || !workspace) return GTS_ERR_NULL;
  if (!volume_ok(X, Y, Z)) return GTS_ERR_SHAPE;
  const int64_t vol = X * Y * Z;
  const StatsLayout l = stats_layout(vol);
  if (workspace_bytes < l.total || n < 1 || n > vol) return GTS_ERR_SHAPE;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  Tops p;
  for (int c = 0; c < kChannels; ++c) p.top[c] = top[c];
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  const auto* bits = reinterpret_cast<const unsigned long long*>(ws + l.mask);
  double* partial = reinterpret_cast<double*>(ws + l.partial);
  const unsigned units = static_cast<unsigned>(l.units), words = static_cast<unsigned>(l.words);
  return with_scan_type(dtype, src, [&](auto* s) {
    dstats_moments_kernel<<<blocks_for(l.units, 1, kMaxBlocks), kBlock, 0, st>>>(s, static_cast<unsigned>(vol), bits, words,
                                                                                 p, units, partial);
    dstats_final_kernel<<<1, kBlock, 0, st>>>(partial, units, static_cast<unsigned long long>(n), out);
    return launch_status();
  });
}
