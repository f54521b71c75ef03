// Exact order statistics of four-channel scan values: the 4-pass, 8-bit radix select that I2
// (gts_intake.hip, elements named by three crop index lists) and D2 (gts_dataset_stats.hip, elements named
// by a voxel bit mask) share.  The element source is a template parameter of the histogram kernel; the
// select state, the step kernel and the workspace layout are the same for both.
#pragma once
#include "gts_scan.h"

namespace gts {
namespace {

constexpr int kChannels = 4;
constexpr int kMaxExtent = 4096;   // LDS flag arrays of I1
constexpr int kMaxBlocks = 2048;
constexpr int kBins = 256;
constexpr int kHist = kChannels * 2 * kBins;   // [channel][rank][bin]

struct SelectState {
  unsigned prefix[kChannels][2];
  unsigned long long rank[kChannels][2];   // rank still to skip inside the current prefix
};

struct Layout {
  int64_t hist, state, total;
};
constexpr Layout kLayout = {0, kHist * 4, kHist * 4 + 256};

// Order-preserving key of a float32; -0.0 is mapped to +0.0 first, so that the two zeros form one
// value (np.partition does not order them; a rank that lands on zeros returns +0.0).
__device__ __forceinline__ unsigned float_key(float v) {
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

template <typename T>
__device__ __forceinline__ float load_f32(const T* __restrict__ p, size_t i) {
  return static_cast<float>(p[i]);
}

// Voxel offset of cropped element (xi, yi, zi); an index outside the volume reads voxel 0 instead of
// leaving the buffer (the host builds the lists from I1's flags, so this never happens there).
__device__ __forceinline__ unsigned crop_offset(const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                                                const int32_t* __restrict__ zs, unsigned xi, unsigned yi, unsigned zi,
                                                int X, int Y, int Z) {
  const unsigned x = static_cast<unsigned>(xs[xi]), y = static_cast<unsigned>(ys[yi]),
                 z = static_cast<unsigned>(zs[zi]);
  if (x >= unsigned(X) || y >= unsigned(Y) || z >= unsigned(Z)) return 0;
  return (z * Y + y) * X + x;
}

// Element sources of the histogram kernel: locate(e, off) says whether element e of [0, n) takes part
// and gives its voxel offset.
struct CropSource {   // I2: element e of the np.ix_ region, x fastest; every element takes part
  const int32_t* __restrict__ xs;
  const int32_t* __restrict__ ys;
  const int32_t* __restrict__ zs;
  int cx, cy, X, Y, Z;
  __device__ __forceinline__ bool locate(unsigned e, unsigned& off) const {
    const unsigned xi = e % cx, r = e / cx;
    off = crop_offset(xs, ys, zs, xi, r % cy, r / cy, X, Y, Z);
    return true;
  }
};

struct MaskSource {   // D2: element e is voxel e; it takes part when its bit is set (64 voxels per word)
  const unsigned long long* __restrict__ bits;
  __device__ __forceinline__ bool locate(unsigned e, unsigned& off) const {
    off = e;
    return (bits[e >> 6] >> (e & 63)) & 1ull;
  }
};

__global__ void intake_select_init_kernel(unsigned* __restrict__ hist, SelectState* __restrict__ st,
                                          unsigned long long rank_lo, unsigned long long rank_hi) {
  for (int i = threadIdx.x; i < kHist; i += blockDim.x) hist[i] = 0;
  if (threadIdx.x < 2 * kChannels) {
    const int c = threadIdx.x >> 1, r = threadIdx.x & 1;
    st->prefix[c][r] = 0;
    st->rank[c][r] = r ? rank_hi : rank_lo;
  }
}

// One pass: histogram of digit (key >> shift) & 255 over the elements whose higher digits equal
// the rank's prefix.
template <typename T, typename Source>
__global__ __launch_bounds__(kBlock) void intake_hist_kernel(const T* __restrict__ src, size_t vol, Source source,
                                                             unsigned n, const SelectState* __restrict__ st,
                                                             unsigned* __restrict__ hist, int shift) {
  __shared__ unsigned h[kHist];
  for (int i = threadIdx.x; i < kHist; i += kBlock) h[i] = 0;
  const unsigned hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
  unsigned p0[kChannels], p1[kChannels];
  bool both[kChannels];
#pragma unroll
  for (int c = 0; c < kChannels; ++c) {
    p0[c] = st->prefix[c][0];
    p1[c] = st->prefix[c][1];
    both[c] = p0[c] != p1[c];
  }
  __syncthreads();
  for (unsigned e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
    unsigned off;
    if (!source.locate(e, off)) continue;
#pragma unroll
    for (int c = 0; c < kChannels; ++c) {
      const unsigned key = float_key(load_f32(src, c * vol + off));
      const unsigned d = (key >> shift) & (kBins - 1);
      if (((key ^ p0[c]) & hi_mask) == 0) atomicAdd(&h[(2 * c) * kBins + d], 1u);
      if (both[c] && ((key ^ p1[c]) & hi_mask) == 0) atomicAdd(&h[(2 * c + 1) * kBins + d], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHist; i += kBlock)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

// One step: each (channel, rank) walks its histogram to the bin that holds its rank, appends the
// digit to its prefix, and the histogram is cleared for the next pass.  After the last pass the
// prefix is the key of the order statistic.
__global__ __launch_bounds__(kBlock) void intake_select_step_kernel(unsigned* __restrict__ hist,
                                                                    SelectState* __restrict__ st, int shift,
                                                                    float* __restrict__ out) {
  const int t = threadIdx.x;
  unsigned prefix = 0, digit = kBins - 1;
  unsigned long long k = 0;
  if (t < 2 * kChannels) {
    const int c = t >> 1, r = t & 1;
    const bool shared_hist = st->prefix[c][0] == st->prefix[c][1];
    const unsigned* h = hist + (2 * c + (shared_hist ? 0 : r)) * kBins;
    prefix = st->prefix[c][r];
    k = st->rank[c][r];
    unsigned long long acc = 0;
    for (int b = 0; b < kBins; ++b) {
      if (k < acc + h[b]) {
        digit = b;
        break;
      }
      acc += h[b];
    }
    k -= acc;
    prefix |= digit << shift;
  }
  __syncthreads();  // every walk has read the prefixes and the histograms
  if (t < 2 * kChannels) {
    st->prefix[t >> 1][t & 1] = prefix;
    st->rank[t >> 1][t & 1] = k;
    if (out) out[t] = key_float(prefix);
  }
  for (int i = t; i < kHist; i += kBlock) hist[i] = 0;
}

inline bool volume_ok(int64_t X, int64_t Y, int64_t Z) {
  return X >= 1 && Y >= 1 && Z >= 1 && X <= kMaxExtent && Y <= kMaxExtent && Z <= kMaxExtent &&
         X * Y * Z < (int64_t{1} << 31);
}

// The four passes over n elements of `source`; out (device float32 [4][2]) is written by the last step.
template <typename T, typename Source>
inline void run_select(const T* src, size_t vol, const Source& source, int64_t n, int64_t rank_lo, int64_t rank_hi,
                       float* out, void* workspace, hipStream_t st) {
  char* ws = static_cast<char*>(workspace);
  unsigned* hist = reinterpret_cast<unsigned*>(ws + kLayout.hist);
  SelectState* state = reinterpret_cast<SelectState*>(ws + kLayout.state);
  const int grid = blocks_for(n, kBlock, kMaxBlocks);
  intake_select_init_kernel<<<1, kBlock, 0, st>>>(hist, state, static_cast<unsigned long long>(rank_lo),
                                                  static_cast<unsigned long long>(rank_hi));
  for (int shift = 24; shift >= 0; shift -= 8) {
    intake_hist_kernel<T, Source><<<grid, kBlock, 0, st>>>(src, vol, source, static_cast<unsigned>(n), state, hist,
                                                            shift);
    intake_select_step_kernel<<<1, kBlock, 0, st>>>(hist, state, shift, shift == 0 ? out : nullptr);
  }
}

}  // namespace
}  // namespace gts
