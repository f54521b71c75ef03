// K11 kernels without matrix cores: a few outputs per row (tiny_fwd, skinny_fwd) and the ReLU mask bits of an
// output the tile kernels stored (relu_bits_kernel).  Included by gts_gemm.hip, which decides when they apply.
#pragma once
#include "gts_gemm_args.h"

namespace gts {
namespace {

// bits[((col / 64) * ceil(rows / 4) + row / 4) * 4 + e], bit 16 (row % 4) + (col % 64) / 4  <=>  c[row][64 (col / 64) + 4 ((col % 64) / 4) + e] > 0:
// the layout the panel kernels write from their epilogue, here for the outputs of the other tile variants
__global__ __launch_bounds__(256) void relu_bits_kernel(const float* __restrict__ c, unsigned long long* __restrict__ bits,
                                                        int rows, int cols) {
  const int lane = threadIdx.x & 63;
  const int blocks = cols >> 6;
  const long long id = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const long long group = id / blocks;
  const int cb = static_cast<int>(id % blocks);
  if (group * 4 >= rows) return;
  const long long row = group * 4 + (lane >> 4);
  v4f v = {0.f, 0.f, 0.f, 0.f};
  if (row < rows) v = *reinterpret_cast<const v4f*>(c + row * cols + 64 * cb + 4 * (lane & 15));
  const unsigned long long w0 = __ballot(v[0] > 0.f), w1 = __ballot(v[1] > 0.f);
  const unsigned long long w2 = __ballot(v[2] > 0.f), w3 = __ballot(v[3] > 0.f);
  const long long groups = (rows + 3) >> 2;
  if (lane < 4) bits[(cb * groups + group) * 4 + lane] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
}

// A few inputs to a few outputs per node (fc_pool of the first layer: 4 -> 4 on 60 000 rows): one lane per row,
// the row's <= 16 inputs as 16-byte loads (consecutive lanes = consecutive rows: contiguous), the weights at
// wave-uniform addresses, fused multiply-adds in reduction order.  A 128 x 64 MFMA tile would multiply zeros for
// 23 us here; this is 0.5 MB of traffic.
template <int N>
__global__ __launch_bounds__(256) void tiny_fwd_kernel(const GemmArgs p) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= p.ra) return;
  float acc[N];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] = p.bias != nullptr ? p.bias[n] : 0.f;
#pragma unroll
  for (int seg = 0; seg < 2; ++seg) {
    const float* a = p.a[seg] + static_cast<size_t>(row) * p.lda[seg];
    for (int k = 0; k < p.kseg[seg]; k += 4) {
      const v4f x = *reinterpret_cast<const v4f*>(a + k);
#pragma unroll
      for (int n = 0; n < N; ++n) {
        const v4f w = *reinterpret_cast<const v4f*>(p.b[seg] + n * p.ldb[seg] + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[n] = __builtin_fmaf(x[e], w[e], acc[n]);
      }
    }
  }
  float* out = p.c + static_cast<size_t>(row) * p.ldc;
#pragma unroll
  for (int n = 0; n < N; n += 4) {
    v4f o = {acc[n], acc[n + 1], acc[n + 2], acc[n + 3]};
    if (p.relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = relu_f32(o[e]);
    }
    *reinterpret_cast<v4f*>(out + n) = o;
  }
}

// Wide inputs to 4 or 8 outputs per node (the classifier layer: 256 + 256 -> 4; g @ W_neigh of the first layer:
// 256 -> 4): HBM-bound row streaming.  A wave takes four rows at a time; lane l holds reduction indices
// 4 l .. 4 l + 3 (+ 256 per further chunk) of each row and of every weight row, accumulates its partial dot
// products in a fixed order and the 64 partials meet in an xor butterfly — the same sum for a row whatever
// the batch holds.  (The 128 x 64 MFMA tile reads the same bytes at 3.1 TB/s: 40 us for the pair at C2.)
template <int N, bool BKC>
__global__ __launch_bounds__(256) void skinny_fwd_kernel(const GemmArgs p) {
  constexpr int R = 4;
  const int lane = threadIdx.x & 63;
  const long long wave = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const long long row0 = wave * R;
  if (row0 >= p.ra) return;
  float acc[R][N];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int n = 0; n < N; ++n) acc[r][n] = 0.f;
#pragma unroll
  for (int seg = 0; seg < 2; ++seg) {
    const int kseg = p.kseg[seg];
    for (int k = 4 * lane; k < kseg; k += 256) {
      v4f w[N];   // w[n][e] = B(n, k + e)
      if constexpr (BKC) {
#pragma unroll
        for (int n = 0; n < N; ++n) w[n] = *reinterpret_cast<const v4f*>(p.b[seg] + static_cast<size_t>(n) * p.ldb[seg] + k);
      } else {      // weights [K, N] with ldb == N: the four reduction rows of this lane are 16 N contiguous bytes
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int n4 = 0; n4 < N; n4 += 4) {
            const v4f t = *reinterpret_cast<const v4f*>(p.b[seg] + static_cast<size_t>(k + e) * p.ldb[seg] + n4);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[n4 + j][e] = t[j];
          }
      }
      v4f x[R];
#pragma unroll
      for (int r = 0; r < R; ++r)
        x[r] = row0 + r < p.ra ? *reinterpret_cast<const v4f*>(p.a[seg] + static_cast<size_t>(row0 + r) * p.lda[seg] + k)
                               : v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[r][n] = __builtin_fmaf(x[r][e], w[n][e], acc[r][n]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[r][n] += __shfl_xor(acc[r][n], o, kWave);
  // lane r * N / 4 + n / 4 stores the float4 (r, n..n+3): every lane holds every total
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int n = 0; n < N; n += 4) {
      if (lane == r * (N / 4) + n / 4 && row0 + r < p.ra) {
        v4f o = {acc[r][n], acc[r][n + 1], acc[r][n + 2], acc[r][n + 3]};
        if (p.bias != nullptr) o += *reinterpret_cast<const v4f*>(p.bias + n);
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = relu_f32(o[e]);
        }
        *reinterpret_cast<v4f*>(p.c + static_cast<size_t>(row0 + r) * p.ldc + n) = o;
      }
    }
}

}  // namespace
}  // namespace gts
