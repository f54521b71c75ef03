// The skinny weight-gradient kernels (tiny N or K) and the fixed-order sum of their chunk partials.  Included by
// gts_gemm_wgrad.h, whose launcher decides when they apply, and by gts_narrow.hip, whose fused first-layer pass writes the
// same partials and finishes them with the same skinny_sum_kernel.
#pragma once
#include "gts_gemm_args.h"

namespace gts {
namespace {

// ---- skinny weight gradients -------------------------------------------------------------------
// When one side of gw[N,K] is tiny (the 4 input channels of the first layer, the 4 classes of the
// last), a 128-row MFMA tile would be >95 % padding and the problem is a stream anyway:
//   P[i, j] = sum_m skinny[m, i] * wide[m, j],   i < S <= 9,  j < w (multiple of 4)
// one 16-byte column group of `wide` per thread, S float4 accumulators, row chunks -> per-chunk
// partials -> fixed-order chunk sum (same determinism as the slab path).  With ones_row the last
// P row is sum_m wide[m, :] (the bias gradient when `wide` is g).
constexpr int kSkinnyMax = 9;
constexpr int kSkinnyChunks = 512;

template <int S>
__global__ __launch_bounds__(kBlock) void skinny_wgrad_kernel(const float* __restrict__ skinny, int s_cols,
                                                             const float* __restrict__ wide,
                                                             float* __restrict__ partial, int64_t m,
                                                             int w, int64_t rows_per_chunk) {
  // 256 threads = (w/4 column groups) x (row lanes): with w = 256 four lanes walk interleaved rows
  // of the chunk and are combined through LDS in lane order before the partial is written.
  __shared__ v4f red[kBlock];
  const int cols4 = w >> 2;
  const int lanes = cols4 >= kBlock ? 1 : kBlock / cols4;
  const int rl = cols4 >= kBlock ? 0 : threadIdx.x / cols4;
  const int64_t row0 = blockIdx.x * rows_per_chunk, row1 = min(m, row0 + rows_per_chunk);
  for (int q0 = 0; q0 < cols4; q0 += kBlock) {
    const int q = q0 + (cols4 >= kBlock ? threadIdx.x : threadIdx.x % cols4);
    const bool live = q < cols4 && rl < lanes;
    v4f acc[S];
#pragma unroll
    for (int i = 0; i < S; ++i) acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
    if (live) {
#pragma unroll 4
      for (int64_t row = row0 + rl; row < row1; row += lanes) {
        const v4f f = *reinterpret_cast<const v4f*>(wide + static_cast<size_t>(row) * w + 4 * q);
#pragma unroll
        for (int i = 0; i < S; ++i) acc[i] += (i < s_cols ? skinny[row * s_cols + i] : 1.0f) * f;
      }
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
      v4f total = acc[i];
      if (lanes > 1) {
        __syncthreads();
        red[threadIdx.x] = acc[i];
        __syncthreads();
        if (rl == 0 && live) {
          for (int l = 1; l < lanes; ++l) total += red[l * cols4 + q];
        }
      }
      if (rl == 0 && live)
        *reinterpret_cast<v4f*>(partial + (static_cast<size_t>(blockIdx.x) * S + i) * w + 4 * q) = total;
    }
  }
}

// out = sum over chunks of partial[chunk][rows*w]; element (i, j) goes to dst0[i*w + j] (direct) or
// dst0[j*s_cols + i] (transposed) for i < s_cols, and row s_cols (the ones row) to dst1[j].
// 16 outputs x 16 chunk lanes per workgroup; lane totals are added in lane order (deterministic).
__global__ __launch_bounds__(kBlock) void skinny_sum_kernel(const float* __restrict__ partial,
                                                           float* __restrict__ dst0,
                                                           float* __restrict__ dst1, int rows, int s_cols,
                                                           int w, int chunks, int transposed) {
  __shared__ float part[16][16];
  const int o = threadIdx.x & 15, lane = threadIdx.x >> 4;
  const int idx = blockIdx.x * 16 + o;
  const int total_out = rows * w;
  float acc = 0.f;
  if (idx < total_out) {
#pragma unroll 8   // independent loads, issued back to back (the adds keep their order)
    for (int c = lane; c < chunks; c += 16) acc += partial[static_cast<size_t>(c) * total_out + idx];
  }
  part[lane][o] = acc;
  __syncthreads();
  if (lane != 0 || idx >= total_out) return;
  float sum = part[0][o];
#pragma unroll
  for (int l = 1; l < 16; ++l) sum += part[l][o];
  const int i = idx / w, j = idx - i * w;
  if (i < s_cols)
    dst0[transposed ? j * s_cols + i : i * w + j] = sum;
  else if (dst1 != nullptr)
    dst1[j] = sum;
}

}  // namespace
}  // namespace gts
