// The 4-wide first layer of a SAGEConv('pool') stack, backward: ONE pass over g [m, 256] (the gradient w.r.t. the
// layer's pre-activation output) where the stack used to stream it three times.
//
// Replaces, for w = 256 and s0 = s1 = 4, three launches of the layer-0 backward (/root/reference/model/networks.py:25-30,
// SAGEConv(in_feats, 256, 'pool') under autograd):
//   gm       = g @ W_neigh                  skinny_fwd_kernel<4, false>   (gts_linear_bwd_input_f32)
//   gw_self  = g^T x, g_bias = g^T 1        skinny_wgrad_kernel<5>        (gts_linear_bwd_weight_f32, problem with bias)
//   gw_neigh = g^T m0                       skinny_wgrad_kernel<4>        (gts_linear_bwd_weight_f32)
// with the SAME BITS: every thread keeps the arithmetic of the kernel it stands for.
//   * lanes: at w = 256 both kernels give lane l the columns 4 l .. 4 l + 3 of a row;
//   * rows: skinny_wgrad_kernel's walk (chunks of ceil(m / 512) rows, wave rl takes rows row0 + rl, step 4), the same
//     `acc += s * f` per row, the same combine of the four waves through LDS in wave order, the same [chunk][row][w]
//     partials, finished by the unchanged skinny_sum_kernel;
//   * dot products: per row the four fmaf chains over e = 0..3 from 0 of skinny_fwd_kernel at K = 256 (one k-step per
//     lane), then its xor butterfly 32..1.  A row's total does not depend on the wave that holds the row.  The butterfly
//     is run as a halving exchange: IEEE addition commutes, so lane i and lane i ^ o hold the same sum after a step and only
//     one of them needs to form it — after step 32 a lane carries two of the four totals, after step 16 one (7 exchanges
//     and 7 additions per row where the butterfly of four values has 24 of each; same tree, same roundings).
#include "gts_gemm_skinny.h"

namespace gts {
namespace {

constexpr int kFirstW = 256, kFirstS = 4;

__global__ __launch_bounds__(kBlock) void first_layer_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                const float* __restrict__ m0,
                                                                const float* __restrict__ w_neigh, float* __restrict__ gm,
                                                                float* __restrict__ part_x, float* __restrict__ part_m,
                                                                int64_t m, int64_t rows_per_chunk) {
  constexpr int W = kFirstW, S = kFirstS;
  __shared__ v4f red[kWavesPerBlock - 1][2 * S + 1][kWave];
  const int lane = threadIdx.x & (kWave - 1), rl = threadIdx.x / kWave;
  const int64_t row0 = blockIdx.x * rows_per_chunk, row1 = min(m, row0 + rows_per_chunk);
  // wn[n][e] = W_neigh[4 lane + e][n]: the four reduction rows of this lane are 64 contiguous bytes of the stored [256, 4]
  v4f wn[S];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const v4f t = *reinterpret_cast<const v4f*>(w_neigh + static_cast<size_t>(4 * lane + e) * S);
#pragma unroll
    for (int j = 0; j < S; ++j) wn[j][e] = t[j];
  }
  v4f ax[S + 1], am[S];
#pragma unroll
  for (int i = 0; i <= S; ++i) ax[i] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < S; ++i) am[i] = v4f{0.f, 0.f, 0.f, 0.f};
  const bool upper32 = (lane & 32) != 0, upper16 = (lane & 16) != 0;
  // one row: what skinny_wgrad_kernel<5>, skinny_wgrad_kernel<4> and skinny_fwd_kernel<4, false> do with it
  auto take_row = [&](int64_t row, const v4f f, const v4f xs, const v4f ms) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < S; ++i) ax[i] += xs[i] * f;
    ax[S] += 1.0f * f;   // the ones row: the bias gradient
#pragma unroll
    for (int i = 0; i < S; ++i) am[i] += ms[i] * f;
    float d[S];
#pragma unroll
    for (int n = 0; n < S; ++n) {
      d[n] = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[n] = __builtin_fmaf(f[e], wn[n][e], d[n]);
    }
    // step 32: the lower half keeps totals 0 and 1, the upper half 2 and 3; step 16 halves again; then one value per lane
    const float keep0 = upper32 ? d[2] : d[0], keep1 = upper32 ? d[3] : d[1];
    const float send0 = upper32 ? d[0] : d[2], send1 = upper32 ? d[1] : d[3];
    const float a = keep0 + __shfl_xor(send0, 32, kWave), b = keep1 + __shfl_xor(send1, 32, kWave);
    float c = (upper16 ? b : a) + __shfl_xor(upper16 ? a : b, 16, kWave);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
    if ((lane & 15) == 0) gm[static_cast<size_t>(row) * S + (lane >> 4)] = c;   // lanes 0 / 16 / 32 / 48 hold totals 0..3
  };
  // the wave's rows row0 + rl, + 4, ... in order, four at a time with their loads issued together (a row past the chunk
  // re-reads the first one and is not taken)
  constexpr int kAhead = 4;
  for (int64_t first = row0 + rl; first < row1; first += kAhead * kWavesPerBlock) {
    v4f f[kAhead], xs[kAhead], ms[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int64_t row = first + u * kWavesPerBlock < row1 ? first + u * kWavesPerBlock : first;
      f[u] = *reinterpret_cast<const v4f*>(g + static_cast<size_t>(row) * W + 4 * lane);
      xs[u] = *reinterpret_cast<const v4f*>(x + static_cast<size_t>(row) * S);
      ms[u] = *reinterpret_cast<const v4f*>(m0 + static_cast<size_t>(row) * S);
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
      if (first + u * kWavesPerBlock < row1) take_row(first + u * kWavesPerBlock, f[u], xs[u], ms[u]);
  }
  if (rl > 0) {
#pragma unroll
    for (int i = 0; i <= S; ++i) red[rl - 1][i][lane] = ax[i];
#pragma unroll
    for (int i = 0; i < S; ++i) red[rl - 1][S + 1 + i][lane] = am[i];
  }
  __syncthreads();
  if (rl != 0) return;
#pragma unroll
  for (int i = 0; i <= S; ++i) {
    v4f total = ax[i];
    for (int l = 1; l < kWavesPerBlock; ++l) total += red[l - 1][i][lane];
    *reinterpret_cast<v4f*>(part_x + (static_cast<size_t>(blockIdx.x) * (S + 1) + i) * W + 4 * lane) = total;
  }
#pragma unroll
  for (int i = 0; i < S; ++i) {
    v4f total = am[i];
    for (int l = 1; l < kWavesPerBlock; ++l) total += red[l - 1][S + 1 + i][lane];
    *reinterpret_cast<v4f*>(part_m + (static_cast<size_t>(blockIdx.x) * S + i) * W + 4 * lane) = total;
  }
}

inline bool first_layer_shape(int64_t m, int64_t w, int64_t s0, int64_t s1) {
  return m > 0 && m < (1LL << 31) && w == kFirstW && s0 == kFirstS && s1 == kFirstS;
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_sage_first_layer_bwd_workspace(int64_t m, int64_t w, int64_t s0, int64_t s1) {
  using namespace gts;
  if (!first_layer_shape(m, w, s0, s1)) return 0;
  return static_cast<int64_t>(kSkinnyChunks) * (s0 + 1 + s1) * w * static_cast<int64_t>(sizeof(float));
}

extern "C" int32_t gts_sage_first_layer_bwd_f32(const float* g, const float* x, const float* m0, const float* w_neigh,
                                                float* gm, float* gw_self, float* g_bias, float* gw_neigh,
                                                float* workspace, int64_t workspace_bytes, int64_t m, int64_t w,
                                                int64_t s0, int64_t s1, void* stream) {
  using namespace gts;
  if (!g || !x || !m0 || !w_neigh || !gm || !gw_self || !g_bias || !gw_neigh || !workspace) return GTS_ERR_NULL;
  if (!first_layer_shape(m, w, s0, s1)) return GTS_ERR_SHAPE;
  if (workspace_bytes < gts_sage_first_layer_bwd_workspace(m, w, s0, s1)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the chunks of skinny_wgrad (gts_gemm_wgrad.h)
  const int64_t rpc = (m + kSkinnyChunks - 1) / kSkinnyChunks;
  const int chunks = static_cast<int>((m + rpc - 1) / rpc);
  const int W = kFirstW, S = kFirstS;
  float* part_x = workspace;
  float* part_m = workspace + static_cast<size_t>(chunks) * (S + 1) * W;
  first_layer_bwd_kernel<<<chunks, kBlock, 0, st>>>(g, x, m0, w_neigh, gm, part_x, part_m, m, rpc);
  skinny_sum_kernel<<<((S + 1) * W + 15) / 16, kBlock, 0, st>>>(part_x, gw_self, g_bias, S + 1, S, W, chunks, 1);
  skinny_sum_kernel<<<(S * W + 15) / 16, kBlock, 0, st>>>(part_m, gw_neigh, nullptr, S, S, W, chunks, 1);
  return launch_status();
}
