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
//
// Further down, the other narrow end: the 256 -> 4 top layer of a training step, whose two 256-wide inputs ONE pass reads once for the
// classifier, the loss, its gradient and the layer's narrow weight gradients (gts_sage_top_layer_train_f32).
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

// ---- the 256 -> 4 top layer of a training step: ONE pass over h [m, 256] (the layer's input) and mx [m, 256] (its max-pooled
// neighbours) where the step used to stream both twice.  Replaces, with the SAME BITS,
//   logits = h Wself^T + mx Wneigh^T + b       skinny_fwd_kernel<4, true>            (gts_linear_fwd_f32)
//   gu, loss terms                             weighted_ce_kernel<4>                 (gts_weighted_ce_f32)
//   g = gu / den                               torch's div_ by the denominator
//   gw_self = g^T h, gw_neigh = g^T mx         skinny_wgrad_kernel<4> twice          (gts_linear_bwd_weight_f32)
//   g_bias = g^T 1                             skinny_wgrad_kernel<1> at w = 4
// and their finishes (weighted_ce_finish_kernel, skinny_sum_kernel three times) by one launch.  Four launches for twelve:
// top_den_kernel, top_layer_train_kernel, top_loss_kernel, top_finish_kernel.
//   * rows and lanes: the walk of skinny_wgrad_kernel at w = 256, as in first_layer_bwd_kernel above; lane l holds the columns
//     4 l .. 4 l + 3 of both rows, which are also the reduction indices skinny_fwd_kernel gives it;
//   * logits: that kernel's fmaf chain over the h segment, then over the mx segment, its butterfly (run as the halving
//     exchange of first_layer_bwd_kernel), then the bias;
//   * loss: four rows of a wave at a time, row u in the lanes with (lane & 3) == u, the statements of weighted_ce_kernel<4>;
//   * the denominator depends on the labels alone: top_den_kernel writes weighted_ce_kernel's block partials of it first and
//     every workgroup here adds them as weighted_ce_finish_kernel does;
//   * the column sums of g keep skinny_wgrad_kernel<1>'s order at w = 4: thread t of a chunk adds the rows row0 + t,
//     + 256, ... (here: slot t of an LDS table, filled in that order by the one wave that meets those rows), thread 0 then
//     adds the 256 threads' sums in thread order.  A slot no row reaches holds +0, and no sum here can be -0, so the tail of
//     zeros is not added.
constexpr int kTopK = 256, kTopC = 4;
constexpr int kCeRowsPerThread = 4, kCeRows = kBlock * kCeRowsPerThread;   // weighted_ce_kernel's partition (gts_loss.hip)

// class weight of a label as weighted_ce_kernel reads it: 0 for a label outside [0, C)
__device__ __forceinline__ float top_label_weight(long long label, const float* __restrict__ class_w, bool* valid, int* y) {
  *valid = label >= 0 && label < kTopC;
  *y = *valid ? static_cast<int>(label) : 0;
  return !*valid ? 0.0f : (class_w != nullptr ? class_w[*y] : 1.0f);
}

// ce_part[2 b + 1] = weighted_ce_kernel's denominator partial of its block b
__global__ __launch_bounds__(kBlock) void top_den_kernel(const int64_t* __restrict__ labels, const float* __restrict__ class_w,
                                                        float* __restrict__ ce_part, int64_t n) {
  __shared__ float red[kWavesPerBlock];
  float den = 0.f;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * kCeRowsPerThread;
  for (int r = 0; r < kCeRowsPerThread; ++r) {
    const int64_t i = base + r;
    if (i >= n) break;
    bool valid;
    int y;
    den += top_label_weight(labels[i], class_w, &valid, &y);
  }
  for (int s = kWave / 2; s >= 1; s >>= 1) den += __shfl_xor(den, s, kWave);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) red[wave] = den;
  __syncthreads();
  if (threadIdx.x == 0) ce_part[2 * blockIdx.x + 1] = (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__global__ __launch_bounds__(kBlock) void top_layer_train_kernel(
    const float* __restrict__ h, const float* __restrict__ mx, const float* __restrict__ w_self,
    const float* __restrict__ w_neigh, const float* __restrict__ bias, const int64_t* __restrict__ labels,
    const float* __restrict__ class_w, const float* __restrict__ ce_part, int ce_blocks, float* __restrict__ logits,
    float* __restrict__ g, float* __restrict__ term, float* __restrict__ part_h, float* __restrict__ part_m,
    float* __restrict__ part_b, int64_t m, int64_t rows_per_chunk) {
  constexpr int W = kTopK, C = kTopC;
  __shared__ v4f red[kWavesPerBlock - 1][2 * C][kWave];
  __shared__ v4f colsum[kBlock];
  __shared__ float dred[kBlock];
  const int lane = threadIdx.x & (kWave - 1), rl = threadIdx.x / kWave;
  const int64_t row0 = blockIdx.x * rows_per_chunk, row1 = min(m, row0 + rows_per_chunk);
  colsum[threadIdx.x] = v4f{0.f, 0.f, 0.f, 0.f};
  // the denominator: weighted_ce_finish_kernel's sum of the block partials (null: the numerator's gradient is wanted)
  float den = 0.f;
  if (ce_part != nullptr) {
    for (int b = threadIdx.x; b < ce_blocks; b += kBlock) den += ce_part[2 * b + 1];
    dred[threadIdx.x] = den;
    __syncthreads();
    for (int s = kBlock / 2; s >= 1; s >>= 1) {
      if (threadIdx.x < s) dred[threadIdx.x] += dred[threadIdx.x + s];
      __syncthreads();
    }
    den = dred[0];
  } else {
    __syncthreads();   // colsum is zero for every wave
  }
  // ws[n] / wn[n] = W_self / W_neigh [n][4 lane .. 4 lane + 3] of the stored [4, 256]
  v4f ws[C], wn[C];
#pragma unroll
  for (int n = 0; n < C; ++n) {
    ws[n] = *reinterpret_cast<const v4f*>(w_self + static_cast<size_t>(n) * W + 4 * lane);
    wn[n] = *reinterpret_cast<const v4f*>(w_neigh + static_cast<size_t>(n) * W + 4 * lane);
  }
  const v4f bv = *reinterpret_cast<const v4f*>(bias);
  v4f ah[C], am[C];
#pragma unroll
  for (int i = 0; i < C; ++i) ah[i] = am[i] = v4f{0.f, 0.f, 0.f, 0.f};
  const bool upper32 = (lane & 32) != 0, upper16 = (lane & 16) != 0;
  const int sel = lane & 3;
  // the four totals of a row's dot products with the weight rows: total n ends up in lane 16 n
  auto dots = [&](const v4f fh, const v4f fm) __attribute__((always_inline)) {
    float d[C];
#pragma unroll
    for (int n = 0; n < C; ++n) {
      d[n] = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[n] = __builtin_fmaf(fh[e], ws[n][e], d[n]);
#pragma unroll
      for (int e = 0; e < 4; ++e) d[n] = __builtin_fmaf(fm[e], wn[n][e], d[n]);
    }
    const float keep0 = upper32 ? d[2] : d[0], keep1 = upper32 ? d[3] : d[1];
    const float send0 = upper32 ? d[0] : d[2], send1 = upper32 ? d[1] : d[3];
    const float a = keep0 + __shfl_xor(send0, 32, kWave), b = keep1 + __shfl_xor(send1, 32, kWave);
    float c = (upper16 ? b : a) + __shfl_xor(upper16 ? a : b, 16, kWave);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
    return c;
  };
  // the wave's rows row0 + rl, + 4, ... in order, four at a time with their loads issued together (a row past the chunk
  // re-reads the first of the four and is not taken).  Issuing the next four rows' loads ahead of the present four's
  // arithmetic was tried: 190 registers and 34.3 us against 32.9 us at 60 000 rows.
  constexpr int kAhead = 4;
  for (int64_t first = row0 + rl; first < row1; first += kAhead * kWavesPerBlock) {
    v4f fh[kAhead], fm[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int64_t row = first + u * kWavesPerBlock < row1 ? first + u * kWavesPerBlock : first;
      fh[u] = *reinterpret_cast<const v4f*>(h + static_cast<size_t>(row) * W + 4 * lane);
      fm[u] = *reinterpret_cast<const v4f*>(mx + static_cast<size_t>(row) * W + 4 * lane);
    }
    // this lane's row: row `sel` of the four
    const bool mine = first + sel * kWavesPerBlock < row1;
    const int64_t my_row = mine ? first + sel * kWavesPerBlock : first;
    const long long label = labels[my_row];
    float x[C];
#pragma unroll
    for (int n = 0; n < C; ++n) x[n] = 0.f;
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const float c = dots(fh[u], fm[u]);
#pragma unroll
      for (int n = 0; n < C; ++n) {
        const float t = lane_value(c, 16 * n);
        x[n] = sel == u ? t : x[n];
      }
    }
#pragma unroll
    for (int n = 0; n < C; ++n) x[n] = x[n] + bv[n];
    // weighted_ce_kernel<4>, one row per lane
    float v[C];
    float top = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = x[c], top = fmaxf(top, v[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = expf(v[c] - top), sum += v[c];
    bool valid;
    int y;
    const float w = top_label_weight(label, class_w, &valid, &y);
    const float xy = y == 0 ? x[0] : y == 1 ? x[1] : y == 2 ? x[2] : x[3];
    const float loss_term = valid ? w * (logf(sum) + top - xy) : (label == -100 ? 0.0f : NAN);
    v4f gv;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float gu = w * (v[c] / sum - (c == y ? 1.0f : 0.0f));
      gv[c] = ce_part != nullptr ? gu / den : gu;
    }
    if (lane < kAhead && mine) {
      *reinterpret_cast<v4f*>(logits + static_cast<size_t>(my_row) * C) = v4f{x[0], x[1], x[2], x[3]};
      *reinterpret_cast<v4f*>(g + static_cast<size_t>(my_row) * C) = gv;
      term[my_row] = loss_term;
      const int slot = static_cast<int>((my_row - row0) & (kBlock - 1));   // slot % 4 == rl: no other wave touches it
      colsum[slot] += 1.0f * gv;
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (first + u * kWavesPerBlock < row1) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
          const float s = lane_value(gv[i], u);
          ah[i] += s * fh[u];
          am[i] += s * fm[u];
        }
      }
    }
  }
  if (rl > 0) {
#pragma unroll
    for (int i = 0; i < C; ++i) red[rl - 1][i][lane] = ah[i], red[rl - 1][C + i][lane] = am[i];
  }
  __syncthreads();
  if (rl != 0) return;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    v4f total = ah[i];
    for (int l = 1; l < kWavesPerBlock; ++l) total += red[l - 1][i][lane];
    *reinterpret_cast<v4f*>(part_h + (static_cast<size_t>(blockIdx.x) * C + i) * W + 4 * lane) = total;
  }
#pragma unroll
  for (int i = 0; i < C; ++i) {
    v4f total = am[i];
    for (int l = 1; l < kWavesPerBlock; ++l) total += red[l - 1][C + i][lane];
    *reinterpret_cast<v4f*>(part_m + (static_cast<size_t>(blockIdx.x) * C + i) * W + 4 * lane) = total;
  }
  if (lane == 0) {
    const int live = static_cast<int>(min(static_cast<int64_t>(kBlock), row1 - row0));
    v4f total = colsum[0];
    for (int l = 1; l < live; ++l) total += colsum[l];
    *reinterpret_cast<v4f*>(part_b + static_cast<size_t>(blockIdx.x) * C) = total;
  }
}

// ce_part[2 b] = weighted_ce_kernel's numerator partial of its block b, from the per-row terms the pass has stored.  (One
// workgroup of the finish launch that walked all blocks took 30 us at 60 000 rows, a chain of load latencies: the partials
// are a launch of their own, as wide as weighted_ce_kernel's.)
__global__ __launch_bounds__(kBlock) void top_loss_kernel(const float* __restrict__ term, float* __restrict__ ce_part, int64_t n) {
  __shared__ float red[kWavesPerBlock];
  float num = 0.f;
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * kCeRowsPerThread;
  if (base + kCeRowsPerThread <= n) {
    const v4f t = *reinterpret_cast<const v4f*>(term + base);
#pragma unroll
    for (int r = 0; r < kCeRowsPerThread; ++r) num += t[r];
  } else {
    for (int r = 0; r < kCeRowsPerThread; ++r) {
      if (base + r >= n) break;
      num += term[base + r];
    }
  }
  for (int s = kWave / 2; s >= 1; s >>= 1) num += __shfl_xor(num, s, kWave);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) red[wave] = num;
  __syncthreads();
  if (threadIdx.x == 0) ce_part[2 * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One finish launch.  Workgroups [0, 2 S): skinny_sum_kernel's sum of the chunk partials of gw_self and gw_neigh (S = 64
// workgroups of 16 outputs each); workgroup 2 S: of the bias partials; workgroup 2 S + 1: weighted_ce_finish_kernel's sum of
// the loss's block partials.
constexpr int kTopSumGroups = kTopC * kTopK / 16;

__global__ __launch_bounds__(kBlock) void top_finish_kernel(const float* __restrict__ part_h, const float* __restrict__ part_m,
                                                           const float* __restrict__ part_b, const float* __restrict__ ce_part,
                                                           float* __restrict__ gw_self, float* __restrict__ gw_neigh,
                                                           float* __restrict__ g_bias, float* __restrict__ out3, int chunks,
                                                           int ce_blocks) {
  if (blockIdx.x <= 2 * kTopSumGroups) {
    __shared__ float part[16][16];
    const bool is_bias = blockIdx.x == 2 * kTopSumGroups;
    const bool is_m = blockIdx.x >= kTopSumGroups;
    const float* partial = is_bias ? part_b : is_m ? part_m : part_h;
    float* dst = is_bias ? g_bias : is_m ? gw_neigh : gw_self;
    const int total_out = is_bias ? kTopC : kTopC * kTopK;
    const int group = is_bias ? 0 : is_m ? blockIdx.x - kTopSumGroups : blockIdx.x;
    const int o = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const int idx = group * 16 + o;
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
    dst[idx] = sum;
    return;
  }
  __shared__ float red[2][kBlock];
  float num = 0.f, den = 0.f;
  for (int b = threadIdx.x; b < ce_blocks; b += kBlock) num += ce_part[2 * b], den += ce_part[2 * b + 1];
  red[0][threadIdx.x] = num, red[1][threadIdx.x] = den;
  __syncthreads();
  for (int s = kBlock / 2; s >= 1; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out3[0] = red[0][0], out3[1] = red[1][0], out3[2] = red[0][0] / red[1][0];
}

inline bool top_layer_shape(int64_t m, int64_t k, int64_t n_classes) {
  return m > 0 && m < (1LL << 31) && k == kTopK && n_classes == kTopC;
}

struct TopWorkspace {   // floats from the start of the workspace
  int chunks, ce_blocks;
  int64_t rows_per_chunk, part_h, part_m, part_b, term, ce_part, total;
};

inline TopWorkspace top_workspace(int64_t m) {
  TopWorkspace t{};
  t.rows_per_chunk = (m + kSkinnyChunks - 1) / kSkinnyChunks;   // the chunks of skinny_wgrad (gts_gemm_wgrad.h)
  t.chunks = static_cast<int>((m + t.rows_per_chunk - 1) / t.rows_per_chunk);
  t.ce_blocks = static_cast<int>((m + kCeRows - 1) / kCeRows);
  const int64_t slab = static_cast<int64_t>(kSkinnyChunks) * kTopC * kTopK;
  t.part_h = 0, t.part_m = slab, t.part_b = 2 * slab;
  t.term = t.part_b + static_cast<int64_t>(kSkinnyChunks) * kTopC;
  t.ce_part = t.term + (m + 3) / 4 * 4;
  t.total = t.ce_part + 2 * static_cast<int64_t>(t.ce_blocks);
  return t;
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

extern "C" int64_t gts_sage_top_layer_train_workspace(int64_t m, int64_t k, int64_t n_classes) {
  using namespace gts;
  if (!top_layer_shape(m, k, n_classes)) return 0;
  return top_workspace(m).total * static_cast<int64_t>(sizeof(float));
}

extern "C" int32_t gts_sage_top_layer_train_f32(const float* h, const float* mx, const float* w_self, const float* w_neigh,
                                                const float* bias, const int64_t* labels, const float* class_w,
                                                int32_t normalise, float* logits, float* g, float* gw_self, float* gw_neigh,
                                                float* g_bias, float* out3, float* workspace, int64_t workspace_bytes,
                                                int64_t m, int64_t k, int64_t n_classes, void* stream) {
  using namespace gts;
  if (!h || !mx || !w_self || !w_neigh || !bias || !labels || !logits || !g || !gw_self || !gw_neigh || !g_bias || !out3 ||
      !workspace)
    return GTS_ERR_NULL;
  if (!top_layer_shape(m, k, n_classes)) return GTS_ERR_SHAPE;
  if (workspace_bytes < gts_sage_top_layer_train_workspace(m, k, n_classes)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TopWorkspace t = top_workspace(m);
  float* ce_part = workspace + t.ce_part;
  top_den_kernel<<<t.ce_blocks, kBlock, 0, st>>>(labels, class_w, ce_part, m);
  top_layer_train_kernel<<<t.chunks, kBlock, 0, st>>>(h, mx, w_self, w_neigh, bias, labels, class_w,
                                                     normalise ? ce_part : nullptr, t.ce_blocks, logits, g,
                                                     workspace + t.term, workspace + t.part_h, workspace + t.part_m,
                                                     workspace + t.part_b, m, t.rows_per_chunk);
  top_loss_kernel<<<t.ce_blocks, kBlock, 0, st>>>(workspace + t.term, ce_part, m);
  top_finish_kernel<<<2 * kTopSumGroups + 2, kBlock, 0, st>>>(workspace + t.part_h, workspace + t.part_m, workspace + t.part_b,
                                                             ce_part, gw_self, gw_neigh, g_bias, out3, t.chunks, t.ce_blocks);
  return launch_status();
}
