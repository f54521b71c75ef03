// Soft Dice over class regions + class-weighted cross-entropy on voxel logits, as two streaming passes
// (DESIGN.md §4p).  [N, C] logits with C <= 32 (4 here), int64 labels, G <= 8 regions given as bitmasks over
// the classes.  Over the valid rows (0 <= y_i < C; y_i == -100 is skipped, anything else poisons the loss):
//
//   p_i   = softmax(x_i)         q_ir = sum_c m_rc p_ic         t_ir = m_r,y_i
//   I_r   = sum_i q_ir t_ir      S_r  = sum_i q_ir              T_r  = sum_i t_ir
//   dice_r = (2 I_r + smooth) / (S_r + T_r + smooth)            L_dice = 1 - mean_r dice_r
//   CE    = sum_i w[y_i] (lse_i - x_i,y_i) / sum_i w[y_i]       L = ce_weight CE + dice_weight L_dice
//
// D1 (dice_ce_stats_kernel + dice_ce_finish_kernel) reads logits and labels once and leaves the sums, the loss
// and its parts in a 40-float `stats` block.  D2 (dice_ce_grad_kernel) reads them again with `stats` and writes
// grad_scale * dL/dx once:
//
//   D_r = S_r + T_r + smooth     a_r = -2 / (G D_r)             b_r = (2 I_r + smooth) / (G D_r^2)
//   k_ir = a_r t_ir + b_r        g_ic = sum_r m_rc k_ir         sum_c g_ic p_ic = sum_r k_ir q_ir
//   dL/dx_ij = ce_weight w[y_i] (p_ij - [j == y_i]) / sum w  +  dice_weight p_ij (g_ij - sum_r k_ir q_ir)
//
// Every sum has a fixed association (thread, wave butterfly, waves in order, blocks in order in float64): no
// float atomics, the bits do not depend on scheduling.  Neither pass keeps a row in an indexed array: the
// runtime-count form walks the row again instead (it is in L1), so no instantiation uses scratch.
#include "gts_common.h"

#include <math.h>

namespace gts {
namespace {

constexpr int kMaxClasses = 32;
constexpr int kMaxGroups = GTS_DICE_CE_MAX_GROUPS;
constexpr int kRowsPerThread = 4;
constexpr int kRowsPerBlock = kBlock * kRowsPerThread;   // row of round r of thread t: block * 1024 + r * 256 + t
constexpr int kMaxCols = 2 + 3 * kMaxGroups;             // CE num, CE den, then I_r, S_r, T_r per region

struct GroupMasks {
  uint32_t m[kMaxGroups];
};

// softmax pieces of one row without keeping the row: its maximum, the sum of exp(x - max), the unnormalised
// region masses sum_c m_rc exp(x_c - max) and x_y.  NC > 0: the row is one float4 (NC == 4 only).  NG: the
// regions walked, 4 or 8 (>= the call's count; the masks past it are 0) — a loop bounded by the run-time count
// instead costs the statistics kernel 216 VGPRs against 44.
template <int NC, int NG>
__device__ __forceinline__ void row_softmax(const float* __restrict__ x, int n_classes, int y, const GroupMasks& masks,
                                            float (&e)[NC ? NC : 1], float& mx, float& sum, float (&qs)[NG],
                                            float& xy) {
#pragma unroll
  for (int r = 0; r < NG; ++r) qs[r] = 0.f;
  sum = 0.f;
  xy = 0.f;
  if constexpr (NC == 4) {
    const Vec<4> v = Vec<4>::load(x);
    mx = fmaxf(fmaxf(v.v[0], v.v[1]), fmaxf(v.v[2], v.v[3]));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      e[c] = expf(v.v[c] - mx);
      sum += e[c];
      xy = c == y ? v.v[c] : xy;
#pragma unroll
      for (int r = 0; r < NG; ++r) qs[r] += ((masks.m[r] >> c) & 1u) ? e[c] : 0.f;
    }
  } else {
    mx = -INFINITY;
    for (int c = 0; c < n_classes; ++c) mx = fmaxf(mx, x[c]);
    for (int c = 0; c < n_classes; ++c) {
      const float ec = expf(x[c] - mx);
      sum += ec;
#pragma unroll
      for (int r = 0; r < NG; ++r) qs[r] += ((masks.m[r] >> c) & 1u) ? ec : 0.f;
    }
    xy = x[y];
  }
}

// D1: per-workgroup partial sums, column-major in `partials` ([2 + 3 G][gridDim.x]).  With the Dice term off the
// caller passes masks of 0: the region columns are then 0.
template <int NC, int NG>
__global__ __launch_bounds__(kBlock) void dice_ce_stats_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ class_w,
    GroupMasks masks, int n_groups, float* __restrict__ partials, int64_t n, int n_classes_rt) {
  const int n_classes = NC ? NC : n_classes_rt;
  constexpr int kCols = 2 + 3 * NG;
  __shared__ float red[kCols][kWavesPerBlock];
  float acc[kCols];
#pragma unroll
  for (int k = 0; k < kCols; ++k) acc[k] = 0.f;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x;
  // branch-free over the four rows (their loads issue together): a row past n or one that is not valid reads
  // row 0 and adds zeros
#pragma unroll
  for (int r4 = 0; r4 < kRowsPerThread; ++r4) {
    const int64_t i = base + static_cast<int64_t>(r4) * kBlock;
    const long long label = i < n ? labels[i] : -100;
    const bool valid = label >= 0 && label < n_classes;
    const int y = valid ? static_cast<int>(label) : 0;
    float e[NC ? NC : 1], mx, sum, qs[NG], xy;
    row_softmax<NC, NG>(logits + (valid ? i : 0) * n_classes, n_classes, y, masks, e, mx, sum, qs, xy);
    const float w = !valid ? 0.0f : (class_w != nullptr ? class_w[y] : 1.0f);
    // torch's ignore_index contributes nothing; any other label outside [0, C) is an error, reported as NaN
    // (mx - x_y) first: it is exact where y is the arg max, so a confident correct row keeps its relative accuracy
    acc[0] += valid ? w * (logf(sum) + (mx - xy)) : (label == -100 ? 0.0f : NAN);
    acc[1] += w;
    const float inv = valid ? 1.0f / sum : 0.0f;
#pragma unroll
    for (int r = 0; r < NG; ++r) {
      const float q = qs[r] * inv;
      const bool t = valid && ((masks.m[r] >> y) & 1u);
      acc[2 + 3 * r] += t ? q : 0.f;
      acc[3 + 3 * r] += q;
      acc[4 + 3 * r] += t ? 1.f : 0.f;
    }
  }
  // wave butterfly, then the four wave totals in wave order: a fixed association
  const int cols = 2 + 3 * n_groups;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    float v = acc[k];
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    if (lane == 0) red[k][wave] = v;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < cols) {
    const int k = threadIdx.x;
    partials[static_cast<int64_t>(k) * gridDim.x + blockIdx.x] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
  }
}

// one workgroup adds the per-block partials in block order, in float64, and writes the stats block
__global__ __launch_bounds__(kBlock) void dice_ce_finish_kernel(const float* __restrict__ partials, int n_blocks,
                                                               int n_groups, float ce_weight, float dice_weight,
                                                               float smooth, float* __restrict__ stats) {
  __shared__ double red[kMaxCols][kWavesPerBlock];
  __shared__ double total[kMaxCols];
  const int cols = 2 + 3 * n_groups;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int k = 0; k < cols; ++k) {
    double v = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += kBlock) v += static_cast<double>(partials[static_cast<int64_t>(k) * n_blocks + b]);
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    if (lane == 0) red[k][wave] = v;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < cols) {
    const int k = threadIdx.x;
    total[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 0; k < GTS_DICE_CE_STATS_FLOATS; ++k) stats[k] = 0.f;
  const double num = total[0], den = total[1];
  // a term whose weight is 0 is skipped, not multiplied: CE of no valid row is 0 / 0
  const double ce = ce_weight != 0.f ? num / den : 0.0;
  double dice_sum = 0.0;
  if (dice_weight != 0.f) {
    for (int r = 0; r < n_groups; ++r) {
      const double i_r = total[2 + 3 * r], s_r = total[3 + 3 * r], t_r = total[4 + 3 * r];
      const double dice = (2.0 * i_r + smooth) / (s_r + t_r + smooth);
      dice_sum += dice;
      stats[GTS_DICE_CE_STATS_DICE + r] = static_cast<float>(dice);
      stats[GTS_DICE_CE_STATS_I + r] = static_cast<float>(i_r);
      stats[GTS_DICE_CE_STATS_S + r] = static_cast<float>(s_r);
      stats[GTS_DICE_CE_STATS_T + r] = static_cast<float>(t_r);
    }
  }
  const double l_dice = dice_weight != 0.f ? 1.0 - dice_sum / n_groups : 0.0;
  double loss = (ce_weight != 0.f ? static_cast<double>(ce_weight) * ce : 0.0) +
                (dice_weight != 0.f ? static_cast<double>(dice_weight) * l_dice : 0.0);
  if (num != num) loss = NAN;   // a label outside [0, C) other than -100, whatever the weights
  stats[GTS_DICE_CE_STATS_LOSS] = static_cast<float>(loss);
  stats[GTS_DICE_CE_STATS_CE] = static_cast<float>(ce);
  stats[GTS_DICE_CE_STATS_LDICE] = static_cast<float>(l_dice);
  stats[GTS_DICE_CE_STATS_CE_NUM] = static_cast<float>(num);
  stats[GTS_DICE_CE_STATS_CE_DEN] = static_cast<float>(den);
}

// D2: grad[i, :] = grad_scale * dL/dx_i, zero for a row that is not valid.  With the Dice term off the caller
// passes masks of 0.
template <int NC, int NG>
__global__ __launch_bounds__(kBlock) void dice_ce_grad_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ class_w,
    GroupMasks masks, int n_groups, float ce_weight, float dice_weight, float smooth,
    const float* __restrict__ stats, const float* __restrict__ grad_scale, float* __restrict__ grad, int64_t n,
    int n_classes_rt) {
  const int n_classes = NC ? NC : n_classes_rt;
  const int ng = dice_weight != 0.f ? n_groups : 0;
  // the coefficients of the step, formed once per workgroup: [0] CE scale, [1 + r] a_r, [9 + r] b_r (upstream
  // gradient and term weights folded in)
  __shared__ float coef[1 + 2 * kMaxGroups];
  if (threadIdx.x < 1 + kMaxGroups) {
    const float up = grad_scale != nullptr ? grad_scale[0] : 1.0f;
    if (threadIdx.x == 0) {
      coef[0] = ce_weight != 0.f ? up * ce_weight / stats[GTS_DICE_CE_STATS_CE_DEN] : 0.f;
    } else {
      const int r = threadIdx.x - 1;
      float a = 0.f, b = 0.f;
      if (r < ng) {
        const float d = stats[GTS_DICE_CE_STATS_S + r] + stats[GTS_DICE_CE_STATS_T + r] + smooth;
        const float gd = static_cast<float>(ng) * d;
        a = up * dice_weight * (-2.0f / gd);
        b = up * dice_weight * ((2.0f * stats[GTS_DICE_CE_STATS_I + r] + smooth) / (gd * d));
      }
      coef[1 + r] = a;
      coef[1 + kMaxGroups + r] = b;
    }
  }
  __syncthreads();
  const float ce_scale = coef[0];
  float a[NG], b[NG];
#pragma unroll
  for (int r = 0; r < NG; ++r) a[r] = coef[1 + r], b[r] = coef[1 + kMaxGroups + r];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x;
  // branch-free up to the store, as in D1: a row that is not valid reads row 0 and writes zeros
#pragma unroll
  for (int r4 = 0; r4 < kRowsPerThread; ++r4) {
    const int64_t i = base + static_cast<int64_t>(r4) * kBlock;
    const bool in = i < n;
    const long long label = in ? labels[i] : -100;
    const bool valid = label >= 0 && label < n_classes;
    const int y = valid ? static_cast<int>(label) : 0;
    const float* x = logits + (valid ? i : 0) * n_classes;
    float e[NC ? NC : 1], mx, sum, qs[NG], xy;
    row_softmax<NC, NG>(x, n_classes, y, masks, e, mx, sum, qs, xy);
    const float inv = valid ? 1.0f / sum : 0.0f;        // p = 0 zeroes both terms of a row that is not valid
    const float wce = !valid ? 0.f : ce_scale * (class_w != nullptr ? class_w[y] : 1.0f);
    // k_r = a_r t_r + b_r and sum_c g_c p_c = sum_r k_r q_r
    float kr[NG], gdot = 0.f;
#pragma unroll
    for (int r = 0; r < NG; ++r) {
      kr[r] = ((masks.m[r] >> y) & 1u) ? a[r] + b[r] : b[r];
      gdot += kr[r] * (qs[r] * inv);
    }
    float* g = grad + i * n_classes;
    if constexpr (NC == 4) {
      Vec<4> out;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float p = e[c] * inv;
        float gc = 0.f;
#pragma unroll
        for (int r = 0; r < NG; ++r) gc += ((masks.m[r] >> c) & 1u) ? kr[r] : 0.f;
        out.v[c] = wce * (p - (c == y ? 1.0f : 0.0f)) + p * (gc - gdot);
      }
      if (in) out.store(g);
    } else {
      if (in)
        for (int c = 0; c < n_classes; ++c) {
          const float p = expf(x[c] - mx) * inv;
          float gc = 0.f;
#pragma unroll
          for (int r = 0; r < NG; ++r) gc += ((masks.m[r] >> c) & 1u) ? kr[r] : 0.f;
          g[c] = wce * (p - (c == y ? 1.0f : 0.0f)) + p * (gc - gdot);
        }
    }
  }
}

// the C == 4 forms move a row as one 16-byte access: a row base that is not 16-byte aligned (a view at an odd
// storage offset) takes the run-time-count form instead, which reads and writes float by float
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int64_t dice_ce_blocks(int64_t n) { return (n + kRowsPerBlock - 1) / kRowsPerBlock; }

// the argument checks shared by both entry points (pointers aside): 0 or the GTS_ERR_* code
int check_args(const uint32_t* group_masks, int32_t n_groups, double ce_weight, double dice_weight, double smooth,
               int64_t n, int64_t n_classes, GroupMasks* masks) {
  if (n <= 0 || n >= (1LL << 40) || n_classes < 1 || n_classes > kMaxClasses) return GTS_ERR_SHAPE;
  if (n_groups < 1 || n_groups > kMaxGroups) return GTS_ERR_SHAPE;
  if (dice_ce_blocks(n) >= (1LL << 31)) return GTS_ERR_SHAPE;
  if (!(ce_weight >= 0.0) || !(dice_weight >= 0.0) || !isfinite(ce_weight) || !isfinite(dice_weight))
    return GTS_ERR_ARGKIND;
  if (!(static_cast<float>(smooth) > 0.f) || !isfinite(smooth)) return GTS_ERR_ARGKIND;   // positive as the kernels see it
  const uint32_t all = n_classes == 32 ? 0xFFFFFFFFu : ((1u << n_classes) - 1u);
  for (int r = 0; r < kMaxGroups; ++r) {
    masks->m[r] = r < n_groups ? group_masks[r] : 0u;
    if (r < n_groups && (masks->m[r] == 0u || (masks->m[r] & ~all) != 0u)) return GTS_ERR_ARGKIND;
  }
  return GTS_OK;
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_dice_ce_workspace(int64_t n, int32_t n_groups) {
  using namespace gts;
  if (n <= 0 || n_groups < 1 || n_groups > kMaxGroups) return 0;
  return dice_ce_blocks(n) * (2 + 3 * n_groups) * static_cast<int64_t>(sizeof(float));
}

extern "C" int32_t gts_dice_ce_fwd_f32(const float* logits, const int64_t* labels, const float* class_w,
                                       const uint32_t* group_masks, int32_t n_groups, double ce_weight,
                                       double dice_weight, double smooth, float* stats, void* workspace,
                                       int64_t workspace_bytes, int64_t n, int64_t n_classes, void* stream) {
  using namespace gts;
  if (!logits || !labels || !group_masks || !stats || !workspace) return GTS_ERR_NULL;
  GroupMasks masks;
  const int bad = check_args(group_masks, n_groups, ce_weight, dice_weight, smooth, n, n_classes, &masks);
  if (bad != GTS_OK) return bad;
  if (workspace_bytes < gts_dice_ce_workspace(n, n_groups)) return GTS_ERR_SHAPE;
  const unsigned blocks = static_cast<unsigned>(dice_ce_blocks(n));
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partials = static_cast<float*>(workspace);
  if (dice_weight == 0.0) masks = GroupMasks{};
  const int nc = static_cast<int>(n_classes);
  const bool row4 = n_classes == 4 && aligned16(logits);
  if (row4 && n_groups <= 4)
    dice_ce_stats_kernel<4, 4><<<blocks, kBlock, 0, st>>>(logits, labels, class_w, masks, n_groups, partials, n, nc);
  else if (row4)
    dice_ce_stats_kernel<4, 8><<<blocks, kBlock, 0, st>>>(logits, labels, class_w, masks, n_groups, partials, n, nc);
  else if (n_groups <= 4)
    dice_ce_stats_kernel<0, 4><<<blocks, kBlock, 0, st>>>(logits, labels, class_w, masks, n_groups, partials, n, nc);
  else
    dice_ce_stats_kernel<0, 8><<<blocks, kBlock, 0, st>>>(logits, labels, class_w, masks, n_groups, partials, n, nc);
  dice_ce_finish_kernel<<<1, kBlock, 0, st>>>(partials, static_cast<int>(blocks), n_groups,
                                              static_cast<float>(ce_weight), static_cast<float>(dice_weight),
                                              static_cast<float>(smooth), stats);
  return launch_status();
}

extern "C" int32_t gts_dice_ce_bwd_f32(const float* logits, const int64_t* labels, const float* class_w,
                                       const uint32_t* group_masks, int32_t n_groups, double ce_weight,
                                       double dice_weight, double smooth, const float* stats,
                                       const float* grad_scale, float* grad, int64_t n, int64_t n_classes,
                                       void* stream) {
  using namespace gts;
  if (!logits || !labels || !group_masks || !stats || !grad) return GTS_ERR_NULL;
  GroupMasks masks;
  const int bad = check_args(group_masks, n_groups, ce_weight, dice_weight, smooth, n, n_classes, &masks);
  if (bad != GTS_OK) return bad;
  const unsigned blocks = static_cast<unsigned>(dice_ce_blocks(n));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float cw = static_cast<float>(ce_weight), dw = static_cast<float>(dice_weight), sm = static_cast<float>(smooth);
  if (dice_weight == 0.0) masks = GroupMasks{};
  const int nc = static_cast<int>(n_classes);
  const bool row4 = n_classes == 4 && aligned16(logits) && aligned16(grad);
  if (row4 && n_groups <= 4)
    dice_ce_grad_kernel<4, 4><<<blocks, kBlock, 0, st>>>(logits, labels, class_w, masks, n_groups, cw, dw, sm, stats,
                                                         grad_scale, grad, n, nc);
  else if (row4)
    dice_ce_grad_kernel<4, 8><<<blocks, kBlock, 0, st>>>(logits, labels, class_w, masks, n_groups, cw, dw, sm, stats,
                                                         grad_scale, grad, n, nc);
  else if (n_groups <= 4)
    dice_ce_grad_kernel<0, 4><<<blocks, kBlock, 0, st>>>(logits, labels, class_w, masks, n_groups, cw, dw, sm, stats,
                                                         grad_scale, grad, n, nc);
  else
    dice_ce_grad_kernel<0, 8><<<blocks, kBlock, 0, st>>>(logits, labels, class_w, masks, n_groups, cw, dw, sm, stats,
                                                         grad_scale, grad, n, nc);
  return launch_status();
}
