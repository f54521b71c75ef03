// K11 dispatch and C entry points: which kernel family a plain (forward / input-gradient) problem goes to, the one
// builder of such a problem, GATConv's fc-plus-scores glue, and the weight-gradient entry points.  The kernels live in
// gts_gemm_tiles.h (32x32x2 tiles; the operand layouts are described there), gts_gemm_panel.h (16x16x4 row panels),
// gts_gemm_wgrad.h and gts_gemm_small.h; the tuning knobs are set by gts_options.hip.
// ONE translation unit on purpose, with the headers and entry points in this order: the compiler's output for six
// gemm_kernel instantiations depends on the order in which the unit instantiates its kernels (profiles/gemm_split).
#include "gts_gemm_tiles.h"
#include "gts_gemm_panel.h"
#include "gts_gemm_wgrad.h"
#include "gts_gemm_small.h"

namespace gts {
namespace {

template <bool AKC, bool BKC>
int pick_plain_variant(const GemmArgs& p) {
  int variant = BKC ? g_fwd_variant : g_igrad_variant;
  if (p.rb <= 128 && variant < 9) return 0;   // narrow outputs: the 128 x 64 / 128 x 128 tiles (unless a panel kernel is forced)
  const bool row_count_invariant = variant == -2;   // automatic, but only 32x32x2 tiles: one reduction order
  if (variant < 0) {
    const int64_t cols = (p.rb + 255) / 256;
    const int64_t big_tiles = static_cast<int64_t>((p.ra + 255) / 256) * cols;
    variant = big_tiles >= 192 ? 8 : 3;
    if constexpr (AKC && BKC) {
      // one workgroup per CU, in rounds of 256: rows a CU walks with 256-row tiles vs 240-row panels
      const int h = panel_rows_for(p.ra, cols);
      const int64_t panels = static_cast<int64_t>((p.ra + h - 1) / h) * cols;
      const int64_t rows256 = (big_tiles + 255) / 256 * 256, rows_panel = (panels + 255) / 256 * h;
      if (variant == 8 && rows_panel < rows256 && !row_count_invariant) variant = 10;
      // shorter operands: panels that fill at least 3/4 of the CUs in their one round beat two half-empty rounds of 64 x 256 tiles
      if (variant == 3 && panels >= 192 && panels <= 256 && !row_count_invariant) variant = 10;
    }
  }
  return variant;
}

template <bool BKC>
inline bool skinny_forward(const GemmArgs& p) {
  const bool automatic = BKC ? g_fwd_variant < 0 : g_igrad_variant <= 1;   // no tile variant forced (the input gradient's default is 1)
  return automatic && (p.rb == 4 || p.rb == 8) && p.ldc == p.rb && p.kseg[0] + p.kseg[1] >= 64 && p.mask == nullptr &&
         p.c2 == nullptr && p.sc_l == nullptr && p.bits_out == nullptr &&
         (BKC || (p.ldb[0] == p.rb && (p.kseg[1] == 0 || p.ldb[1] == p.rb)));
}

inline bool tiny_forward(const GemmArgs& p) {
  return (p.rb == 4 || p.rb == 8) && p.ldc == p.rb && p.kseg[0] + p.kseg[1] <= 16 && p.mask == nullptr && p.c2 == nullptr &&
         p.sc_l == nullptr && p.bits_out == nullptr && g_fwd_variant < 0;
}

template <bool AKC, bool BKC>
int launch_plain_tiles(const GemmArgs& p, int variant, hipStream_t st) {
  if constexpr (AKC && BKC) {
    if (tiny_forward(p)) {
      const unsigned blocks = static_cast<unsigned>((p.ra + 255) / 256);
      if (p.rb == 4) tiny_fwd_kernel<4><<<blocks, 256, 0, st>>>(p);
      else tiny_fwd_kernel<8><<<blocks, 256, 0, st>>>(p);
      return launch_status();
    }
  }
  if constexpr (AKC) {
    if (skinny_forward<BKC>(p)) {
      const unsigned blocks = static_cast<unsigned>((p.ra + 15) / 16);   // four waves of four rows
      if (p.rb == 4) skinny_fwd_kernel<4, BKC><<<blocks, 256, 0, st>>>(p);
      else skinny_fwd_kernel<8, BKC><<<blocks, 256, 0, st>>>(p);
      return launch_status();
    }
  }
  if (p.rb <= 64) return launch_tiles<128, 64, 2, 2, AKC, BKC>(p, 1, 1, st);
  if (p.rb <= 128) return launch_tiles<128, 128, 2, 2, AKC, BKC>(p, 1, 1, st);
  switch (variant) {
    // the variants that survived the sweeps in profiles/r01_tune_gemm.log (numbers kept from there)
    case 3: return launch_tiles<64, 256, 2, 4, AKC, BKC>(p, 1, 1, st);
    case 5: return launch_tiles<256, 128, 4, 2, AKC, BKC>(p, 1, 1, st);
    case 8: return launch_tiles<256, 256, 4, 4, AKC, BKC, true>(p, 1, 1, st);
    default: return launch_tiles<128, 256, 2, 4, AKC, BKC>(p, 1, 1, st);   // 1
  }
}

template <bool AKC, bool BKC>
int launch_plain(const GemmArgs& p, hipStream_t st) {
  const int variant = pick_plain_variant<AKC, BKC>(p);
  if constexpr (AKC && BKC) {
    if (p.c2 != nullptr && !(variant == 10 && p.rb <= kC240 && p.rb2 <= kC240 && p.rb2 > 128)) {
      // not a one-panel-per-row-block launch (or a narrow second output, which a launch of its own
      // would give to the 32x32x2 tiles): the chained GEMM runs as a launch of its own — same bits either way
      GemmArgs first = p, next{};
      first.c2 = nullptr;
      int rc = launch_plain<true, true>(first, st);
      if (rc != GTS_OK) return rc;
      next.a[0] = next.a[1] = p.c, next.b[0] = next.b[1] = p.b2, next.bp[0] = p.bp2;
      first.bp2 = nullptr;
      next.lda[0] = next.lda[1] = p.ldc, next.ldb[0] = next.ldb[1] = p.ldb2;
      next.kseg[0] = p.rb, next.kseg[1] = 0;
      next.ra = p.ra, next.rb = p.rb2, next.c = p.c2, next.ldc = p.ldc2, next.bias = p.bias2, next.relu = p.relu2;
      next.tiles_per_split = (p.rb + kBK - 1) / kBK;
      return launch_plain<true, true>(next, st);
    }
    // the panel kernels keep the mask bits themselves (written / read in their epilogue)
    if (variant == 10) {
      switch (panel_rows_for(p.ra, (p.rb + kC240 - 1) / kC240)) {
        case 144: return launch_panel_direct<3, 4, 1, NoProbe, 144>(p, st);
        case 192: return launch_panel_direct<3, 4, 1, NoProbe, 192>(p, st);
        default: return launch_panel_direct<3, 4, 1>(p, st);
      }
    }
  }
  // every other tile: the float mask is read as before, and the bits of the output come from a pass of their own
  int rc = launch_plain_tiles<AKC, BKC>(p, variant, st);
  if (rc != GTS_OK || p.bits_out == nullptr) return rc;
  const long long words = static_cast<long long>((p.ra + 3) / 4) * (p.rb >> 6);
  relu_bits_kernel<<<static_cast<unsigned>((words + 3) / 4), 256, 0, st>>>(p.c, p.bits_out, p.ra, p.rb);
  return launch_status();
}

// The plain problem c[m, rb] = a0 b0^T (+ a1 b1^T) every forward and input-gradient entry point starts from:
// a0 [m, k0], a1 [m, k1] row-major, the second pair optional, c [m, rb].  An entry point reports missing() as
// GTS_ERR_NULL and bad_shape() as GTS_ERR_SHAPE beside its own conditions of each kind, returns for m == 0, and
// sets on top of args() only what is its own.
struct PlainProblem {
  const float *a0, *b0, *a1, *b1;
  float* c;
  int64_t m, rb, k0, k1;
  bool missing() const { return !a0 || !b0 || !c || ((a1 == nullptr) != (b1 == nullptr)); }
  bool bad_shape() const {
    return m < 0 || rb <= 0 || k0 <= 0 || k1 < 0 || m >= (1LL << 31) || rb >= (1 << 20) || k0 >= (1 << 20) || k1 >= (1 << 20) ||
           !aligned4(k0) || !aligned4(k1) || (a1 && k1 == 0);
  }
  // b0 / b1 with leading dimensions ldb0 / ldb1 (k0 / k1 when their reduction index is contiguous, rb when it is
  // strided); packed = the weights in fragment order (may be null; entry 1 is read only with a second pair)
  GemmArgs args(int64_t ldb0, int64_t ldb1, const float* const* packed) const {
    GemmArgs p{};
    p.a[0] = a0, p.b[0] = b0, p.lda[0] = p.kseg[0] = static_cast<int>(k0), p.ldb[0] = static_cast<int>(ldb0);
    p.a[1] = a1 ? a1 : a0, p.b[1] = b1 ? b1 : b0, p.lda[1] = static_cast<int>(k1), p.ldb[1] = static_cast<int>(ldb1);
    p.kseg[1] = a1 ? static_cast<int>(k1) : 0;
    p.ra = static_cast<int>(m), p.rb = static_cast<int>(rb), p.c = c, p.ldc = static_cast<int>(rb);
    p.tiles_per_split = (p.kseg[0] + kBK - 1) / kBK + (p.kseg[1] + kBK - 1) / kBK;
    if (packed != nullptr) p.bp[0] = packed[0], p.bp[1] = a1 ? packed[1] : nullptr;
    return p;
  }
};

// the chained second stage c2[m, rb2] = act2(c b2^T + bias2) of a filled problem (b2 [rb2, rb]; packed entry 2)
void chain_second(GemmArgs* p, const float* b2, const float* bias2, float* c2, int64_t rb2, int relu2,
                  const float* const* packed) {
  p->b2 = b2, p->bias2 = bias2, p->c2 = c2, p->rb2 = static_cast<int>(rb2), p->ldb2 = p->rb;
  p->ldc2 = static_cast<int>(rb2), p->relu2 = relu2;
  if (packed != nullptr) p->bp2 = packed[2];
}

// out[i] = sum_p in[i * parts + p] (fixed order), two arrays in one launch
__global__ __launch_bounds__(kBlock) void sum_parts_kernel(const float* __restrict__ in_l, const float* __restrict__ in_r,
                                                           float* __restrict__ out_l, float* __restrict__ out_r,
                                                           int64_t n, int parts) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  float sl = 0.f, sr = 0.f;
  for (int q = 0; q < parts; ++q) sl += in_l[i * parts + q], sr += in_r[i * parts + q];
  out_l[i] = sl, out_r[i] = sr;
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_linear_fwd_f32(const float* a0, const float* w0, const float* a1, const float* w1, const float* bias,
                                      float* out, int64_t m, int64_t n, int64_t k0, int64_t k1, int32_t relu,
                                      uint64_t* relu_bits, const float* const* packed, void* stream) {
  using namespace gts;
  const PlainProblem q{a0, w0, a1, w1, out, m, n, k0, k1};
  if (q.missing()) return GTS_ERR_NULL;
  if (q.bad_shape() || (relu_bits && n % 64 != 0)) return GTS_ERR_SHAPE;
  if (m == 0) return GTS_OK;
  GemmArgs p = q.args(k0, k1, packed);
  p.bias = bias, p.relu = relu, p.bits_out = reinterpret_cast<unsigned long long*>(relu_bits);
  return launch_plain<true, true>(p, static_cast<hipStream_t>(stream));
}

extern "C" int32_t gts_relu_bits_pay(int64_t m, int64_t n) {
  using namespace gts;
  if (m <= 0 || n <= 0 || n % 64 != 0 || m >= (1LL << 31) || n >= (1 << 20)) return 0;
  GemmArgs p{};
  p.ra = static_cast<int>(m), p.rb = static_cast<int>(n);
  const int variant = pick_plain_variant<true, true>(p);
  return variant >= 10 && variant <= 12 ? 1 : 0;
}

extern "C" int64_t gts_relu_bits_bytes(int64_t m, int64_t n) {
  if (m < 0 || n <= 0 || n % 64 != 0) return 0;
  return (m + 3) / 4 * (n / 64) * 4 * static_cast<int64_t>(sizeof(uint64_t));
}

extern "C" int64_t gts_gat_fc_scores_workspace(int64_t m, int64_t heads, int64_t dim) {
  if (m <= 0 || heads <= 0 || dim <= 0 || dim % 64 != 0) return 0;
  return 2 * m * heads * (dim / 64) * static_cast<int64_t>(sizeof(float));
}

extern "C" int32_t gts_gat_fc_scores_f32(const float* h, const float* w_fc, const float* attn_l, const float* attn_r,
                                         float* ft, float* el, float* er, float* workspace, int64_t workspace_bytes,
                                         int64_t m, int64_t heads, int64_t dim, int64_t k, const float* w_fc_packed,
                                         void* stream) {
  using namespace gts;
  const int64_t n = heads * dim;
  const float* const packed[2] = {w_fc_packed, nullptr};
  const PlainProblem q{h, w_fc, nullptr, nullptr, ft, m, n, k, 0};
  if (q.missing() || !attn_l || !attn_r || !el || !er) return GTS_ERR_NULL;
  if (q.bad_shape() || heads <= 0 || dim <= 0) return GTS_ERR_SHAPE;
  if (m == 0) return GTS_OK;
  GemmArgs p = q.args(k, 0, packed);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int parts = static_cast<int>(dim / 64);
  const bool fuse = dim % 64 == 0 && pick_plain_variant<true, true>(p) == 10 &&
                    (parts == 1 || (workspace && workspace_bytes >= gts_gat_fc_scores_workspace(m, heads, dim)));
  if (!fuse) {   // small problems / odd head widths: the GEMM, then the scores in a pass of their own
    const int rc = launch_plain<true, true>(p, st);
    return rc != GTS_OK ? rc : gts_gat_scores_f32(ft, attn_l, attn_r, el, er, m, heads, dim, stream);
  }
  p.sc_l = attn_l, p.sc_r = attn_r;
  p.sc_el = parts == 1 ? el : workspace, p.sc_er = parts == 1 ? er : workspace + m * heads * parts;
  const int rc = launch_plain<true, true>(p, st);
  if (rc != GTS_OK || parts == 1) return rc;
  const int64_t rows = m * heads;
  sum_parts_kernel<<<static_cast<unsigned>((rows + kBlock - 1) / kBlock), kBlock, 0, st>>>(p.sc_el, p.sc_er, el, er, rows, parts);
  return launch_status();
}

extern "C" int32_t gts_linear_fwd_chain_f32(const float* a0, const float* w0, const float* a1, const float* w1,
                                            const float* bias, float* out, const float* w2, const float* bias2, float* out2,
                                            int64_t m, int64_t n, int64_t k0, int64_t k1, int32_t relu, int64_t n2,
                                            int32_t relu2, uint64_t* relu_bits, const float* const* packed, void* stream) {
  using namespace gts;
  const PlainProblem q{a0, w0, a1, w1, out, m, n, k0, k1};
  if (q.missing() || !w2 || !out2) return GTS_ERR_NULL;
  if (q.bad_shape() || n2 <= 0 || n2 >= (1 << 20) || !aligned4(n) || (relu_bits && n % 64 != 0)) return GTS_ERR_SHAPE;
  if (m == 0) return GTS_OK;
  GemmArgs p = q.args(k0, k1, packed);
  p.bias = bias, p.relu = relu, p.bits_out = reinterpret_cast<unsigned long long*>(relu_bits);
  chain_second(&p, w2, bias2, out2, n2, relu2, packed);
  return launch_plain<true, true>(p, static_cast<hipStream_t>(stream));
}

extern "C" int32_t gts_linear_bwd_input_chain_t_f32(const float* g0, const float* w0t, const float* g1, const float* w1t,
                                                    const float* relu_mask, const uint64_t* relu_bits, float* gin,
                                                    const float* w2t, float* gin2, int64_t m, int64_t k, int64_t n0,
                                                    int64_t n1, int64_t k2, const float* const* packed, void* stream) {
  using namespace gts;
  const PlainProblem q{g0, w0t, g1, w1t, gin, m, k, n0, n1};
  if (q.missing() || !w2t || !gin2 || (relu_bits && !relu_mask)) return GTS_ERR_NULL;
  if (q.bad_shape() || k2 <= 0 || k2 >= (1 << 20) || !aligned4(k) || (relu_bits && k % 64 != 0)) return GTS_ERR_SHAPE;
  if (m == 0) return GTS_OK;
  GemmArgs p = q.args(n0, n1, packed);
  p.mask = relu_mask, p.bits_in = reinterpret_cast<const unsigned long long*>(relu_bits);
  chain_second(&p, w2t, nullptr, gin2, k2, 0, packed);
  return launch_plain<true, true>(p, static_cast<hipStream_t>(stream));
}

extern "C" int32_t gts_linear_bwd_input_f32(const float* g0, const float* w0, const float* g1, const float* w1,
                                            const float* relu_mask, float* gin, int64_t m, int64_t k, int64_t n0,
                                            int64_t n1, void* stream) {
  using namespace gts;
  // C[m, k] = sum_n g[m, n] * W[n, k]:  A = g (reduction contiguous), B(k, n) = W[n*K + k]
  const PlainProblem q{g0, w0, g1, w1, gin, m, k, n0, n1};
  if (q.missing()) return GTS_ERR_NULL;
  if (q.bad_shape() || !aligned4(k)) return GTS_ERR_SHAPE;
  if (m == 0) return GTS_OK;
  GemmArgs p = q.args(k, k, nullptr);
  p.mask = relu_mask;
  return launch_plain<true, false>(p, static_cast<hipStream_t>(stream));
}

extern "C" int32_t gts_linear_bwd_input_t_f32(const float* g0, const float* w0t, const float* g1, const float* w1t,
                                              const float* relu_mask, const uint64_t* relu_bits, float* gin, int64_t m,
                                              int64_t k, int64_t n0, int64_t n1, const float* const* packed, void* stream) {
  using namespace gts;
  // C[m, k] = sum_n g[m, n] * Wt[k, n]: the forward form (both operands reduction-contiguous)
  const PlainProblem q{g0, w0t, g1, w1t, gin, m, k, n0, n1};
  if (q.missing() || (relu_bits && !relu_mask)) return GTS_ERR_NULL;
  if (q.bad_shape() || !aligned4(k) || (relu_bits && k % 64 != 0)) return GTS_ERR_SHAPE;
  if (m == 0) return GTS_OK;
  GemmArgs p = q.args(n0, n1, packed);
  p.mask = relu_mask, p.bits_in = reinterpret_cast<const unsigned long long*>(relu_bits);
  return launch_plain<true, true>(p, static_cast<hipStream_t>(stream));
}

// The panel launch that can carry an activation backward + column sums in its epilogue: tall, whole 256-column blocks.
static bool act_fold_in_epilogue(const gts::GemmArgs& p) {
  return gts::pick_plain_variant<true, true>(p) == 10 && p.rb % gts::kC240 == 0;
}

extern "C" int64_t gts_linear_bwd_input_t_act_workspace(int64_t m, int64_t k) {
  if (m <= 0 || k <= 0) return 0;
  const int64_t row_blocks = (m + 143) / 144 * 3;   // the shortest panel: most row blocks
  const int64_t pass = gts_gat_reduce_workspace(m, k) / 2;
  const int64_t fold = row_blocks * k * static_cast<int64_t>(sizeof(float));
  return fold > pass ? fold : pass;
}

extern "C" int32_t gts_linear_bwd_input_t_act_f32(const float* g0, const float* w0t, const float* g1, const float* w1t,
                                                  const float* act_out, int32_t activation, float* gin, float* g_bias,
                                                  float* workspace, int64_t workspace_bytes, int64_t m, int64_t k,
                                                  int64_t n0, int64_t n1, const float* const* packed, void* stream) {
  using namespace gts;
  const PlainProblem q{g0, w0t, g1, w1t, gin, m, k, n0, n1};
  if (q.missing() || !act_out || (g_bias && !workspace)) return GTS_ERR_NULL;
  if (activation != 1 && activation != 2) return GTS_ERR_ARGKIND;
  if (q.bad_shape() || !aligned4(k)) return GTS_ERR_SHAPE;
  if (g_bias && workspace_bytes < gts_linear_bwd_input_t_act_workspace(m, k)) return GTS_ERR_SHAPE;
  if (m == 0) return GTS_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  GemmArgs p = q.args(n0, n1, packed);
  if (activation == 1 && g_bias && act_fold_in_epilogue(p)) {
    const int rows = panel_rows_for(p.ra, p.rb / kC240);
    const int row_blocks = (p.ra + rows - 1) / rows * 3;
    p.mask = act_out, p.mask_kind = 1, p.col_partial = workspace;
    const int rc = launch_plain<true, true>(p, st);
    if (rc != GTS_OK) return rc;
    return sum_chunks(workspace, g_bias, p.rb, row_blocks, st);
  }
  // every other shape: the product, then the activation backward as the pass of its own (in place)
  const int rc = launch_plain<true, true>(p, st);
  if (rc != GTS_OK) return rc;
  return gts_gat_act_bwd_f32(gin, act_out, activation, gin, g_bias, workspace, workspace_bytes, m, k, stream);
}

extern "C" int64_t gts_linear_bwd_weight_workspace(int64_t m, int64_t n, int64_t k, int32_t n_problems) {
  using namespace gts;
  if (m <= 0 || n <= 0 || k <= 0 || n_problems < 1 || n_problems > kMaxProblems) return 0;
  const int64_t splits = wgrad_plan(m, n, k, n_problems).splits;
  const int64_t slabs = n_problems * splits * (n * k + n);
  // the skinny path handles one problem at a time: [chunks][small+1][big] (+ [chunks][small] bias)
  const int64_t skinny = skinny_workspace_floats(m, n, k) + kSkinnyChunks * (n < k ? n : 0);
  return (slabs > skinny ? slabs : skinny) * static_cast<int64_t>(sizeof(float));
}

extern "C" int32_t gts_linear_bwd_weight_f32(const float* const* g, const float* const* a, float* const* gw,
                                             float* const* gb, int32_t n_problems, float* workspace,
                                             int64_t workspace_bytes, int64_t m, int64_t n, int64_t k, void* stream) {
  using namespace gts;
  if (!g || !a || !gw || !workspace) return GTS_ERR_NULL;
  if (n_problems < 1 || n_problems > kMaxProblems) return GTS_ERR_ARGKIND;
  if (m <= 0 || n <= 0 || k <= 0 || m >= (1LL << 31) || n >= (1 << 20) || k >= (1 << 20) || !aligned4(n) || !aligned4(k))
    return GTS_ERR_SHAPE;
  if (workspace_bytes < gts_linear_bwd_weight_workspace(m, n, k, n_problems)) return GTS_ERR_SHAPE;
  bool any_bias = false;
  for (int q = 0; q < n_problems; ++q) {
    if (!g[q] || !a[q] || !gw[q]) return GTS_ERR_NULL;
    any_bias = any_bias || (gb && gb[q]);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (skinny_workspace_floats(m, n, k) > 0) {   // tiny N or K: streaming kernel, problem by problem
    for (int q = 0; q < n_problems; ++q)
      skinny_wgrad(g[q], a[q], gw[q], gb ? gb[q] : nullptr, workspace, m, n, k, st);
    return launch_status();
  }
  const WgradPlan plan = wgrad_plan(m, n, k, n_problems);
  const int splits = plan.splits;
  const int tiles = static_cast<int>((m + kBK - 1) / kBK);
  GemmArgs p{};
  // C[n, k] = sum_m g[m, n] * act[m, k]: both operands reduction-strided
  for (int q = 0; q < n_problems; ++q) p.pa[q] = g[q], p.pb[q] = a[q];
  p.a[0] = p.a[1] = g[0], p.b[0] = p.b[1] = a[0];
  p.lda[0] = p.lda[1] = static_cast<int>(n), p.ldb[0] = p.ldb[1] = static_cast<int>(k);
  p.kseg[0] = static_cast<int>(m), p.kseg[1] = 0;
  p.ra = static_cast<int>(n), p.rb = static_cast<int>(k);
  p.c = workspace, p.ldc = static_cast<int>(k);
  p.colsum = any_bias ? workspace + static_cast<size_t>(n_problems) * splits * n * k : nullptr;
  for (int q = 0; q < n_problems && any_bias; ++q)
    if (gb[q]) p.colsum_mask |= 1u << q;
  p.n_problems = n_problems, p.n_splits = splits;
  p.tiles_per_split = (tiles + splits - 1) / splits;
  int rc = launch_wgrad(p, plan, st);
  if (rc != GTS_OK) return rc;
  // one reduction launch: weight slabs of every problem, then the bias slabs that were asked for
  ReduceArgs r{};
  r.splits = splits;
  int jobs = 0;
  for (int q = 0; q < n_problems; ++q, ++jobs) {
    r.slabs[jobs] = workspace + static_cast<size_t>(q) * splits * n * k;
    r.out[jobs] = gw[q], r.n4[jobs] = static_cast<int>(n * k / 4);
  }
  for (int q = 0; q < n_problems && any_bias; ++q) {
    if (!gb[q]) continue;
    r.slabs[jobs] = p.colsum + static_cast<size_t>(q) * splits * n;
    r.out[jobs] = gb[q], r.n4[jobs] = static_cast<int>(n / 4);
    ++jobs;
  }
  reduce_slabs_kernel<<<dim3(static_cast<unsigned>((n * k / 4 + 63) / 64), jobs), kBlock, 0, st>>>(r);
  return launch_status();
}
