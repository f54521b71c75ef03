// K11 common ground: the argument block every dense GEMM kernel takes (GemmArgs), the probe hook, the shared constants
// and vector types, and the GEMM tuning knobs (gts_options.hip sets them).  Included by the gts_gemm_*.h kernel headers;
// gts_stack.hip takes kMaxProblems from here.
#pragma once
#include "gts_common.h"

namespace gts {

// Tuning knobs of the GEMM kernels (gts_set_option; the other kernels' knobs are in gts_rows.h).
inline int g_gemm_sched = 1;   // GemmArgs::sched (GTS_OPT_GEMM_SCHED); bit 0 on: -0.9 % on the 19-problem weight-gradient launch
// Tile configurations (runtime-selectable for tuning through gts_set_option).
// Defaults from tools/tune_gemm.py at M = 60 000, 256-wide (profiles/r01_tune_gemm.log).
inline int g_fwd_variant = -1;    // forward kernels (both operands kk-contiguous); -1 = a one-round tile (10 = 240-row
                                  // panels on the 16x16x4 MFMA with direct-to-fragment loads when panels leave fewer rows
                                  // per CU, else 8 = double-buffered 256x256) when that fills >= 3/4 of the CUs, else 3
                                  // (64x256, two per CU).  profiles/r02_tune_gemm.log: at M = 60 000, 256-wide, K = 256 / 512:
                                  // 8: 74.7 / 137.5 us, 9 (same panels through LDS): 73.1 / 134.3, 10: 70.4 / 129.8,
                                  // 11 / 12 (one 240 x 64 wave per SIMD, depth 1 / 2): 74.2 / 129.7, 76.0 / 134.1
inline int g_igrad_variant = 1;   // input-gradient kernels (B kk-strided)
inline int g_wgrad_variant = -1;  // split-reduction kernel; -1 = chosen per launch by wgrad_plan()
inline int g_panel_rows = 0;      // panel height (panel_rows_for): 0 = automatic; 240 / 192 / 144 force one (tools/tune_gemm.py)

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kBK = 32;         // reduction elements per LDS tile
constexpr int kMaxProblems = 32;
constexpr unsigned kOutOfRange = 0x7FFFFFF0u;   // byte offset no operand panel reaches: the load returns 0

struct GemmArgs {
  const float* a[2];    // forward / input grad: the two (a, b) reduction segments
  const float* b[2];
  int lda[2], ldb[2];
  int kseg[2];          // reduction length of each segment; kseg[1] = 0 when unused
  int ra, rb;           // output rows / cols
  float* c;             // [ra, rb]  (weight grad: slabs [problem][split][ra, rb])
  int ldc;
  const float* bias;    // [rb] or null
  int relu;
  const float* mask;    // [ra, rb] or null: output zeroed where mask <= 0 (fused ReLU backward)
  // split-reduction (weight gradient) only
  const float* pa[kMaxProblems];  // per-problem operands (same shapes)
  const float* pb[kMaxProblems];
  float* colsum;        // [problem][split][ra] column sums of A, or null
  unsigned colsum_mask; // bit q: problem q wants its column sums (wgrad_stream_kernel; the other kernels sum them all)
  int n_problems;       // 0 -> plain GEMM
  int tiles_n;          // output tiles along rb per problem
  int n_splits;
  int tiles_per_split;  // reduction tiles handled by one blockIdx.z
  int sched;            // tuning bits (GTS_OPT_GEMM_SCHED): 1 = waves further into a tile yield MFMA issue
  // chained second GEMM of the panel kernels (c2 != null): c2[ra, rb2] = act2(c[ra, rb] . b2[rb2, rb]^T + bias2),
  // computed by the workgroup that has just produced those rows of c (rb <= 256: one workgroup per row panel)
  const float* b2;
  const float* bias2;
  float* c2;
  int rb2, ldb2, ldc2, relu2;
  // attention scores riding in the epilogue of the panel kernels (GATConv: el / er = <ft[n, h, :], attn_l/r[h, :]>):
  // per output row and 64-column block the partial dot products with sc_l / sc_r [rb] go to sc_el / sc_er [ra, rb / 64]
  const float* sc_l;
  const float* sc_r;
  float* sc_el;
  float* sc_er;
  // ReLU masks as bits (layout: gts_relu_bits_bytes in gts_hip.h).  bits_out: c > 0 is recorded while c is stored;
  // bits_in: the same mask as `mask`, read by the kernels that can (the others read the floats of `mask`)
  unsigned long long* bits_out;
  const unsigned long long* bits_in;
  // the activation backward of the layer BELOW riding in an input gradient's epilogue (panel kernels only; GATConv stacks):
  // mask_kind 1 = ELU through its output: c *= mask > 0 ? 1 : mask + 1 (mask = that layer's output, read as floats);
  // col_partial [row blocks][rb]: column sums of the rows each wave stored (the bias gradient of the layer below, summed
  // over the row blocks in fixed order by sum_chunks)
  int mask_kind;
  float* col_partial;
  // the same weights in FRAGMENT ORDER (gts_pack_weights_f32; panel kernels only, null = read b / b2 as they are):
  // bp[seg] for b[seg], bp2 for b2.  One buffer_load_dwordx4 of a 16-row weight fragment then reads 1 KiB of
  // consecutive bytes (16 accesses of the vector L1) instead of 64 pieces of 16 bytes 1 KiB apart (64 accesses).
  const float* bp[2];
  const float* bp2;
};

// Phase probe of the kernel (start / operands staged / main loop done / tile stored).  The
// library only ever instantiates NoProbe, which compiles to nothing; tools/diag/gemm_probe.hip
// includes the kernel headers and instantiates the same kernels with a probe that records timestamps.
struct NoProbe {
  __device__ __forceinline__ static void mark(int /*phase*/) {}
};

inline bool aligned4(int64_t x) { return (x & 3) == 0; }

}  // namespace
}  // namespace gts
