// K11 weight gradients: the LDS-DMA streaming tile (wgrad_stream_kernel), the fixed-order slab reduction, the split
// plan and launcher, and the skinny path for tiny N or K.  Included by gts_gemm.hip; tools/diag/gemm_probe.hip
// includes it for the rejected weight-gradient tiles of tools/diag/gemm_rejected_forms.inc.
#pragma once
#include <type_traits>

#include "gts_gemm_tiles.h"

namespace gts {
namespace {

// ---- weight gradients, a main loop of MFMAs, LDS reads and nothing else (round 3) -----------------------------------
// The f32 MFMA and the vector ALU share their arithmetic on gfx950: a vector instruction between two MFMAs costs the
// wave ~17 cycles of matrix-pipe time, each further one ~4 (profiles/r03_mfma_valu_coissue.log).  gemm_kernel
// (gts_gemm_tiles.h) and the rejected wgrad_dma_kernel carry 20 - 30 of them per reduction tile (fragment addresses, DMA offsets, the bias column sums in every wave): that,
// not the issue of the LDS reads, is what held them at 87.9 % of the matrix pipe.  Same 256 x 256 tile, slabs, MFMA
// order and column-sum order as gemm_kernel<256, 256, 4, 4, false, false, true> (bit-identical results), same
// LDS-DMA tile copies (as the rejected wgrad_dma_kernel, tools/diag/gemm_rejected_forms.inc), but:
//   * LDS holds [A image 0 | A image 1 | B image 0 | B image 1] (32 KiB each), so ONE address register per 32-row
//     block reaches every fragment element of BOTH images through the immediate offsets of ds_read2st64_b32 (units of
//     256 B: reduction row r of image I sits 4 r + 128 I units up; a read fetches steps j, j + 1);
//   * the reduction tiles are walked two at a time, the image a compile-time fact;
//   * a tile's DMA descriptor is built by the scalar unit (base and length of the tile's 32 rows: rows past the split
//     read as zeros), the lane offsets never change;
//   * the bias column sums run in one wave per SIMD (wn == wm) and only for the problems that have a bias, in a
//     copy of the loop of their own, so the other waves' loop has no vector instruction at all.
// Fragment reads are issued one pair of steps ahead by inline assembly (the compiler would pair tm = 0 / 1 into
// ds_read2_b32 and add up a new address per step); each wait carries the fragment registers as operands so the MFMAs
// that consume them cannot be scheduled above it.
typedef float v2f __attribute__((ext_vector_type(2)));

template <int O0, int O1>
__device__ __forceinline__ v2f lds_read2st64(unsigned addr) {
  static_assert(O0 >= 0 && O1 <= 255, "ds_read2st64_b32 offsets are 8 bits");
  v2f r;
  asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(r) : "v"(addr), "n"(O0), "n"(O1));
  return r;
}

template <class Probe = NoProbe>
__global__ __launch_bounds__(1024, 4) void wgrad_stream_kernel(const GemmArgs p) {
  constexpr int BM = 256, BN = 256, WM = 4, WN = 4, WTM = 64, WTN = 64, TM = 2, TN = 2;
  constexpr int kPlane = kBK * BM;   // floats of one operand image (32 KiB)
  static_assert(BM == BN && kPlane * 4 == 128 * 256, "image I of an operand sits 128 offset units above image 0");
  __shared__ float lds[4 * kPlane];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int i = lane & 31, h = lane >> 5;
  const int problem = blockIdx.y / p.tiles_n, tile_n = blockIdx.y % p.tiles_n;
  const int m0 = blockIdx.x * BM, n0 = tile_n * BN;   // output rows (columns of g) / output columns (columns of act)
  const float* g = kernarg_entry<const float*>(offsetof(GemmArgs, pa), problem);
  const float* act = kernarg_entry<const float*>(offsetof(GemmArgs, pb), problem);
  const int ldg = p.lda[0], lda = p.ldb[0];
  const int n_tiles_all = (p.kseg[0] + kBK - 1) / kBK;
  const int t_beg = min(n_tiles_all, static_cast<int>(blockIdx.z) * p.tiles_per_split);
  const int t_end = min(n_tiles_all, t_beg + p.tiles_per_split);
  const int row_beg = t_beg * kBK, rows = min(p.kseg[0], t_end * kBK) - row_beg;   // reduction rows of this split
  const int n_tiles = t_end - t_beg;
  // wave w copies rows w and w + 16 of both tiles; a lane whose four columns lie past the operand is parked outside
  // the descriptor (zeros land in LDS)
  const bool g_ok = m0 + 4 * lane < p.ra, a_ok = n0 + 4 * lane < p.rb;
  const unsigned vg0 = g_ok ? static_cast<unsigned>(wave * ldg + m0 + 4 * lane) * 4 : kOutOfRange;
  const unsigned vg1 = g_ok ? static_cast<unsigned>((wave + 16) * ldg + m0 + 4 * lane) * 4 : kOutOfRange;
  const unsigned va0 = a_ok ? static_cast<unsigned>(wave * lda + n0 + 4 * lane) * 4 : kOutOfRange;
  const unsigned va1 = a_ok ? static_cast<unsigned>((wave + 16) * lda + n0 + 4 * lane) * 4 : kOutOfRange;
  auto dma = [&](int t, int image) __attribute__((always_inline)) {   // tile t (counted from t_beg) -> image
    const int r0 = row_beg + t * kBK, nr = min(kBK, rows - t * kBK);
    __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g + static_cast<size_t>(r0) * ldg), 0,
                                                                  nr * ldg * 4, 0x00020000);
    __amdgpu_buffer_rsrc_t ract = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(act + static_cast<size_t>(r0) * lda), 0,
                                                                    nr * lda * 4, 0x00020000);
    float* ia = lds + image * kPlane + wave * BM;
    float* ib = lds + (2 + image) * kPlane + wave * BN;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, ia, 16, vg0, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, ia + 16 * BM, 16, vg1, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(ract, ib, 16, va0, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(ract, ib + 16 * BN, 16, va1, 0, 0, 0);
  };

  v16f acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
  float csum[TM] = {0.f, 0.f};
  const bool want_colsum = p.colsum != nullptr && tile_n == 0 && wn == wm && ((p.colsum_mask >> problem) & 1u) != 0;

  // fragment addresses (LDS bytes) of image 0: element (reduction row 4 h, column of this lane's 32-row block)
  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)lds));
  const unsigned a_addr0 = lds0 + static_cast<unsigned>(4 * h * BM + wm * WTM + i) * 4, a_addr1 = a_addr0 + 128;
  const unsigned b_addr0 = lds0 + static_cast<unsigned>(2 * kPlane + 4 * h * BN + wn * WTN + i) * 4, b_addr1 = b_addr0 + 128;
  v2f fa[2][TM], fb[2][TN];   // two pairs of steps in flight: pair q in slot q & 1
  fa[0][0] = fa[0][1] = fa[1][0] = fa[1][1] = v2f{0.f, 0.f};
  fb[0][0] = fb[0][1] = fb[1][0] = fb[1][1] = v2f{0.f, 0.f};

  // the four reads of pair Q (steps 2 Q, 2 Q + 1: reduction rows 8 (Q / 2) + 2 (Q % 2) + {0, 1} (+ 4 h)) of image IMG
  auto issue = [&](auto img_c, auto pair_c) __attribute__((always_inline)) {
    constexpr int IMG = decltype(img_c)::value, Q = decltype(pair_c)::value;
    constexpr int O = 4 * (8 * (Q / 2) + 2 * (Q % 2)) + 128 * IMG;
    fa[Q & 1][0] = lds_read2st64<O, O + 4>(a_addr0);
    fa[Q & 1][1] = lds_read2st64<O, O + 4>(a_addr1);
    fb[Q & 1][0] = lds_read2st64<O, O + 4>(b_addr0);
    fb[Q & 1][1] = lds_read2st64<O, O + 4>(b_addr1);
  };
  auto multiply = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[slot][tm][e], fb[slot][tn][e], acc[tm][tn], 0, 0, 0);
  };
  float half_sum[TM] = {0.f, 0.f};
  // one reduction tile out of image IMG; on entry the reads of its pair 0 are in flight (slot 0)
  auto tile = [&](auto img_c, auto cs_c, int t) __attribute__((always_inline)) {
    constexpr int IMG = decltype(img_c)::value;
    constexpr bool CS = decltype(cs_c)::value;
    auto pair = [&](auto pair_c) __attribute__((always_inline)) {
      constexpr int Q = decltype(pair_c)::value, S = Q & 1;
      if constexpr (Q < 7) {
        issue(img_c, std::integral_constant<int, Q + 1>{});
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(fa[S][0]), "+v"(fa[S][1]), "+v"(fb[S][0]), "+v"(fb[S][1]));
      } else {
        // every read of this image has been issued: wait for them and for this wave's pieces of the next tile, meet
        // the other waves, hand the image to the DMA of the tile after next and start on the next image
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier"
                     : "+v"(fa[S][0]), "+v"(fa[S][1]), "+v"(fb[S][0]), "+v"(fb[S][1]) : : "memory");
        if (t + 2 < n_tiles) dma(t + 2, IMG);
        if (t + 1 < n_tiles) issue(std::integral_constant<int, IMG ^ 1>{}, std::integral_constant<int, 0>{});
      }
      if constexpr (Q % 2 == 0) {   // waves further into a tile yield MFMA issue (the builtin wants a literal)
        if constexpr (Q == 0) __builtin_amdgcn_s_setprio(3);
        else if constexpr (Q == 2) __builtin_amdgcn_s_setprio(2);
        else if constexpr (Q == 4) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      if constexpr (CS) {   // csum += (a0 + a1) + (a2 + a3) per group of four steps, as gemm_kernel sums them; the adds are
                            // pinned here (left to the compiler they drift away from the fragments, which it then spills)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
          if constexpr (Q % 2 == 0) {
            asm volatile("v_add_f32 %0, %1, %2" : "=v"(half_sum[tm]) : "v"(fa[S][tm][0]), "v"(fa[S][tm][1]));
          } else {
            float upper;
            asm volatile("v_add_f32 %0, %1, %2" : "=v"(upper) : "v"(fa[S][tm][0]), "v"(fa[S][tm][1]));
            asm volatile("v_add_f32 %0, %1, %2" : "=v"(upper) : "v"(half_sum[tm]), "v"(upper));
            asm volatile("v_add_f32 %0, %1, %2" : "+v"(csum[tm]) : "v"(csum[tm]), "v"(upper));
          }
        }
      }
      multiply(S);
    };
    pair(std::integral_constant<int, 0>{}), pair(std::integral_constant<int, 1>{}), pair(std::integral_constant<int, 2>{}),
        pair(std::integral_constant<int, 3>{}), pair(std::integral_constant<int, 4>{}), pair(std::integral_constant<int, 5>{}),
        pair(std::integral_constant<int, 6>{}), pair(std::integral_constant<int, 7>{});
  };
  auto reduce = [&](auto cs_c) __attribute__((always_inline)) {
    int t = 0;
    for (; t + 1 < n_tiles; t += 2) {
      tile(std::integral_constant<int, 0>{}, cs_c, t);
      tile(std::integral_constant<int, 1>{}, cs_c, t + 1);
    }
    if (t < n_tiles) tile(std::integral_constant<int, 0>{}, cs_c, t);
  };

  Probe::mark(0);
  if (n_tiles > 0) {
    dma(0, 0);
    if (n_tiles > 1) dma(1, 1);
    // every piece has landed, everybody's.  vmcnt(0), not (4): should the compiler ever spill around here, its scratch
    // stores would count in vmcnt too and need not retire in order with the loads
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    issue(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
  }
  Probe::mark(1);
  if (want_colsum) reduce(std::true_type{});
  else reduce(std::false_type{});
  __builtin_amdgcn_s_setprio(0);
  Probe::mark(2);
  const size_t slab = static_cast<size_t>(problem) * p.n_splits + blockIdx.z;
  write_tile<BM, BN, WM, WN>(p, lds, p.c + slab * p.ra * p.ldc, acc, m0, n0);
  Probe::mark(3);
  if (want_colsum) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const float total = csum[tm] + __shfl_xor(csum[tm], 32, kWave);   // the two kk halves
      const int row = m0 + wm * WTM + tm * 32 + i;
      if (h == 0 && row < p.ra) p.colsum[slab * p.ra + row] = total;
    }
  }
}

struct ReduceArgs {   // weight-slab + bias-slab jobs of every problem in one launch (blockIdx.y = job)
  const float* slabs[2 * kMaxProblems];
  float* out[2 * kMaxProblems];
  int n4[2 * kMaxProblems];  // float4 per job
  int splits;
};

__global__ __launch_bounds__(kBlock) void reduce_slabs_kernel(const ReduceArgs p) {
  __shared__ v4f part[4][64];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int q = blockIdx.y;
  const float* slabs = kernarg_entry<const float*>(offsetof(ReduceArgs, slabs), q);
  float* out = kernarg_entry<float*>(offsetof(ReduceArgs, out), q);
  const int n4 = kernarg_entry<int>(offsetof(ReduceArgs, n4), q);
  const int i = blockIdx.x * 64 + col;
  if (blockIdx.x * 64 >= n4) return;   // whole workgroup past this job's end
  v4f acc = {0.f, 0.f, 0.f, 0.f};
  if (i < n4) {
    const v4f* src = reinterpret_cast<const v4f*>(slabs) + i;
#pragma unroll 8   // independent loads, issued back to back (the adds keep their order)
    for (int s = grp; s < p.splits; s += 4) acc += src[static_cast<size_t>(s) * n4];
  }
  part[grp][col] = acc;
  __syncthreads();
  if (grp == 0 && i < n4) {
    const v4f total = (part[0][col] + part[1][col]) + (part[2][col] + part[3][col]);
    reinterpret_cast<v4f*>(out)[i] = total;
  }
}

}  // namespace
}  // namespace gts
// the skinny kernels, at this place of the unit (gts_gemm.hip: its kernels keep their order)
#include "gts_gemm_skinny.h"
namespace gts {
namespace {

inline int64_t skinny_workspace_floats(int64_t m, int64_t n, int64_t k) {
  const int64_t small = n < k ? n : k, big = n < k ? k : n;
  if (small + 1 > kSkinnyMax || big < 64) return 0;
  return static_cast<int64_t>(kSkinnyChunks) * (small + 1) * big;
}

template <int S>
void launch_skinny(const float* skinny, int s_cols, const float* wide, float* partial, int64_t m, int w,
                   int chunks, int64_t rpc, hipStream_t st) {
  skinny_wgrad_kernel<S><<<chunks, kBlock, 0, st>>>(skinny, s_cols, wide, partial, m, w, rpc);
}

// gw[n,k] (+ gb[n]) of ONE problem through the skinny path; returns false when it does not apply
inline bool skinny_wgrad(const float* g, const float* a, float* gw, float* gb, float* workspace, int64_t m,
                  int64_t n, int64_t k, hipStream_t st) {
  if (skinny_workspace_floats(m, n, k) == 0) return false;
  const bool g_is_skinny = n < k;          // gw[n,k] = skinny^T wide directly; else transposed
  const float* skinny = g_is_skinny ? g : a;
  const float* wide = g_is_skinny ? a : g;
  const int s_cols = static_cast<int>(g_is_skinny ? n : k), w = static_cast<int>(g_is_skinny ? k : n);
  const bool ones_row = !g_is_skinny && gb != nullptr;   // colsum(wide = g) is the bias gradient
  const int rows = s_cols + (ones_row ? 1 : 0);
  const int64_t rpc = (m + kSkinnyChunks - 1) / kSkinnyChunks;
  const int chunks = static_cast<int>((m + rpc - 1) / rpc);
  switch (rows) {
    case 1: launch_skinny<1>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
    case 2: launch_skinny<2>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
    case 3: launch_skinny<3>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
    case 4: launch_skinny<4>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
    case 5: launch_skinny<5>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
    case 6: launch_skinny<6>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
    case 7: launch_skinny<7>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
    case 8: launch_skinny<8>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
    default: launch_skinny<9>(skinny, s_cols, wide, workspace, m, w, chunks, rpc, st); break;
  }
  skinny_sum_kernel<<<(rows * w + 15) / 16, kBlock, 0, st>>>(
      workspace, gw, ones_row ? gb : nullptr, rows, s_cols, w, chunks, g_is_skinny ? 0 : 1);
  if (g_is_skinny && gb != nullptr) {
    // bias gradient = column sums of the skinny g [m, n]: the same kernel with a 1-column "ones"
    // operand (s_cols = 0 -> the single P row is sum_m wide) over wide = g needs n % 4 == 0
    float* part = workspace + static_cast<size_t>(chunks) * rows * w;
    skinny_wgrad_kernel<1><<<chunks, kBlock, 0, st>>>(nullptr, 0, g, part, m, static_cast<int>(n), rpc);
    skinny_sum_kernel<<<(static_cast<int>(n) + 15) / 16, kBlock, 0, st>>>(
        part, nullptr, gb, 1, 0, static_cast<int>(n), chunks, 0);
  }
  return true;
}

// Split-reduction plan of a weight-gradient launch: tile variant, its edge lengths, and how many
// ways the reduction over the M nodes is split (also sizes the workspace).
struct WgradPlan {
  int variant, bm, bn, splits;
};

inline void wgrad_candidate(int variant, int64_t k, int* bm, int* bn, int64_t* slots) {
  *bm = 128, *bn = k <= 64 ? 64 : 128, *slots = 512;   // 2 workgroups per CU
  if (k <= 64) return;
  if (variant == 2) *bn = 256;
  if (variant == 4 || variant == 6) *bm = 256, *bn = 256, *slots = 256;  // one workgroup per CU
}

inline WgradPlan wgrad_plan(int64_t m, int64_t n, int64_t k, int n_problems) {
  const int64_t tiles = (m + kBK - 1) / kBK;
  // automatic (in-bench sweeps, profiles/r01_tune_gemm.log): up to 4 problems (one layer) ->
  // 128x128 tiles (1): 42 splits of the three 256x256 problems fill 504 of 512 slots with half the
  // slab traffic of the wider tiles.  More problems (a whole layer stack at once) -> of the
  // double-buffered 256x256 tile (4) and the 128x256 tile (2), the one whose workgroup count
  // (output tiles x splits, never more than the slots: no lone tail round) fills the chip best;
  // 19 problems: variant 4, 13 splits, 247 of 256 slots, 144 reduction tiles per workgroup.
  // Few problems with LARGE outputs (GAT: one or two 1024 x 1024 gradients per layer, 16 output
  // tiles of 256 x 256 x 16 splits = 256 workgroups): the double-buffered 256x256 tile again
  // (C3 308 -> 312 graphs/s, profiles/r02_ab_c3_wgrad.log).
  // Round 3: 6 (wgrad_stream_kernel: the same tile and bits as 4 with a main loop free of vector instructions) takes
  // the place of 4 — 1 094 against 1 193 us for the 19 problems of C2 (profiles/r03_tune_wgrad.log).
  static const int kMany[2] = {6, 2};
  static const int kFewLarge[2] = {6, 1};
  const bool few = n_problems <= 4;
  const bool large = n * k * n_problems >= (1 << 20);
  const int n_candidates = g_wgrad_variant >= 0 || (few && !large) ? 1 : 2;
  WgradPlan best{};
  double best_fill = -1.0;
  for (int c = 0; c < n_candidates; ++c) {
    WgradPlan plan{};
    plan.variant = g_wgrad_variant >= 0 ? g_wgrad_variant : (few ? (large ? kFewLarge[c] : 1) : kMany[c]);
    int64_t slots;
    wgrad_candidate(plan.variant, k, &plan.bm, &plan.bn, &slots);
    const int64_t out_tiles = ((n + plan.bm - 1) / plan.bm) * ((k + plan.bn - 1) / plan.bn) * n_problems;
    int64_t splits = out_tiles >= slots ? 1 : slots / out_tiles;
    if (splits > tiles) splits = tiles;
    plan.splits = static_cast<int>(splits < 1 ? 1 : splits);
    const int64_t groups = out_tiles * plan.splits;
    const int64_t rounds = (groups + slots - 1) / slots;
    const double fill = static_cast<double>(groups) / static_cast<double>(rounds * slots);
    if (fill > best_fill + 1e-9) best = plan, best_fill = fill;
  }
  return best;
}

inline int launch_wgrad(const GemmArgs& p, const WgradPlan& plan, hipStream_t st) {
  const int np = p.n_problems, splits = plan.splits;
  if (p.rb <= 64) return launch_tiles<128, 64, 2, 2, false, false>(p, np, splits, st);
  switch (plan.variant) {
    case 2: return launch_tiles<128, 256, 2, 4, false, false>(p, np, splits, st);
    case 4: return launch_tiles<256, 256, 4, 4, false, false, true>(p, np, splits, st);
    case 6: {
      GemmArgs q = p;
      q.tiles_n = (p.rb + 255) / 256;
      dim3 grid((p.ra + 255) / 256, q.tiles_n * np, splits);
      wgrad_stream_kernel<><<<grid, 1024, 0, st>>>(q);
      return launch_status();
    }
    default: return launch_tiles<128, 128, 2, 4, false, false>(p, np, splits, st);   // 1
  }
}

}  // namespace
}  // namespace gts
