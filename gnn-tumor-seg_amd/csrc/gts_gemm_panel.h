// K11 row panels on v_mfma_f32_16x16x4_f32 with direct-to-fragment buffer loads: the panel kernel, its chained
// second stage, the launcher with its compile-time epilogues and the panel-height heuristic.  Included by gts_gemm.hip
// and tools/diag/gemm_probe.hip (the rejected LDS-staged panels of tools/diag/gemm_rejected_forms.inc build on it).
#pragma once
#include <type_traits>

#include "gts_gemm_args.h"

namespace gts {
namespace {

// ---- 240-row panels on v_mfma_f32_16x16x4_f32 -------------------------------------------------
// The layer GEMMs of the path have 60 000 (or 120 000) rows and 256 columns: with 256-row tiles
// that is 235 workgroups for 256 CUs — 21 CUs idle and every busy CU carrying 256 rows where
// 234.4 would do.  Row panels of 240 = 15 x 16 rows make it 250 workgroups of 240 rows (60 000 =
// 250 x 240 exactly): -6 % rows per CU.  240 is not a multiple of 32, so this kernel is built
// on the 16x16x4 MFMA (same flops per cycle as 32x32x2, exact fp32): 12 waves (3 x 4), one
// wave = 80 x 64 outputs = 5 x 4 tiles, 3 waves per SIMD, 5 x 4 x 4 = 80 accumulator registers.
// Forward form only (both operands reduction-contiguous; input gradients reach it through
// transposed weights).  Reduction index consumed by MFMA step (g, j) on lane quarter q:
// 16 g + 4 q + j for both operands.  (The first form of these panels staged its operands through
// two LDS images per operand, one barrier per reduction tile: tools/diag/gemm_rejected_forms.inc,
// which also uses the constants below.)
typedef float v4acc __attribute__((ext_vector_type(4)));

constexpr int kR240 = 240, kC240 = 256, kWm240 = 3, kWn240 = 4, kThreads240 = 64 * kWm240 * kWn240;
constexpr int kTm240 = kR240 / kWm240 / 16, kTn240 = kC240 / kWn240 / 16;   // 5 x 4 tiles per wave
constexpr int kStage240 = 16 * (kC240 / kWn240 + 4);                       // per-wave epilogue patch [16][68]

// ---- 240-row panels, operands straight into MFMA fragments (no LDS staging, no barriers) --------
// 240 x 256 outputs per workgroup on the 16x16x4 MFMA (a form that staged the panels through LDS is in tools/diag); a
// lane fetches its own fragments from global memory: lane (i, q) of a wave needs
// A[row i][16 g + 4 q .. + 3] — one 16-byte buffer load — and the 16 lanes of a quarter cover 16
// rows x 64 contiguous bytes.  No LDS images, no stash, no barrier: the waves of a workgroup are
// independent instruction streams, one wave's wait for memory is another wave's MFMA time, and
// the store burst of the epilogue spreads out the same way.  DEPTH + 1 register sets of fragments:
// the loads of reduction groups g+1 .. g+DEPTH are in flight under the MFMAs of group g.
//   WM x WN = 3 x 4: twelve waves of 80 x 64 outputs (3 per SIMD, 80 accumulator registers); every
//             A row is fetched by four waves and every weight row by three (L1 / L2 hits, but
//             42 B/clk of L1 traffic per CU);
//   WM x WN = 1 x 4: four waves of 240 x 64 outputs, ONE per SIMD with 240 accumulator registers and
//             the whole 512-register file: every A element is fetched exactly once per workgroup,
//             10 B/clk of L1 traffic, and a group of 240 MFMAs (3.2 us) covers the next loads.
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// TM + TN 16-byte buffer loads: address = panel base (SGPR resource) + lane offset (one VGPR per
// fragment row block) + reduction offset (SGPR); offsets past the panel's bytes read as 0
// (`group` = reduction group of 16; the activation panel advances 64 bytes per group, the weights `b_step` bytes: 64 as
// stored by torch, 1024 in fragment order)
template <int TM, int TN, bool B_FIRST = false, int B_STEP = 64>
__device__ __forceinline__ void load_fragments(v4f (&af)[TM], v4f (&bf)[TN], __amdgpu_buffer_rsrc_t ra,
                                               __amdgpu_buffer_rsrc_t rb, const unsigned (&off_a)[TM],
                                               const unsigned (&off_b)[TN], int group) {
  const int k_bytes = 64 * group, kb_bytes = B_STEP * group;
  if constexpr (B_FIRST) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
      bf[tn] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rb, off_b[tn], kb_bytes, 0));
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
      af[tm] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(ra, off_a[tm], k_bytes, 0));
    return;
  }
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
    af[tm] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(ra, off_a[tm], k_bytes, 0));
#pragma unroll
  for (int tn = 0; tn < TN; ++tn)
    bf[tn] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rb, off_b[tn], kb_bytes, 0));
}

template <int TM, int TN>
__device__ __forceinline__ void mfma_group(v4acc (&acc)[TM][TN], const v4f (&af)[TM], const v4f (&bf)[TN]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[tm][j], bf[tn][j], acc[tm][tn], 0, 0, 0);
}

struct PanelStage {   // one GEMM of the panel kernel: c[rows of the panel, rb] = act(a0 b0^T + a1 b1^T + bias) (. mask)
  const float* a[2];
  const float* b[2];
  const float* bp[2];   // b[seg] in fragment order, or null (GemmArgs::bp)
  int lda[2], ldb[2], kseg[2];
  int ra, rb, ldc, relu;
  float* c;
  const float* bias;
  const float* mask;
  const float* sc_l;   // optional score vectors / partial-score outputs (see GemmArgs)
  const float* sc_r;
  float* sc_el;
  float* sc_er;
  unsigned long long* bits_out;        // optional: sign bits of c (see GemmArgs)
  const unsigned long long* bits_in;   // optional: `mask` as bits
  int mask_kind;                       // 0: ReLU mask, 1: ELU derivative through `mask` (see GemmArgs)
  float* col_partial;                  // optional: column sums per wave row block
};

// What the epilogue of a stage does, as template bits: with kEpiRuntime every switch is read from the arguments
// (any shape); without it the switches are compile-time facts and the output is whole 256-column blocks
// (host-checked) — the epilogue of the layer-stack launches loses its ~50 uniform branches per 16 rows and
// most of its code (the generic kernel is ~100 KB of instructions, more than the instruction cache).
enum : int { kEpiBias = 1, kEpiRelu = 2, kEpiMaskBits = 4, kEpiScores = 8, kEpiBitsOut = 16, kEpiEluSums = 32, kEpiRuntime = 256, kEpiAbsent = -1 };

template <int WM, int WN, int DEPTH, int F = kEpiRuntime, int ROWS = kR240, int ILV = 0, bool PK = false>
__device__ __forceinline__ void panel_stage(const PanelStage s, float* lds, int sched, int m0, int n0, int row_end) {
  constexpr bool G = (F & kEpiRuntime) != 0;
  constexpr int WTM = ROWS / WM, WTN = kC240 / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int R = DEPTH + 1;                     // register sets of fragments
  constexpr int kLd = WTN + 4, kStage = 16 * kLd;  // per-wave epilogue patch [16][WTN + 4]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave index in an SGPR
  const int wm = wave / WN, wn = wave % WN;
  const int i16 = lane & 15, q = lane >> 4;

  v4acc acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = v4acc{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int seg = 0; seg < 2; ++seg) {
    const int kseg = s.kseg[seg];
    if (kseg == 0) continue;
    const int lda = s.lda[seg], ldb = s.ldb[seg];
    // buffer resources over this workgroup's operand panels: rows [m0, row_end) of A, weight rows
    // [n0, n0 + 256) — anything past their last byte reads as 0 (no row clamps, no branches)
    const int cols = min(s.rb - n0, kC240);
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(s.a[seg] + static_cast<size_t>(m0) * lda), 0, (row_end - m0) * lda * 4, 0x00020000);
    // PK: the weights come in fragment order (s.bp): [16-row tile of B][reduction group of 16][lane][4 floats], zero-padded
    // to whole tiles and groups — a fragment is 1 KiB of consecutive bytes, lane l takes bytes 16 l .. 16 l + 15.  A
    // compile-time fact of the instantiation (a run-time choice between the two address forms cost 240 spilled registers)
    constexpr int b_step = PK ? 1024 : 64;
    const int groups = (kseg + 15) >> 4;
    __amdgpu_buffer_rsrc_t rb;
    unsigned off_a[TM], off_b[TN];
    if constexpr (PK) {
      rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(s.bp[seg]), 0, ((s.rb + 15) >> 4) * groups * 1024, 0x00020000);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) off_b[tn] = (static_cast<unsigned>((n0 + wn * WTN) / 16 + tn) * groups * 64 + lane) * 16;
    } else {
      rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(s.b[seg] + static_cast<size_t>(n0) * ldb), 0, cols * ldb * 4,
                                             0x00020000);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) off_b[tn] = (static_cast<unsigned>(wn * WTN + tn * 16 + i16) * ldb + 4 * q) * 4;
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) off_a[tm] = (static_cast<unsigned>(wm * WTM + tm * 16 + i16) * lda + 4 * q) * 4;
    const int n_full = kseg / 16, tail = kseg % 16;
    v4f af[R][TM], bf[R][TN];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u)     // groups 0 .. DEPTH-1 (clamped: re-reads are harmless)
      if (n_full > 0) load_fragments<TM, TN, false, b_step>(af[u], bf[u], ra, rb, off_a, off_b, min(u, n_full - 1));
    int g = 0;
    for (; g + R <= n_full; g += R) {
#pragma unroll
      for (int u = 0; u < R; ++u) {
        load_fragments<TM, TN, ILV >= 0, b_step>(af[(u + DEPTH) % R], bf[(u + DEPTH) % R], ra, rb, off_a, off_b,
                                                 min(g + u + DEPTH, n_full - 1));
        mfma_group(acc, af[u], bf[u]);
      }
      // pin the software pipeline: the loads of a group are issued before the MFMAs of the group
      // DEPTH in front of it (left alone, the scheduler sinks them to save registers and the wave
      // then waits for each load right after issuing it)
#pragma unroll
      for (int u = 0; u < R; ++u) {
        if constexpr (ILV < 0) {   // the loads of a group in one burst in front of its MFMAs (rounds 1 - 2; kept for A/B runs)
          __builtin_amdgcn_sched_group_barrier(0x020, TM + TN, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 4 * TM * TN, 0);
        } else {   // one load, then kPer MFMAs, ...: a burst of nine loads holds up the wave's own MFMA issue (round 3)
          constexpr int kPer = ILV > 0 ? ILV : 4 * TM * TN / (TM + TN);
          constexpr int kRest = 4 * TM * TN - kPer * (TM + TN);
          static_assert(kPer >= 1 && kRest >= 0, "MFMAs per load do not fit the group");
#pragma unroll
          for (int l = 0; l < TM + TN; ++l) {
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, kPer, 0);
          }
          if (kRest > 0) __builtin_amdgcn_sched_group_barrier(0x008, kRest, 0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < R - 1; ++u) {   // the last n_full % R groups: their fragments are already on the way
      if (g + u < n_full) {
        if (g + u + DEPTH < n_full)
          load_fragments<TM, TN, false, b_step>(af[(u + DEPTH) % R], bf[(u + DEPTH) % R], ra, rb, off_a, off_b, g + u + DEPTH);
        mfma_group(acc, af[u], bf[u]);
      }
    }
    if (tail != 0) {   // kseg is a multiple of 4: quarter q lies inside the tail or past the row's end
      if (4 * q >= tail) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) off_a[tm] = kOutOfRange;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) off_b[tn] = kOutOfRange;
      }
      load_fragments<TM, TN, false, b_step>(af[0], bf[0], ra, rb, off_a, off_b, n_full);
      mfma_group(acc, af[0], bf[0]);
    }
  }

  // Epilogue: a row of TN tiles (16 x WTN outputs) through the wave's LDS
  // patch, out as 16-byte row segments with bias / ReLU / mask applied as float4.
  float* stage = lds + wave * kStage;
  const bool wide = G ? (s.rb & 3) == 0 && (s.ldc & 3) == 0 : true;
  constexpr int kC4 = WTN / 4;                // float4 per patch row
  constexpr int kRowsPerIt = 64 / kC4;        // patch rows one pass of the wave covers
  const int c4 = (lane % kC4) * 4, rsub = lane / kC4;
  const int col = n0 + wn * WTN + c4;
  const bool col_ok = G ? col < s.rb : true;
  const bool has_bias = G ? s.bias != nullptr : (F & kEpiBias) != 0;
  const bool relu = G ? s.relu != 0 : (F & kEpiRelu) != 0;
  const bool scores = G ? s.sc_l != nullptr : (F & kEpiScores) != 0;
  v4f bias = {0.f, 0.f, 0.f, 0.f};
  if (wide && has_bias && col_ok) bias = *reinterpret_cast<const v4f*>(s.bias + col);
  v4f sc_wl = {0.f, 0.f, 0.f, 0.f}, sc_wr = sc_wl;
  if (wide && scores && col_ok) {
    sc_wl = *reinterpret_cast<const v4f*>(s.sc_l + col);
    sc_wr = *reinterpret_cast<const v4f*>(s.sc_r + col);
  }
  // ReLU masks as bits (GemmArgs::bits_out / bits_in): this wave's TM * 4 row groups of its 64-column block are
  // TM * 16 consecutive words of the [column block][row group][4] layout
  constexpr int kBitWords = TM * 16;
  static_assert(G || WTN == 64, "the compile-time epilogues keep mask bits: 64-column wave tiles");
  const bool bits_here = G ? WTN == 64 && wide && n0 + wn * WTN < s.rb : true;
  const bool bit_mask = G ? bits_here && s.bits_in != nullptr && s.mask != nullptr : (F & kEpiMaskBits) != 0;
  const bool bits_wanted = G ? bits_here && s.bits_out != nullptr : (F & kEpiBitsOut) != 0;
  const size_t bits_at = (static_cast<size_t>((n0 + wn * WTN) >> 6) * ((s.ra + 3) >> 2) + ((m0 + wm * WTM) >> 2)) * 4;
  unsigned long long* bit_words = reinterpret_cast<unsigned long long*>(lds + WM * WN * kStage) + wave * kBitWords;
  const bool elu_mask = G ? s.mask_kind == 1 : (F & kEpiEluSums) != 0;
  const bool col_sums = G ? s.col_partial != nullptr : (F & kEpiEluSums) != 0;
  v4f csum = {0.f, 0.f, 0.f, 0.f};   // this lane's four columns over the rows it stores (rsub, rsub + 4, ...: fixed order)
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int row_base = m0 + wm * WTM + tm * 16;
    if (wide) {
      v4f mk[16 / kRowsPerIt];
      const bool float_mask = G ? s.mask != nullptr && !bit_mask : (F & kEpiEluSums) != 0;
      if (float_mask) {
#pragma unroll
        for (int it = 0; it < 16 / kRowsPerIt; ++it) {
          const int row = row_base + it * kRowsPerIt + rsub;
          mk[it] = (row < row_end && col_ok)
                       ? *reinterpret_cast<const v4f*>(s.mask + static_cast<size_t>(row) * s.ldc + col)
                       : v4f{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[(4 * q + r) * kLd + tn * 16 + i16] = acc[tm][tn][r];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int it = 0; it < 16 / kRowsPerIt; ++it) {
        const int lrow = it * kRowsPerIt + rsub, row = row_base + lrow;
        v4f val = *reinterpret_cast<const v4f*>(stage + lrow * kLd + c4) + bias;
        // four rows x 64 columns per pass: their four mask words (bit = lane) sit at one wave-uniform
        // address — scalar loads, which do not queue behind this wave's stores as vector loads do
        if (bit_mask && row_base + it * kRowsPerIt < row_end) {
          const unsigned long long* words = s.bits_in + bits_at + (tm * (16 / kRowsPerIt) + it) * 4;
#pragma unroll
          for (int e = 0; e < 4; ++e) val[e] = (words[e] >> lane) & 1ull ? val[e] : 0.f;
        }
        if (row < row_end && col_ok) {
          if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) val[e] = relu_f32(val[e]);
          }
          if (float_mask) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              val[e] = mk[it][e] > 0.f ? val[e] : elu_mask ? val[e] * (mk[it][e] + 1.0f) : 0.f;
          }
          if (col_sums) csum += val;
          v4f* dst = reinterpret_cast<v4f*>(s.c + static_cast<size_t>(row) * s.ldc + col);
          if (G && (sched & 2)) __builtin_nontemporal_store(val, dst);
          else *dst = val;
        }
        if (bits_wanted) {   // one wave-wide comparison per element slot = one word; collected in LDS, stored once
          const unsigned long long w0 = __ballot(val[0] > 0.f), w1 = __ballot(val[1] > 0.f);
          const unsigned long long w2 = __ballot(val[2] > 0.f), w3 = __ballot(val[3] > 0.f);
          if (lane < 4) bit_words[(tm * (16 / kRowsPerIt) + it) * 4 + lane] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
        }
        if (scores) {   // rb is a multiple of WTN here: every lane's columns are real
          float pl = (val[0] * sc_wl[0] + val[1] * sc_wl[1]) + (val[2] * sc_wl[2] + val[3] * sc_wl[3]);
          float pr = (val[0] * sc_wr[0] + val[1] * sc_wr[1]) + (val[2] * sc_wr[2] + val[3] * sc_wr[3]);
#pragma unroll
          for (int o = 1; o < kC4; o <<= 1) pl += __shfl_xor(pl, o, kWave), pr += __shfl_xor(pr, o, kWave);
          if (lane % kC4 == 0 && row < row_end) {
            const size_t at = static_cast<size_t>(row) * (s.rb / WTN) + (n0 / WTN + wn);
            s.sc_el[at] = pl, s.sc_er[at] = pr;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    } else {
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int c = n0 + wn * WTN + tn * 16 + i16;
        const float bs = (s.bias != nullptr && c < s.rb) ? s.bias[c] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row_base + 4 * q + r;
          if (row < row_end && c < s.rb) {
            const size_t off = static_cast<size_t>(row) * s.ldc + c;
            float val = acc[tm][tn][r] + bs;
            if (s.relu) val = relu_f32(val);
            if (s.mask != nullptr) val = s.mask[off] > 0.f ? val : 0.f;
            s.c[off] = val;
          }
        }
      }
    }
  }
  static_assert(kC4 == 16 || !(F & kEpiEluSums), "column sums: 64-column wave tiles");
  if (col_sums && wide && kC4 == 16) {   // the four row residues of a column group sit 16 lanes apart: two fixed-order exchanges
#pragma unroll
    for (int e = 0; e < 4; ++e) csum[e] += __shfl_xor(csum[e], 16, kWave);
#pragma unroll
    for (int e = 0; e < 4; ++e) csum[e] += __shfl_xor(csum[e], 32, kWave);
    if (lane < kC4 && col_ok)
      *reinterpret_cast<v4f*>(s.col_partial + static_cast<size_t>((m0 / ROWS) * WM + wm) * s.rb + col) = csum;
  }
  if (bits_wanted) {
    __builtin_amdgcn_wave_barrier();
    const int valid = min(kBitWords, ((row_end - (m0 + wm * WTM) + 3) >> 2) * 4);   // words of rows that exist
#pragma unroll
    for (int base = 0; base < kBitWords; base += 64)
      if (base + lane < valid) s.bits_out[bits_at + base + lane] = bit_words[base + lane];
    __builtin_amdgcn_wave_barrier();
  }
}

template <int WM, int WN, int DEPTH, class Probe = NoProbe, int F1 = kEpiRuntime, int F2 = kEpiRuntime, int ROWS = kR240, int ILV = 0,
          bool PK = false>
__global__ __launch_bounds__(64 * WM * WN, WM * WN / 4) void gemm_panel_direct_kernel(const GemmArgs p) {
  constexpr int WTN = kC240 / WN;
  static_assert((ROWS / WM) % 16 == 0 && WTN % 16 == 0 && WTN % 4 == 0 && (WM * WN) % 4 == 0, "wave tiles are whole 16x16 tiles");
  // epilogue patches [16][WTN + 4] per wave, then the waves' mask words (ROWS / WM / 16 * 16 of 8 bytes each)
  __shared__ __attribute__((aligned(16))) float lds[WM * WN * 16 * (WTN + 4) + WM * WN * (ROWS / WM) * 2];
  const int m0 = blockIdx.x * ROWS, n0 = blockIdx.y * kC240;
  const int row_end = min(p.ra, m0 + ROWS);
  Probe::mark(0);
  Probe::mark(1);
  PanelStage s0{};
  s0.a[0] = p.a[0], s0.a[1] = p.a[1], s0.b[0] = p.b[0], s0.b[1] = p.b[1], s0.bp[0] = p.bp[0], s0.bp[1] = p.bp[1];
  s0.lda[0] = p.lda[0], s0.lda[1] = p.lda[1], s0.ldb[0] = p.ldb[0], s0.ldb[1] = p.ldb[1];
  s0.kseg[0] = p.kseg[0], s0.kseg[1] = p.kseg[1];
  s0.ra = p.ra, s0.rb = p.rb, s0.ldc = p.ldc, s0.relu = p.relu, s0.c = p.c, s0.bias = p.bias, s0.mask = p.mask;
  s0.sc_l = p.sc_l, s0.sc_r = p.sc_r, s0.sc_el = p.sc_el, s0.sc_er = p.sc_er;
  s0.bits_out = p.bits_out, s0.bits_in = p.bits_in, s0.mask_kind = p.mask_kind, s0.col_partial = p.col_partial;
  panel_stage<WM, WN, DEPTH, F1, ROWS, ILV, PK>(s0, lds, p.sched, m0, n0, row_end);
  Probe::mark(2);
  // With c2 set a second GEMM follows in the same launch: the rows this workgroup has just stored are
  // its A operand (the next layer's fc_pool behind fc_self + fc_neigh; the next input gradient behind
  // this one) — one launch, one cold start and one output burst less per layer, and the operand
  // comes back out of this CU's own L2 slice.
  if (F2 != kEpiAbsent && ((F2 & kEpiRuntime) == 0 || p.c2 != nullptr)) {
    // Stage 2 re-reads rows of c that OTHER waves of this workgroup stored.  Ordering: every wave's vmcnt(0), then the
    // workgroup barrier.  That is enough because the workgroup runs on one CU whose vector L1 all its waves share
    // (the default, non-tgsplit execution mode) and the stores are ordinary ones (the launcher never combines
    // non-temporal stores, sched bit 2, with a second stage).
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's rows of c are in memory ...
    __threadfence_block();
    __syncthreads();                       // ... and so are every other wave's, before any is read back
    PanelStage s1{};
    s1.a[0] = p.c, s1.a[1] = p.c, s1.b[0] = p.b2, s1.b[1] = p.b2, s1.bp[0] = p.bp2, s1.bp[1] = nullptr;
    s1.lda[0] = s1.lda[1] = p.ldc, s1.ldb[0] = s1.ldb[1] = p.ldb2;
    s1.kseg[0] = p.rb, s1.kseg[1] = 0;
    s1.ra = p.ra, s1.rb = p.rb2, s1.ldc = p.ldc2, s1.relu = p.relu2, s1.c = p.c2, s1.bias = p.bias2, s1.mask = nullptr;
    panel_stage<WM, WN, DEPTH, F2 == kEpiAbsent ? kEpiRuntime : F2, ROWS, ILV, PK>(s1, lds, p.sched, m0, 0, row_end);
  }
  Probe::mark(3);
}

// the instantiation that reads its weights in fragment order when the call brought a copy of EVERY weight operand
// (GemmArgs::bp / bp2), else the one that reads them as stored
#define GTS_PANEL_LAUNCH(F1_, F2_, ILV_)                                                                   \
  do {                                                                                                    \
    if (all_packed) gemm_panel_direct_kernel<3, 4, 1, NoProbe, F1_, F2_, ROWS, ILV_, true><<<grid, 768, 0, st>>>(q);   \
    else gemm_panel_direct_kernel<3, 4, 1, NoProbe, F1_, F2_, ROWS, ILV_, false><<<grid, 768, 0, st>>>(q);             \
    return launch_status();                                                                               \
  } while (0)

template <int WM, int WN, int DEPTH, class Probe = NoProbe, int ROWS = kR240>
int launch_panel_direct(const GemmArgs& p, hipStream_t st) {
  dim3 grid((p.ra + ROWS - 1) / ROWS, (p.rb + kC240 - 1) / kC240, 1);
  GemmArgs q = p;
  q.sched = g_gemm_sched;
  if (p.c2 != nullptr) q.sched &= ~2;   // chained launches read their own output back through L1 / L2: ordinary stores only
  const bool all_packed = p.bp[0] != nullptr && (p.kseg[1] == 0 || p.bp[1] != nullptr) && (p.c2 == nullptr || p.bp2 != nullptr) &&
                          !(q.sched & 16);   // GTS_OPT_GEMM_SCHED bit 16: ignore the copies (A/B runs)
  if constexpr (WM == 3 && WN == 4 && DEPTH == 1 && std::is_same<Probe, NoProbe>::value) {
    // the launches of the SAGE-pool layer stack at its 256-wide layers: compile-time epilogues
    const bool whole_cols = p.rb % kC240 == 0 && p.ldc % 4 == 0 && (p.mask == nullptr || p.bits_in != nullptr) &&
                            (p.c2 == nullptr || (p.rb2 % kC240 == 0 && p.ldc2 % 4 == 0)) && !(q.sched & 2) && !(q.sched & 4);
    const bool whole = whole_cols && p.sc_l == nullptr && p.mask_kind == 0 && p.col_partial == nullptr;
    if (p.rb % kC240 == 0 && p.ldc % 4 == 0 && p.mask_kind == 1 && p.mask != nullptr && p.col_partial != nullptr &&
        p.bits_in == nullptr && p.bits_out == nullptr && p.sc_l == nullptr && p.c2 == nullptr && p.bias == nullptr &&
        !p.relu && !(q.sched & 6)) {   // an input gradient through the ELU of the layer below, with that layer's bias gradient
      GTS_PANEL_LAUNCH(kEpiEluSums, kEpiAbsent, 0);
    }
    const int f1 = (p.bias ? kEpiBias : 0) | (p.relu ? kEpiRelu : 0) | (p.mask ? kEpiMaskBits : 0) | (p.bits_out ? kEpiBitsOut : 0);
    const int f2 = p.c2 == nullptr ? kEpiAbsent : (p.bias2 ? kEpiBias : 0) | (p.relu2 ? kEpiRelu : 0);
    constexpr int kFwd = kEpiBias | kEpiRelu;
    if (whole && f1 == (kFwd | kEpiBitsOut) && f2 == kFwd) {          // fc_self + fc_neigh, then the next fc_pool (training)
      if constexpr (ROWS == kR240) {
        if (q.sched & 8) {   // A/B: the grouped load order of rounds 1 - 2
          gemm_panel_direct_kernel<3, 4, 1, NoProbe, kFwd | kEpiBitsOut, kFwd, ROWS, -1><<<grid, 768, 0, st>>>(q);
          return launch_status();
        }
      }
      GTS_PANEL_LAUNCH(kFwd | kEpiBitsOut, kFwd, 0);
    }
    if (whole && f1 == kEpiMaskBits && f2 == 0) {                     // a layer's input gradient, then g @ W_neigh below
      if constexpr (ROWS == kR240) {
        if (q.sched & 8) {   // A/B: the grouped load order of rounds 1 - 2
          gemm_panel_direct_kernel<3, 4, 1, NoProbe, kEpiMaskBits, 0, ROWS, -1><<<grid, 768, 0, st>>>(q);
          return launch_status();
        }
      }
      GTS_PANEL_LAUNCH(kEpiMaskBits, 0, 0);
    }
    if (whole && f1 == kFwd && f2 == kFwd) {                          // the same pair without mask bits (no-grad forward: inference, evaluate)
      GTS_PANEL_LAUNCH(kFwd, kFwd, 0);
    }
    if (whole && f1 == kFwd && f2 == kEpiAbsent) {                    // one biased ReLU layer on its own (fc_pool of the first wide layer)
      GTS_PANEL_LAUNCH(kFwd, kEpiAbsent, 0);
    }
    if (whole_cols && p.sc_l != nullptr && f1 == 0 && f2 == kEpiAbsent) {   // GATConv's fc with the attention scores in its epilogue
      GTS_PANEL_LAUNCH(kEpiScores, kEpiAbsent, 0);
    }
    if (whole && f1 == 0 && f2 == kEpiAbsent) {                       // a plain product (g @ W_neigh of the top layer)
      GTS_PANEL_LAUNCH(0, kEpiAbsent, 0);
    }
    GTS_PANEL_LAUNCH(kEpiRuntime, kEpiRuntime, 0);
  }
  gemm_panel_direct_kernel<WM, WN, DEPTH, Probe, kEpiRuntime, kEpiRuntime, ROWS><<<grid, 64 * WM * WN, 0, st>>>(q);
  return launch_status();
}
#undef GTS_PANEL_LAUNCH

// Height of the row panels the direct-to-fragment kernel (variant 10) cuts `rows` into.  One workgroup per CU per
// round, so a CU walks rounds x height rows: 240 rows suit 60 000 (250 panels) and 120 000 rows (500 = two rounds),
// but 35 000 rows (the reference's real batches: 6 graphs of ~6k nodes) are 146 panels of 240 on 256 CUs; 144-row
// panels (243 of them) fill the chip.  Candidates 240 / 192 / 144 (5 / 4 / 3 MFMA row blocks per wave); the taller
// panel wins ties (fewer loads per MFMA).  The result of a row does not depend on the height (same reduction order).
inline int panel_rows_for(int64_t rows, int64_t col_blocks) {
  if (g_panel_rows == 240 || g_panel_rows == 192 || g_panel_rows == 144) return g_panel_rows;
  int best = kR240;
  int64_t best_cost = -1;
  for (int h : {240, 192, 144}) {
    const int64_t panels = (rows + h - 1) / h * col_blocks;
    const int64_t cost = (panels + 255) / 256 * h;
    if (best_cost < 0 || cost < best_cost) best = h, best_cost = cost;
  }
  return best;
}

}  // namespace
}  // namespace gts
