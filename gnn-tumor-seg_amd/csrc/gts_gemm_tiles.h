// K11: dense fp32 layer GEMMs on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32,
// 157 TF peak — the ONLY MFMA use of the path; gfx950 has no xf32/TF32).
//
// One tiled kernel serves the three GEMMs of a layer; what differs is only how each operand
// is laid out with respect to the reduction index kk:
//     C[ra, rb] = sum_kk  A(ra, kk) * B(rb, kk)
//   forward      out[M,N] = act[M,K] . W[N,K]^T (+ second pair) + bias, ReLU
//                A = act  (kk contiguous),  B = W   (kk contiguous)
//   input grad   gin[M,K] = g[M,N] . W[N,K]   (+ second pair), optional ReLU mask on gin
//                A = g    (kk contiguous),  B = W   (kk strided: B(k, n) = W[n*K + k])
//   weight grad  gw[N,K]  = g[M,N]^T . act[M,K]   (reduction over the 60 000 nodes, split
//                over blockIdx.z into per-split slabs that a second kernel sums in a fixed
//                order -> bitwise reproducible, no float atomics); up to 4 same-shape
//                problems share one launch (the three weight gradients of a SAGE layer);
//                A = g    (kk strided: A(n, m) = g[m*N + n]),  B = act (kk strided)
//                + the bias gradient (column sums of g) from the A fragments on the way.
//
// Tile: BM x BN outputs per workgroup of WM x WN waves, each wave (BM/WM)x(BN/WN) = TMxTN
// 32x32 MFMA tiles, reduction in steps of 32.  Global -> registers (16 B/lane, issued one
// tile ahead, in flight under the MFMAs) -> LDS (ds_write_b128) -> fragments.  LDS images:
//   kk-contiguous operand: [rows][36]  (32 + 4 pad floats: ds_read_b128 of 4 consecutive kk per
//                          lane is conflict-free for any 16 rows distinct mod 16);
//   kk-strided operand:    [32][rows]  (ds_read_b32, lanes on consecutive addresses).
// The reduction index consumed by MFMA step (g, j) on lane-half h is 8g + 4h + j for both
// operands — a permutation of kk inside each 8-block, free for a sum, chosen so that the
// contiguous operand needs ONE 16-byte LDS read per four MFMAs.
//
// This header: the LDS operand images, the shared epilogue, the 32x32x2 tile kernel and its launcher.  Included by
// gts_gemm.hip (forward / input gradient), gts_gemm_wgrad.h (split reduction) and tools/diag/gemm_probe.hip.
#pragma once
#include "gts_gemm_args.h"

namespace gts {
namespace {

constexpr int kKcLd = kBK + 4;  // padded row of a kk-contiguous LDS image

template <int ROWS, bool KC, int THREADS>
struct OperandTile {
  static constexpr int kFloats = KC ? ROWS * kKcLd : kBK * ROWS;
  static constexpr int kVec = ROWS * kBK / 4 / THREADS;  // float4 per thread per tile
  static_assert(ROWS * kBK / 4 % THREADS == 0 && kVec >= 1, "tile must divide over the workgroup");

  // global -> registers.  `row0` first row of the tile, `k0` first reduction index.
  __device__ __forceinline__ static void load(v4f (&reg)[kVec], const float* __restrict__ p, int ld,
                                              int row0, int k0, int n_rows, int n_k) {
#pragma unroll
    for (int q = 0; q < kVec; ++q) {
      const int idx = threadIdx.x + THREADS * q;
      int r, kk;
      if constexpr (KC) {
        r = idx >> 3, kk = (idx & 7) * 4;  // 8 float4 per 32-wide row
      } else {
        kk = idx / (ROWS / 4), r = (idx % (ROWS / 4)) * 4;
      }
      const int gr = row0 + r, gk = k0 + kk;
      const bool ok = gr < n_rows && gk < n_k;  // dims are multiples of 4: all-or-nothing
      const size_t off = KC ? static_cast<size_t>(gr) * ld + gk : static_cast<size_t>(gk) * ld + gr;
      reg[q] = ok ? *reinterpret_cast<const v4f*>(p + off) : v4f{0.f, 0.f, 0.f, 0.f};
    }
  }

  __device__ __forceinline__ static void store(const v4f (&reg)[kVec], float* lds) {
#pragma unroll
    for (int q = 0; q < kVec; ++q) {
      const int idx = threadIdx.x + THREADS * q;
      int off;
      if constexpr (KC) {
        off = (idx >> 3) * kKcLd + (idx & 7) * 4;
      } else {
        off = (idx / (ROWS / 4)) * ROWS + (idx % (ROWS / 4)) * 4;
      }
      *reinterpret_cast<v4f*>(lds + off) = reg[q];
    }
  }

  // fragment for the 32-row MFMA tile starting at `row` of the image, k-group g:
  // out[j] feeds MFMA step j (reduction index 8g + 4h + j)
  __device__ __forceinline__ static void fragment(float (&out)[4], const float* lds, int row, int g) {
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    if constexpr (KC) {
      const v4f t = *reinterpret_cast<const v4f*>(lds + (row + i) * kKcLd + g * 8 + 4 * h);
      out[0] = t[0], out[1] = t[1], out[2] = t[2], out[3] = t[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = lds[(g * 8 + 4 * h + j) * ROWS + row + i];
    }
  }
};

// Epilogue shared by the GEMM kernels.  C/D layout of the 32x32 MFMA: col = lane & 31,
// row = (r&3) + 8*(r>>2) + 4*(lane>>5).  `lds` is the (now dead) operand area.
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void write_tile(const GemmArgs& p, float* lds, float* c,
                                           v16f (&acc)[BM / WM / 32][BN / WN / 32], int m0, int n0) {
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int i = lane & 31, h = lane >> 5;
  if ((p.rb & 3) == 0 && (p.ldc & 3) == 0) {
    // Wide path: each 32x32 accumulator tile goes through a per-wave [32][36] LDS patch (the
    // operand images are dead after the loop's last barrier) and leaves as 16-byte-per-lane row
    // segments: 4x fewer store instructions, and bias / ReLU mask arrive as float4 too.
    float* stage = lds + wave * (32 * kKcLd);
    const int srow = lane >> 3, c4 = (lane & 7) * 4;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int col = n0 + wn * WTN + tn * 32 + c4;
      const bool col_ok = col < p.rb;
      v4f bias = {0.f, 0.f, 0.f, 0.f};
      if (p.bias != nullptr && col_ok) bias = *reinterpret_cast<const v4f*>(p.bias + col);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        // the ReLU mask of this tile is requested first: its latency hides behind the LDS staging
        v4f mk[4];
        if (p.mask != nullptr) {
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            const int row = m0 + wm * WTM + tm * 32 + it * 8 + srow;
            mk[it] = (row < p.ra && col_ok)
                         ? *reinterpret_cast<const v4f*>(p.mask + static_cast<size_t>(row) * p.ldc + col)
                         : v4f{0.f, 0.f, 0.f, 0.f};
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * h) * kKcLd + i] = acc[tm][tn][r];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int lrow = it * 8 + srow;
          v4f val = *reinterpret_cast<const v4f*>(stage + lrow * kKcLd + c4) + bias;
          const int row = m0 + wm * WTM + tm * 32 + lrow;
          if (row < p.ra && col_ok) {
            const size_t off = static_cast<size_t>(row) * p.ldc + col;
            if (p.relu) {
#pragma unroll
              for (int e = 0; e < 4; ++e) val[e] = relu_f32(val[e]);
            }
            if (p.mask != nullptr) {
#pragma unroll
              for (int e = 0; e < 4; ++e) val[e] = mk[it][e] > 0.f ? val[e] : 0.f;
            }
            *reinterpret_cast<v4f*>(c + off) = val;
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  } else {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int col = n0 + wn * WTN + tn * 32 + i;
      const float bias = (p.bias != nullptr && col < p.rb) ? p.bias[col] : 0.f;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * WTM + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (row < p.ra && col < p.rb) {
            const size_t off = static_cast<size_t>(row) * p.ldc + col;
            float val = acc[tm][tn][r] + bias;
            if (p.relu) val = relu_f32(val);
            if (p.mask != nullptr) val = p.mask[off] > 0.f ? val : 0.f;
            c[off] = val;
          }
        }
      }
    }
  }
}

// waves per SIMD to plan registers for: two co-resident workgroups when the accumulators allow
constexpr int min_waves_per_simd(int wm, int wn, int tm, int tn) {
  const int per_block = wm * wn / 4;                       // waves per SIMD of one workgroup
  return per_block * ((tm * tn * 16 <= 64 || per_block == 1) ? 2 : 1);
}

// DB = false: one LDS image per operand, two barriers per reduction tile; meant for two
//   co-resident workgroups per CU that fill each other's bubbles.
// DB = true:  two images and ONE barrier per tile: while the waves multiply tile t out of image
//   t&1, tile t+1 (already in registers) is written to the other image and tile t+2 is requested
//   from memory, so a workgroup that is alone on its CU (256 x 256 tiles, 16 waves: one round
//   over the 60 000-row matrices) keeps its matrix cores fed without a partner.
template <int BM, int BN, int WM, int WN, bool AKC, bool BKC, bool DB = false, class Probe = NoProbe>
__global__ __launch_bounds__(64 * WM * WN, DB ? WM * WN / 4 : min_waves_per_simd(WM, WN, BM / WM / 32, BN / WN / 32))
void gemm_kernel(const GemmArgs p) {
  constexpr int THREADS = 64 * WM * WN;
  using TA = OperandTile<BM, AKC, THREADS>;
  using TB = OperandTile<BN, BKC, THREADS>;
  constexpr int WTM = BM / WM, WTN = BN / WN;    // wave tile
  constexpr int TM = WTM / 32, TN = WTN / 32;    // MFMA tiles per wave
  static_assert(TM >= 1 && TN >= 1, "wave tile must hold at least one 32x32 MFMA tile");
  constexpr int kImage = TA::kFloats + TB::kFloats;
  constexpr int kOperandFloats = (DB ? 2 : 1) * kImage;
  constexpr int kStageFloats = WM * WN * 32 * kKcLd;  // epilogue patches, one per wave
  __shared__ float lds[kOperandFloats > kStageFloats ? kOperandFloats : kStageFloats];
  const float* lds_a = lds;
  const float* lds_b = lds + TA::kFloats;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int problem = p.n_problems ? blockIdx.y / p.tiles_n : 0;
  const int tile_n = p.n_problems ? blockIdx.y % p.tiles_n : blockIdx.y;
  const int m0 = blockIdx.x * BM, n0 = tile_n * BN;
  const float* a_first = p.a[0];
  const float* b_first = p.b[0];
  if (p.n_problems) {
    a_first = kernarg_entry<const float*>(offsetof(GemmArgs, pa), problem);
    b_first = kernarg_entry<const float*>(offsetof(GemmArgs, pb), problem);
  }

  const int nt0 = (p.kseg[0] + kBK - 1) / kBK;
  const int nt1 = (p.kseg[1] + kBK - 1) / kBK;
  const int t_beg = blockIdx.z * p.tiles_per_split;
  const int t_end = min(nt0 + nt1, t_beg + p.tiles_per_split);

  v16f acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
  float csum[TM];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) csum[tm] = 0.f;
  // the wave that sums the A columns of row block wm: one per SIMD where the wave grid is square (wave w runs on SIMD w % 4,
  // so `wn == 0` would put the four of them — and their vector adds, which the f32 matrix pipe does not overlap — on SIMD 0)
  const bool want_colsum = !AKC && p.colsum != nullptr && tile_n == 0 && wn == (WM == WN ? wm : 0);

  v4f ra[TA::kVec], rb[TB::kVec];
  auto fetch_a = [&](v4f (&dst)[TA::kVec], int t) {
    const bool second = t >= nt0;
    TA::load(dst, second ? p.a[1] : a_first, second ? p.lda[1] : p.lda[0], m0,
             (second ? t - nt0 : t) * kBK, p.ra, second ? p.kseg[1] : p.kseg[0]);
  };
  auto fetch_b = [&](int t) {
    const bool second = t >= nt0;
    TB::load(rb, second ? p.b[1] : b_first, second ? p.ldb[1] : p.ldb[0], n0,
             (second ? t - nt0 : t) * kBK, p.rb, second ? p.kseg[1] : p.kseg[0]);
  };
  auto compute = [&]() {
#pragma unroll
    for (int g = 0; g < kBK / 8; ++g) {
      if (DB && (p.sched & 1)) {   // the builtin wants a literal
        if (g == 0) __builtin_amdgcn_s_setprio(3);
        else if (g == 1) __builtin_amdgcn_s_setprio(2);
        else if (g == 2) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      float af[TM][4], bf[TN][4];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) TA::fragment(af[tm], lds_a, wm * WTM + tm * 32, g);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) TB::fragment(bf[tn], lds_b, wn * WTN + tn * 32, g);
      if (want_colsum) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) csum[tm] += (af[tm][0] + af[tm][1]) + (af[tm][2] + af[tm][3]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tm][j], bf[tn][j], acc[tm][tn], 0, 0, 0);
    }
  };
  Probe::mark(0);
  auto stash = [&](int image) {
    TA::store(ra, lds + image * kImage);
    TB::store(rb, lds + image * kImage + TA::kFloats);
  };
  if (t_beg < t_end) {
    fetch_a(ra, t_beg);
    fetch_b(t_beg);
    stash(0);
    if (DB && t_beg + 1 < t_end) {
      fetch_a(ra, t_beg + 1);
      fetch_b(t_beg + 1);
    }
    __syncthreads();
  }
  Probe::mark(1);
  if constexpr (DB) {
    for (int t = t_beg; t < t_end; ++t) {
      const int cur = (t - t_beg) & 1;
      if (t + 1 < t_end) stash(cur ^ 1);  // tile t+1: requested one iteration ago
      if (t + 2 < t_end) {                // lands under the MFMAs below
        fetch_a(ra, t + 2);
        fetch_b(t + 2);
      }
      lds_a = lds + cur * kImage;
      lds_b = lds_a + TA::kFloats;
      compute();
      __syncthreads();  // image cur^1 complete for the next tile; everyone is done reading image cur
    }
  } else {
    for (int t = t_beg; t < t_end; ++t) {
      const bool more = t + 1 < t_end;
      if (more) {  // in flight under the MFMAs below
        fetch_a(ra, t + 1);
        fetch_b(t + 1);
      }
      compute();
      __syncthreads();  // every wave is done reading this tile
      if (more) {
        stash(0);
        __syncthreads();
      }
    }
  }

  Probe::mark(2);
  const size_t slab = p.n_problems ? static_cast<size_t>(problem) * p.n_splits + blockIdx.z : 0;
  write_tile<BM, BN, WM, WN>(p, lds, p.c + slab * p.ra * p.ldc, acc, m0, n0);
  Probe::mark(3);
  if (want_colsum) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const float total = csum[tm] + __shfl_xor(csum[tm], 32, kWave);  // the two kk halves
      const int row = m0 + wm * WTM + tm * 32 + (lane & 31);
      if ((lane >> 5) == 0 && row < p.ra) p.colsum[slab * p.ra + row] = total;
    }
  }
}

template <int BM, int BN, int WM, int WN, bool AKC, bool BKC, bool DB = false, class Probe = NoProbe>
int launch_tiles(const GemmArgs& p, int grid_y_mult, int splits, hipStream_t st) {
  GemmArgs q = p;
  q.sched = g_gemm_sched;
  q.tiles_n = (p.rb + BN - 1) / BN;
  dim3 grid((p.ra + BM - 1) / BM, q.tiles_n * grid_y_mult, splits);
  gemm_kernel<BM, BN, WM, WN, AKC, BKC, DB, Probe><<<grid, 64 * WM * WN, 0, st>>>(q);
  return launch_status();
}

}  // namespace
}  // namespace gts
