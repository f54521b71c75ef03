// C1-C5: the refinement CNN's 5x5x5 replicate-padded Conv3d (reference model/networks.py:83-93) for
// training, forward and backward, on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).  Restated in
// DESIGN.md §4h.
//
// Activations are channels-last [cx, cy, cz, C] (= [V, C], z fastest); weights are torch's
// [Cout, Cin, 5, 5, 5].  Every launch is an implicit GEMM over one output brick of 4 x 4 x 16
// voxels whose 8 x 8 x 20 input halo sits in LDS:
//   - replicate padding is the clamp of the halo's global coordinate; no padded copy exists;
//   - the A fragment of a tap is one LDS read at a compile-time offset from a per-lane base
//     (dz, the k-step and the M tile are unrolled; dx / dy advance the base once per 5 taps);
//   - channels go through LDS in chunks of CC <= 16 (Cin padded to a multiple of 4 with zeros).
// Data gradient = the same kernel as a zero-padded transposed convolution (flipped, transposed
// weights) onto the grid padded by 2 per side, then a fold that adds each side's two outer planes
// onto the boundary plane (the exact adjoint of the clamp) and applies the ReLU mask.
// Weight gradients: split-K over voxel bricks into a workspace, then a fixed-order sum.  No float
// atomics: two runs give identical bits.
#include "gts_common.h"

namespace gts {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kTX = 4, kTY = 4, kTZ = 16;                      // output brick (4 waves x 4 M tiles of 16 z)
constexpr int kHX = kTX + 4, kHY = kTY + 4, kHZ = kTZ + 4;
constexpr int kHalo = kHX * kHY * kHZ;                         // 1280 voxels
constexpr int kTaps = 125;
constexpr int kMaxChannels = 32;
constexpr int kWgradTilesPerWave = 8;                          // N tiles of 16 columns per wave in C5
constexpr int kWgradTargetBlocks = 512;
constexpr int kBiasBlocks = 64;

__host__ __device__ inline int round4(int c) { return (c + 3) & ~3; }
inline int chunk_width(int c) { return round4(c) > 16 ? 16 : round4(c); }
inline int n_chunks(int c) { return (round4(c) + chunk_width(c) - 1) / chunk_width(c); }
inline int n_tiles16(int c) { return (c + 15) / 16; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// packed fragments of one layer: [chunk][tap][k-step][n tile][lane]
inline int64_t packed_floats(int cin, int cout) {
  return static_cast<int64_t>(n_chunks(cin)) * kTaps * (chunk_width(cin) / 4) * n_tiles16(cout) * kWave;
}

struct PackArgs {
  const float* w;   // [co_t][ci_t][125] of the torch layout
  float* out;
  int cin, cout;    // of the GEMM this feeds (transposed: cin = torch Cout, cout = torch Cin)
  int cc, nt;
  int transposed;   // 1: B[ci][co][tap] = w[ci][co][124 - tap] (flipped taps, swapped channels)
  int64_t total;
};

// lane l of k-step s, n tile j: B[k = l >> 4][n = l & 15] = W[co = 16 j + (l & 15)][ci = chunk CC + 4 s + (l >> 4)]
__global__ __launch_bounds__(kBlock) void pack_kernel(PackArgs a) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= a.total) return;
  const int lane = static_cast<int>(e % kWave);
  int64_t r = e / kWave;
  const int j = static_cast<int>(r % a.nt);
  r /= a.nt;
  const int s = static_cast<int>(r % (a.cc / 4));
  r /= a.cc / 4;
  const int tap = static_cast<int>(r % kTaps);
  const int ch = static_cast<int>(r / kTaps);
  const int co = 16 * j + (lane & 15), ci = ch * a.cc + 4 * s + (lane >> 4);
  float v = 0.0f;
  if (co < a.cout && ci < a.cin)
    v = a.transposed ? a.w[(static_cast<int64_t>(ci) * a.cout + co) * kTaps + (kTaps - 1 - tap)]
                     : a.w[(static_cast<int64_t>(co) * a.cin + ci) * kTaps + tap];
  a.out[e] = v;
}

struct ConvArgs {
  const float* in;    // [ix, iy, iz, cin]
  const float* wpk;   // packed_floats(cin, cout)
  const float* bias;  // [cout] or NULL
  float* out;         // [ox, oy, oz, cout]
  int ix, iy, iz, cin;
  int ox, oy, oz, cout;
  int off;            // input coordinate = output coordinate + off + tap
  int clamp;          // 1: replicate (clamp), 0: zero outside the input
  int relu;
  int tiles_y, tiles_z;
};

// Load the CC-channel slice `ch` of the halo of the brick at (x0, y0, z0) + off into LDS
// (row stride VS = CC + 1 floats: odd, so the 16 voxels of one A fragment fall in distinct banks).
template <int CC>
__device__ __forceinline__ void load_halo(float* halo, const float* in, int ix, int iy, int iz, int cin, int ch,
                                          int x0, int y0, int z0, int clamp) {
  constexpr int VS = CC + 1;
  for (int e = threadIdx.x; e < kHalo * CC; e += kBlock) {
    const int c = e % CC, hv = e / CC;
    const int hz = hv % kHZ, hy = (hv / kHZ) % kHY, hx = hv / (kHZ * kHY);
    int gx = x0 + hx, gy = y0 + hy, gz = z0 + hz;
    const int ci = ch * CC + c;
    bool ok = ci < cin;
    if (clamp) {
      gx = min(max(gx, 0), ix - 1), gy = min(max(gy, 0), iy - 1), gz = min(max(gz, 0), iz - 1);
    } else {
      ok = ok && gx >= 0 && gx < ix && gy >= 0 && gy < iy && gz >= 0 && gz < iz;
    }
    halo[hv * VS + c] = ok ? in[((static_cast<int64_t>(gx) * iy + gy) * iz + gz) * cin + ci] : 0.0f;
  }
}

// C1 / C2 / C3a: out = act(conv(in) + bias).  Wave w owns x = x0 + w and the 4 M tiles y0 .. y0 + 3
// (16 z each); lane l: A[z = l & 15][k = l >> 4], D[z = 4 (l >> 4) + r][co = l & 15].
template <int CC, int NT>
__global__ __launch_bounds__(kBlock) void conv_kernel(ConvArgs a) {
  constexpr int VS = CC + 1, KS = CC / 4;
  extern __shared__ float halo[];
  const int tile = blockIdx.x;
  const int tz = tile % a.tiles_z, ty = (tile / a.tiles_z) % a.tiles_y, tx = tile / (a.tiles_z * a.tiles_y);
  const int x0 = tx * kTX, y0 = ty * kTY, z0 = tz * kTZ;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  v4f acc[4][NT];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[m][j] = v4f{0.f, 0.f, 0.f, 0.f};
  const int chunks = (round4(a.cin) + CC - 1) / CC;
  for (int ch = 0; ch < chunks; ++ch) {
    if (ch) __syncthreads();
    load_halo<CC>(halo, a.in, a.ix, a.iy, a.iz, a.cin, ch, x0 + a.off, y0 + a.off, z0 + a.off, a.clamp);
    __syncthreads();
    const float* wch = a.wpk + static_cast<int64_t>(ch) * kTaps * KS * NT * kWave + lane;
    const float* abase = halo + ((wave * kHY) * kHZ + (lane & 15)) * VS + (lane >> 4);
    for (int dx = 0; dx < 5; ++dx) {
      for (int dy = 0; dy < 5; ++dy) {
        const float* wr = wch + (dx * 5 + dy) * 5 * KS * NT * kWave;
        float b[5][KS][NT];
#pragma unroll
        for (int dz = 0; dz < 5; ++dz)
#pragma unroll
          for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < NT; ++j) b[dz][s][j] = wr[((dz * KS + s) * NT + j) * kWave];
        const float* ar = abase + (dx * kHY * kHZ + dy * kHZ) * VS;
#pragma unroll
        for (int dz = 0; dz < 5; ++dz)
#pragma unroll
          for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              const float av = ar[(m * kHZ + dz) * VS + 4 * s];
#pragma unroll
              for (int j = 0; j < NT; ++j)
                acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[dz][s][j], acc[m][j], 0, 0, 0);
            }
      }
    }
  }
  const int x = x0 + wave;
  if (x >= a.ox) return;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int y = y0 + m;
    if (y >= a.oy) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int co = 16 * j + (lane & 15);
      if (co >= a.cout) continue;
      const float bias = a.bias ? a.bias[co] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int z = z0 + 4 * (lane >> 4) + r;
        if (z >= a.oz) continue;
        float v = acc[m][j][r] + bias;
        if (a.relu) v = relu_f32(v);
        a.out[((static_cast<int64_t>(x) * a.oy + y) * a.oz + z) * a.cout + co] = v;
      }
    }
  }
}

// C3b: dh[u, c] = [h[u, c] > 0] * sum of g over the padded positions that clamp onto u.  g is the
// transposed convolution on the grid padded by 2 per side; per axis those positions are u + 2, plus
// 0, 1 when u is the first plane and n + 2, n + 3 when u is the last (all five when n == 1).
__global__ __launch_bounds__(kBlock) void fold_kernel(const float* __restrict__ g, const float* __restrict__ h,
                                                      float* __restrict__ dh, int cx, int cy, int cz, int c) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t total = static_cast<int64_t>(cx) * cy * cz * c;
  if (e >= total) return;
  const int ch = static_cast<int>(e % c);
  const int64_t u = e / c;
  const int uz = static_cast<int>(u % cz), uy = static_cast<int>((u / cz) % cy), ux = static_cast<int>(u / (cz * static_cast<int64_t>(cy)));
  if (h && !(h[e] > 0.0f)) {
    dh[e] = 0.0f;
    return;
  }
  int px[5], py[5], pz[5];
  int nx = 0, ny = 0, nz = 0;
  px[nx++] = ux + 2, py[ny++] = uy + 2, pz[nz++] = uz + 2;
  if (ux == 0) px[nx++] = 0, px[nx++] = 1;
  if (ux == cx - 1) px[nx++] = cx + 2, px[nx++] = cx + 3;
  if (uy == 0) py[ny++] = 0, py[ny++] = 1;
  if (uy == cy - 1) py[ny++] = cy + 2, py[ny++] = cy + 3;
  if (uz == 0) pz[nz++] = 0, pz[nz++] = 1;
  if (uz == cz - 1) pz[nz++] = cz + 2, pz[nz++] = cz + 3;
  const int64_t gy = cy + 4, gz = cz + 4;
  float sum = 0.0f;
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < ny; ++j)
      for (int k = 0; k < nz; ++k) sum += g[((px[i] * gy + py[j]) * gz + pz[k]) * c + ch];
  dh[e] = sum;
}

struct WgradArgs {
  const float* x;    // [cx, cy, cz, cin] layer input
  const float* dy;   // [cx, cy, cz, cout] gradient of the layer output
  float* part;       // [nsplit][cout][chunks][ntn * 16]
  int cx, cy, cz, cin, cout;
  int tiles_y, tiles_z, n_bricks;
  int groups;        // N tile groups per chunk (kWavesPerBlock * kWgradTilesPerWave tiles each)
  int chunks, ntn;   // ntn: N tiles of one chunk = ceil(125 CC / 16)
  int per_split;     // bricks per split
};

// C4 / C5 partial: part[split][co][ch][col] = sum over the split's bricks of dy[v, co] x[clamp(v + tap - 2), ci],
// col = tap CC + ci % CC.  M = co (MT tiles), N = columns, K = the brick's 256 voxels, 4 per k-step
// (lane l: A[co = l & 15][v = l >> 4], B[v = l >> 4][col = l & 15]).
template <int CC, int MT>
__global__ __launch_bounds__(kBlock) void wgrad_kernel(WgradArgs a) {
  constexpr int VS = CC + 1, DS = MT * 16 + 1;
  extern __shared__ float smem[];
  float* halo = smem;
  float* dys = smem + kHalo * VS;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int unit = blockIdx.x % (a.chunks * a.groups), split = blockIdx.x / (a.chunks * a.groups);
  const int ch = unit / a.groups, grp = unit % a.groups;
  const int nt0 = (grp * kWavesPerBlock + wave) * kWgradTilesPerWave;
  int bbase[kWgradTilesPerWave];
#pragma unroll
  for (int n = 0; n < kWgradTilesPerWave; ++n) {
    const int col = (nt0 + n) * 16 + (lane & 15);
    const int tap = col < kTaps * CC ? col / CC : 0, ci = col % CC;
    bbase[n] = (((tap / 25) * kHY + (tap / 5) % 5) * kHZ + tap % 5) * VS + ci + (lane >> 4) * VS;
  }
  v4f acc[MT][kWgradTilesPerWave];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < kWgradTilesPerWave; ++n) acc[m][n] = v4f{0.f, 0.f, 0.f, 0.f};
  const int b_end = min(a.n_bricks, (split + 1) * a.per_split);
  for (int brick = split * a.per_split; brick < b_end; ++brick) {
    const int tz = brick % a.tiles_z, ty = (brick / a.tiles_z) % a.tiles_y, tx = brick / (a.tiles_z * a.tiles_y);
    const int x0 = tx * kTX, y0 = ty * kTY, z0 = tz * kTZ;
    __syncthreads();
    load_halo<CC>(halo, a.x, a.cx, a.cy, a.cz, a.cin, ch, x0 - 2, y0 - 2, z0 - 2, 1);
    for (int e = threadIdx.x; e < kTX * kTY * kTZ * MT * 16; e += kBlock) {
      const int co = e % (MT * 16), v = e / (MT * 16);
      const int x = x0 + v / (kTY * kTZ), y = y0 + (v / kTZ) % kTY, z = z0 + v % kTZ;
      const bool ok = co < a.cout && x < a.cx && y < a.cy && z < a.cz;   // voxels past the volume contribute 0
      dys[v * DS + co] = ok ? a.dy[((static_cast<int64_t>(x) * a.cy + y) * a.cz + z) * a.cout + co] : 0.0f;
    }
    __syncthreads();
    if (nt0 >= a.ntn) continue;
#pragma unroll
    for (int kk = 0; kk < kTX * kTY * kTZ / 4; ++kk) {
      const int vx = kk / 16, vy = (kk / 4) % 4, vz = 4 * (kk % 4);   // k-step: voxels vz .. vz + 3 of row (vx, vy)
      const int hoff = ((vx * kHY + vy) * kHZ + vz) * VS;
      const int v = (vx * kTY + vy) * kTZ + vz + (lane >> 4);
      // a k-step voxel past the volume: dy is 0 there, and so must x be (0 * Inf from the clamped halo would be NaN)
      const bool inside = x0 + vx < a.cx && y0 + vy < a.cy && z0 + vz + (lane >> 4) < a.cz;
      float av[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) av[m] = dys[v * DS + m * 16 + (lane & 15)];
#pragma unroll
      for (int n = 0; n < kWgradTilesPerWave; ++n) {
        const float bv = inside ? halo[bbase[n] + hoff] : 0.0f;
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv, acc[m][n], 0, 0, 0);
      }
    }
  }
  if (nt0 >= a.ntn) return;
  const int row_cols = a.ntn * 16;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = m * 16 + 4 * (lane >> 4) + r;
      if (co >= a.cout) continue;
      float* dst = a.part + ((static_cast<int64_t>(split) * a.cout + co) * a.chunks + ch) * row_cols;
#pragma unroll
      for (int n = 0; n < kWgradTilesPerWave; ++n) {
        const int nt = nt0 + n;
        if (nt < a.ntn) dst[nt * 16 + (lane & 15)] = acc[m][n][r];
      }
    }
}

// C4 / C5 finish: dw[co][ci][tap] = sum over splits in split order of the partials.
__global__ __launch_bounds__(kBlock) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                              int cin, int cout, int cc, int chunks, int row_cols,
                                                              int nsplit) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= cout * cin * kTaps) return;
  const int tap = e % kTaps, ci = (e / kTaps) % cin, co = e / (kTaps * cin);
  const int ch = ci / cc;
  const int64_t stride = static_cast<int64_t>(cout) * chunks * row_cols;
  const float* p = part + (static_cast<int64_t>(co) * chunks + ch) * row_cols + tap * cc + ci % cc;
  float sum = 0.0f;
  for (int s = 0; s < nsplit; ++s) sum += p[s * stride];
  dw[e] = sum;
}

// bias gradient: block b sums voxels b, b + kBiasBlocks, ... per lane-strided run, then a fixed tree
__global__ __launch_bounds__(kBlock) void bias_partial_kernel(const float* __restrict__ dy, float* __restrict__ part,
                                                              int64_t n_vox, int cout) {
  __shared__ float red[kBlock];
  for (int co = 0; co < cout; ++co) {
    float s = 0.0f;
    for (int64_t v = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; v < n_vox;
         v += static_cast<int64_t>(kBiasBlocks) * kBlock)
      s += dy[v * cout + co];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlock / 2; w >= 1; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x * kMaxChannels + co] = red[0];
    __syncthreads();
  }
}

__global__ void bias_finish_kernel(const float* __restrict__ part, float* __restrict__ db, int cout) {
  const int co = threadIdx.x;
  if (co >= cout) return;
  float s = 0.0f;
  for (int b = 0; b < kBiasBlocks; ++b) s += part[b * kMaxChannels + co];
  db[co] = s;
}

// ---- host side -------------------------------------------------------------------------------

struct Geometry {
  int64_t tiles_x, tiles_y, tiles_z;
  int64_t bricks() const { return tiles_x * tiles_y * tiles_z; }
};

inline Geometry geometry(int64_t x, int64_t y, int64_t z) {
  return Geometry{cdiv(x, kTX), cdiv(y, kTY), cdiv(z, kTZ)};
}

// dims >= 1, every padded volume x channels indexable in int32, channels 1..32
inline bool valid_shape(int64_t cx, int64_t cy, int64_t cz, int64_t c0, int64_t c1) {
  if (cx < 1 || cy < 1 || cz < 1 || cx > (1 << 20) || cy > (1 << 20) || cz > (1 << 20)) return false;
  if (c0 < 1 || c0 > kMaxChannels || c1 < 1 || c1 > kMaxChannels) return false;
  const int64_t padded = (cx + 4) * (cy + 4) * (cz + 4);
  return padded * kMaxChannels < (1LL << 31);
}

inline size_t halo_bytes(int cc) { return static_cast<size_t>(kHalo) * (cc + 1) * sizeof(float); }

int launch_pack(const float* w, float* out, int cin, int cout, int transposed, hipStream_t st) {
  PackArgs a{w, out, cin, cout, chunk_width(cin), n_tiles16(cout), transposed, packed_floats(cin, cout)};
  pack_kernel<<<static_cast<unsigned>(cdiv(a.total, kBlock)), kBlock, 0, st>>>(a);
  return launch_status();
}

template <int CC, int NT>
int launch_conv_t(const ConvArgs& a, unsigned blocks, hipStream_t st) {
  const size_t lds = halo_bytes(CC);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_kernel<CC, NT>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
  if (e != hipSuccess) return static_cast<int>(e);
  conv_kernel<CC, NT><<<blocks, kBlock, lds, st>>>(a);
  return launch_status();
}

template <int CC>
int launch_conv_cc(const ConvArgs& a, unsigned blocks, hipStream_t st) {
  return n_tiles16(a.cout) == 1 ? launch_conv_t<CC, 1>(a, blocks, st) : launch_conv_t<CC, 2>(a, blocks, st);
}

int launch_conv(ConvArgs a, hipStream_t st) {
  const Geometry g = geometry(a.ox, a.oy, a.oz);
  a.tiles_y = static_cast<int>(g.tiles_y), a.tiles_z = static_cast<int>(g.tiles_z);
  const unsigned blocks = static_cast<unsigned>(g.bricks());
  switch (chunk_width(a.cin)) {
    case 4: return launch_conv_cc<4>(a, blocks, st);
    case 8: return launch_conv_cc<8>(a, blocks, st);
    case 12: return launch_conv_cc<12>(a, blocks, st);
    default: return launch_conv_cc<16>(a, blocks, st);
  }
}

struct WgradPlan {
  int cc, chunks, ntn, groups, nsplit, per_split;
  int64_t n_bricks;
  int64_t part_floats() const;
};

WgradPlan wgrad_plan(int64_t cx, int64_t cy, int64_t cz, int cin, int cout) {
  WgradPlan p;
  p.cc = chunk_width(cin), p.chunks = n_chunks(cin);
  p.ntn = static_cast<int>(cdiv(kTaps * p.cc, 16));
  p.groups = static_cast<int>(cdiv(p.ntn, kWavesPerBlock * kWgradTilesPerWave));
  p.n_bricks = geometry(cx, cy, cz).bricks();
  const int64_t want = cdiv(kWgradTargetBlocks, p.chunks * p.groups);
  p.per_split = static_cast<int>(cdiv(p.n_bricks, want < p.n_bricks ? want : p.n_bricks));
  p.nsplit = static_cast<int>(cdiv(p.n_bricks, p.per_split));
  return p;
}

int64_t WgradPlan::part_floats() const { return static_cast<int64_t>(nsplit) * chunks * ntn * 16; }

template <int CC, int MT>
int launch_wgrad_t(const WgradArgs& a, unsigned blocks, hipStream_t st) {
  const size_t lds = halo_bytes(CC) + static_cast<size_t>(kTX * kTY * kTZ) * (MT * 16 + 1) * sizeof(float);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_kernel<CC, MT>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
  if (e != hipSuccess) return static_cast<int>(e);
  wgrad_kernel<CC, MT><<<blocks, kBlock, lds, st>>>(a);
  return launch_status();
}

template <int CC>
int launch_wgrad_cc(const WgradArgs& a, unsigned blocks, hipStream_t st) {
  return n_tiles16(a.cout) == 1 ? launch_wgrad_t<CC, 1>(a, blocks, st) : launch_wgrad_t<CC, 2>(a, blocks, st);
}

}  // namespace
}  // namespace gts

using namespace gts;

extern "C" int64_t gts_conv3d_fwd_workspace(int32_t cin, int32_t cout) {
  if (cin < 1 || cin > kMaxChannels || cout < 1 || cout > kMaxChannels) return 0;
  return packed_floats(cin, cout) * static_cast<int64_t>(sizeof(float));
}

extern "C" int32_t gts_conv3d_fwd_f32(const float* x, const float* w, const float* bias, float* y, int64_t cx,
                                      int64_t cy, int64_t cz, int32_t cin, int32_t cout, int32_t relu,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !w || !y || !workspace) return GTS_ERR_NULL;
  if (!valid_shape(cx, cy, cz, cin, cout)) return GTS_ERR_SHAPE;
  if (relu != 0 && relu != 1) return GTS_ERR_ARGKIND;
  if (workspace_bytes < gts_conv3d_fwd_workspace(cin, cout)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* wpk = static_cast<float*>(workspace);
  int rc = launch_pack(w, wpk, cin, cout, 0, st);
  if (rc) return rc;
  const int X = static_cast<int>(cx), Y = static_cast<int>(cy), Z = static_cast<int>(cz);
  ConvArgs a{x, wpk, bias, y, X, Y, Z, cin, X, Y, Z, cout, -2, 1, relu, 0, 0};
  return launch_conv(a, st);
}

extern "C" int64_t gts_conv3d_bwd_data_workspace(int64_t cx, int64_t cy, int64_t cz, int32_t cin, int32_t cout) {
  if (!valid_shape(cx, cy, cz, cin, cout)) return 0;
  const int64_t pk = cdiv(packed_floats(cout, cin), 64) * 64;   // keeps g 256-byte aligned
  return (pk + (cx + 4) * (cy + 4) * (cz + 4) * cin) * static_cast<int64_t>(sizeof(float));
}

extern "C" int32_t gts_conv3d_bwd_data_f32(const float* dy, const float* w, const float* h, float* dx, int64_t cx,
                                           int64_t cy, int64_t cz, int32_t cin, int32_t cout, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  if (!dy || !w || !dx || !workspace) return GTS_ERR_NULL;
  if (!valid_shape(cx, cy, cz, cin, cout)) return GTS_ERR_SHAPE;
  if (workspace_bytes < gts_conv3d_bwd_data_workspace(cx, cy, cz, cin, cout)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* wpk = static_cast<float*>(workspace);
  float* g = wpk + cdiv(packed_floats(cout, cin), 64) * 64;
  int rc = launch_pack(w, wpk, cout, cin, 1, st);
  if (rc) return rc;
  const int X = static_cast<int>(cx), Y = static_cast<int>(cy), Z = static_cast<int>(cz);
  ConvArgs a{dy, wpk, nullptr, g, X, Y, Z, cout, X + 4, Y + 4, Z + 4, cin, -4, 0, 0, 0, 0};
  rc = launch_conv(a, st);
  if (rc) return rc;
  const int64_t total = cx * cy * cz * cin;
  fold_kernel<<<static_cast<unsigned>(cdiv(total, kBlock)), kBlock, 0, st>>>(g, h, dx, X, Y, Z, cin);
  return launch_status();
}

extern "C" int64_t gts_conv3d_bwd_weight_workspace(int64_t cx, int64_t cy, int64_t cz, int32_t cin, int32_t cout) {
  if (!valid_shape(cx, cy, cz, cin, cout)) return 0;
  const WgradPlan p = wgrad_plan(cx, cy, cz, cin, cout);
  return (p.part_floats() * cout + static_cast<int64_t>(kBiasBlocks) * kMaxChannels) *
         static_cast<int64_t>(sizeof(float));
}

extern "C" int32_t gts_conv3d_bwd_weight_f32(const float* x, const float* dy, float* dw, float* db, int64_t cx,
                                             int64_t cy, int64_t cz, int32_t cin, int32_t cout, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
  if (!x || !dy || !dw || !workspace) return GTS_ERR_NULL;
  if (!valid_shape(cx, cy, cz, cin, cout)) return GTS_ERR_SHAPE;
  if (workspace_bytes < gts_conv3d_bwd_weight_workspace(cx, cy, cz, cin, cout)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const WgradPlan p = wgrad_plan(cx, cy, cz, cin, cout);
  float* part = static_cast<float*>(workspace);
  const Geometry g = geometry(cx, cy, cz);
  WgradArgs a{x, dy, part, static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(cz), cin, cout,
              static_cast<int>(g.tiles_y), static_cast<int>(g.tiles_z), static_cast<int>(p.n_bricks), p.groups,
              p.chunks, p.ntn, p.per_split};
  const unsigned blocks = static_cast<unsigned>(p.nsplit * p.chunks * p.groups);
  int rc;
  switch (p.cc) {
    case 4: rc = launch_wgrad_cc<4>(a, blocks, st); break;
    case 8: rc = launch_wgrad_cc<8>(a, blocks, st); break;
    case 12: rc = launch_wgrad_cc<12>(a, blocks, st); break;
    default: rc = launch_wgrad_cc<16>(a, blocks, st); break;
  }
  if (rc) return rc;
  const int n_out = cout * cin * kTaps;
  wgrad_reduce_kernel<<<static_cast<unsigned>(cdiv(n_out, kBlock)), kBlock, 0, st>>>(
      part, dw, cin, cout, p.cc, p.chunks, p.ntn * 16, p.nsplit);
  rc = launch_status();
  if (rc || !db) return rc;
  float* bpart = part + p.part_floats() * cout;
  bias_partial_kernel<<<kBiasBlocks, kBlock, 0, st>>>(dy, bpart, cx * cy * cz, cout);
  bias_finish_kernel<<<1, kMaxChannels, 0, st>>>(bpart, db, cout);
  return launch_status();
}
