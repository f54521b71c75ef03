// I1-I3: intake of a raw four-modality scan on the device — the crop, normalize and standardize step
// of DataPreprocessor.load (scripts/preprocess_dataset.py):
//
//   crop  = determine_brain_crop(image)                               # planes where max_c > 0.01
//   image = standardize_img(normalize_img(image[crop]), mean, std)    # x / q995_c, (x - mean_c) / std_c
//
// Source: the four volumes as NIfTI stores them, [4][Z][Y][X] (x fastest), int16 or float32; every
// value is taken as float32 (exact for int16), as read_nifti(..., np.float32) gives it.
//
//   I1  plane occupancy: np.amax over channels (a NaN anywhere makes the max NaN and the test false)
//       compared with 0.01, reduced to one flag per x, y and z plane through LDS byte flags; the same
//       pass counts voxels that hold a non-finite value;
//   I2  two exact order statistics per channel over the cropped region (an np.ix_ of the flag masks,
//       not a box): a 4-pass radix select on the order-preserving uint32 key, 8 bits per pass, with
//       LDS-privatised histograms merged into the workspace per pass and a one-block step that walks
//       the 256 bins; the two ranks are followed separately (they may fall into different buckets)
//       and share one histogram while their prefixes agree;
//   I3  fused gather + ((x / top_c) - mean_c) / std_c in IEEE float32 (-ffp-contract=off, correctly
//       rounded division) into C-order [cx, cy, cz, 4]: a 64 (x) x 16 (z) tile per workgroup is read
//       along x into LDS and written along z with one 16-byte store per voxel.
#include "gts_common.h"

namespace gts {
namespace {

constexpr int kChannels = 4;
constexpr int kMaxExtent = 4096;   // LDS flag arrays of I1
constexpr int kMaxBlocks = 2048;
constexpr int kBins = 256;
constexpr int kHist = kChannels * 2 * kBins;   // [channel][rank][bin]
constexpr int kTileX = 64, kTileZ = 16;
constexpr int32_t kI16 = 4, kF32 = 16;       // NIfTI datatype codes

struct SelectState {
  unsigned prefix[kChannels][2];
  unsigned long long rank[kChannels][2];   // rank still to skip inside the current prefix
};

struct Layout {
  int64_t hist, state, total;
};
constexpr Layout kLayout = {0, kHist * 4, kHist * 4 + 256};

// Order-preserving key of a float32; -0.0 is mapped to +0.0 first, so that the two zeros form one
// value (np.partition does not order them; a rank that lands on zeros returns +0.0).
__device__ __forceinline__ unsigned float_key(float v) {
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

template <typename T>
__device__ __forceinline__ float load_f32(const T* __restrict__ p, size_t i) {
  return static_cast<float>(p[i]);
}

// I1.
template <typename T>
__global__ __launch_bounds__(kBlock) void intake_occupancy_kernel(const T* __restrict__ src, int X, int Y, int Z,
                                                                  int32_t* __restrict__ fx, int32_t* __restrict__ fy,
                                                                  int32_t* __restrict__ fz,
                                                                  unsigned long long* __restrict__ nonfinite) {
  __shared__ uint8_t sx[kMaxExtent], sy[kMaxExtent], sz[kMaxExtent];
  __shared__ unsigned bad;
  for (int i = threadIdx.x; i < kMaxExtent; i += kBlock) sx[i] = sy[i] = sz[i] = 0;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const unsigned xy = static_cast<unsigned>(X) * Y, vol = xy * Z;
  unsigned mine = 0;
  for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < vol; i += gridDim.x * kBlock) {
    float v[kChannels];
#pragma unroll
    for (int c = 0; c < kChannels; ++c) v[c] = load_f32(src, static_cast<size_t>(c) * vol + i);
    bool nan = false, finite = true;
    float m = v[0];
#pragma unroll
    for (int c = 0; c < kChannels; ++c) {
      nan |= v[c] != v[c];
      finite &= __builtin_isfinite(v[c]);
      m = v[c] > m ? v[c] : m;
    }
    mine += finite ? 0u : 1u;
    if (!nan && m > 0.01f) {
      const unsigned x = i % X, r = i / X;
      sx[x] = 1;
      sy[r % Y] = 1;
      sz[r / Y] = 1;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && mine) atomicAdd(&bad, mine);
  __syncthreads();
  for (int i = threadIdx.x; i < X; i += kBlock)
    if (sx[i]) fx[i] = 1;
  for (int i = threadIdx.x; i < Y; i += kBlock)
    if (sy[i]) fy[i] = 1;
  for (int i = threadIdx.x; i < Z; i += kBlock)
    if (sz[i]) fz[i] = 1;
  if (threadIdx.x == 0 && bad) atomicAdd(nonfinite, static_cast<unsigned long long>(bad));
}

// Voxel offset of cropped element (xi, yi, zi); an index outside the volume reads voxel 0 instead of
// leaving the buffer (the host builds the lists from I1's flags, so this never happens there).
__device__ __forceinline__ unsigned crop_offset(const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                                                const int32_t* __restrict__ zs, unsigned xi, unsigned yi, unsigned zi,
                                                int X, int Y, int Z) {
  const unsigned x = static_cast<unsigned>(xs[xi]), y = static_cast<unsigned>(ys[yi]),
                 z = static_cast<unsigned>(zs[zi]);
  if (x >= unsigned(X) || y >= unsigned(Y) || z >= unsigned(Z)) return 0;
  return (z * Y + y) * X + x;
}

__global__ void intake_select_init_kernel(unsigned* __restrict__ hist, SelectState* __restrict__ st,
                                          unsigned long long rank_lo, unsigned long long rank_hi) {
  for (int i = threadIdx.x; i < kHist; i += blockDim.x) hist[i] = 0;
  if (threadIdx.x < 2 * kChannels) {
    const int c = threadIdx.x >> 1, r = threadIdx.x & 1;
    st->prefix[c][r] = 0;
    st->rank[c][r] = r ? rank_hi : rank_lo;
  }
}

// I2, one pass: histogram of digit (key >> shift) & 255 over the elements whose higher digits equal
// the rank's prefix.
template <typename T>
__global__ __launch_bounds__(kBlock) void intake_hist_kernel(const T* __restrict__ src, int X, int Y, int Z,
                                                             const int32_t* __restrict__ xs, int cx,
                                                             const int32_t* __restrict__ ys, int cy,
                                                             const int32_t* __restrict__ zs,
                                                             unsigned n, const SelectState* __restrict__ st,
                                                             unsigned* __restrict__ hist, int shift) {
  __shared__ unsigned h[kHist];
  for (int i = threadIdx.x; i < kHist; i += kBlock) h[i] = 0;
  const unsigned hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
  unsigned p0[kChannels], p1[kChannels];
  bool both[kChannels];
#pragma unroll
  for (int c = 0; c < kChannels; ++c) {
    p0[c] = st->prefix[c][0];
    p1[c] = st->prefix[c][1];
    both[c] = p0[c] != p1[c];
  }
  __syncthreads();
  const size_t vol = static_cast<size_t>(X) * Y * Z;
  for (unsigned e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
    const unsigned xi = e % cx, r = e / cx;
    const unsigned off = crop_offset(xs, ys, zs, xi, r % cy, r / cy, X, Y, Z);
#pragma unroll
    for (int c = 0; c < kChannels; ++c) {
      const unsigned key = float_key(load_f32(src, c * vol + off));
      const unsigned d = (key >> shift) & (kBins - 1);
      if (((key ^ p0[c]) & hi_mask) == 0) atomicAdd(&h[(2 * c) * kBins + d], 1u);
      if (both[c] && ((key ^ p1[c]) & hi_mask) == 0) atomicAdd(&h[(2 * c + 1) * kBins + d], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHist; i += kBlock)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

// I2, one step: each (channel, rank) walks its histogram to the bin that holds its rank, appends the
// digit to its prefix, and the histogram is cleared for the next pass.  After the last pass the
// prefix is the key of the order statistic.
__global__ __launch_bounds__(kBlock) void intake_select_step_kernel(unsigned* __restrict__ hist,
                                                                    SelectState* __restrict__ st, int shift,
                                                                    float* __restrict__ out) {
  const int t = threadIdx.x;
  unsigned prefix = 0, digit = kBins - 1;
  unsigned long long k = 0;
  if (t < 2 * kChannels) {
    const int c = t >> 1, r = t & 1;
    const bool shared_hist = st->prefix[c][0] == st->prefix[c][1];
    const unsigned* h = hist + (2 * c + (shared_hist ? 0 : r)) * kBins;
    prefix = st->prefix[c][r];
    k = st->rank[c][r];
    unsigned long long acc = 0;
    for (int b = 0; b < kBins; ++b) {
      if (k < acc + h[b]) {
        digit = b;
        break;
      }
      acc += h[b];
    }
    k -= acc;
    prefix |= digit << shift;
  }
  __syncthreads();  // every walk has read the prefixes and the histograms
  if (t < 2 * kChannels) {
    st->prefix[t >> 1][t & 1] = prefix;
    st->rank[t >> 1][t & 1] = k;
    if (out) out[t] = key_float(prefix);
  }
  for (int i = t; i < kHist; i += kBlock) hist[i] = 0;
}

struct StandardizeParams {
  float top[kChannels], mean[kChannels], std[kChannels];
};

// I3.  Workgroup (x tile, yi, z tile); LDS tile [c][z][x] padded to 65 floats per row: the read phase
// walks x (consecutive words), the write phase walks z (stride 65, conflict-free).
template <typename T>
__global__ __launch_bounds__(kBlock) void intake_standardize_kernel(const T* __restrict__ src, int X, int Y, int Z,
                                                                    const int32_t* __restrict__ xs, int cx,
                                                                    const int32_t* __restrict__ ys, int cy,
                                                                    const int32_t* __restrict__ zs, int cz,
                                                                    StandardizeParams p, float* __restrict__ out) {
  __shared__ float tile[kChannels][kTileZ][kTileX + 1];
  const int x0 = blockIdx.x * kTileX, yi = blockIdx.y, z0 = blockIdx.z * kTileZ;
  const size_t vol = static_cast<size_t>(X) * Y * Z;
  {
    const int lx = threadIdx.x % kTileX, lz0 = threadIdx.x / kTileX;
    const int xi = x0 + lx;
    if (xi < cx) {
#pragma unroll
      for (int lz = lz0; lz < kTileZ; lz += kBlock / kTileX) {
        const int zi = z0 + lz;
        if (zi >= cz) break;
        const unsigned off = crop_offset(xs, ys, zs, xi, yi, zi, X, Y, Z);
#pragma unroll
        for (int c = 0; c < kChannels; ++c) tile[c][lz][lx] = load_f32(src, c * vol + off);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int v = threadIdx.x; v < kTileX * kTileZ; v += kBlock) {
    const int lx = v / kTileZ, lz = v % kTileZ;
    const int xi = x0 + lx, zi = z0 + lz;
    if (xi >= cx || zi >= cz) continue;
    float r[kChannels];
#pragma unroll
    for (int c = 0; c < kChannels; ++c) r[c] = (tile[c][lz][lx] / p.top[c] - p.mean[c]) / p.std[c];
    const size_t o = ((static_cast<size_t>(xi) * cy + yi) * cz + zi) * kChannels;
    *reinterpret_cast<float4*>(out + o) = make_float4(r[0], r[1], r[2], r[3]);
  }
}

inline bool volume_ok(int64_t X, int64_t Y, int64_t Z) {
  return X >= 1 && Y >= 1 && Z >= 1 && X <= kMaxExtent && Y <= kMaxExtent && Z <= kMaxExtent &&
         X * Y * Z < (int64_t{1} << 31);
}

inline bool crop_ok(int64_t X, int64_t Y, int64_t Z, int64_t cx, int64_t cy, int64_t cz) {
  return cx >= 1 && cy >= 1 && cz >= 1 && cx <= X && cy <= Y && cz <= Z;
}

inline int grid_for(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return static_cast<int>(b < kMaxBlocks ? b : kMaxBlocks);
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_intake_occupancy(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                                        int32_t* flag_x, int32_t* flag_y, int32_t* flag_z,
                                        uint64_t* nonfinite, void* stream) {
  using namespace gts;
  if (!src || !flag_x || !flag_y || !flag_z || !nonfinite) return GTS_ERR_NULL;
  if (!volume_ok(X, Y, Z)) return GTS_ERR_SHAPE;
  if (dtype != kI16 && dtype != kF32) return GTS_ERR_ARGKIND;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(flag_x, 0, X * 4, st) != hipSuccess || hipMemsetAsync(flag_y, 0, Y * 4, st) != hipSuccess ||
      hipMemsetAsync(flag_z, 0, Z * 4, st) != hipSuccess || hipMemsetAsync(nonfinite, 0, 8, st) != hipSuccess)
    return launch_status();
  const int x = static_cast<int>(X), y = static_cast<int>(Y), z = static_cast<int>(Z);
  auto* bad = reinterpret_cast<unsigned long long*>(nonfinite);
  const int grid = grid_for(X * Y * Z);
  if (dtype == kI16)
    intake_occupancy_kernel<int16_t><<<grid, kBlock, 0, st>>>(static_cast<const int16_t*>(src), x, y, z, flag_x,
                                                              flag_y, flag_z, bad);
  else
    intake_occupancy_kernel<float><<<grid, kBlock, 0, st>>>(static_cast<const float*>(src), x, y, z, flag_x, flag_y,
                                                            flag_z, bad);
  return launch_status();
}

extern "C" int64_t gts_intake_select_workspace(void) { return gts::kLayout.total; }

extern "C" int32_t gts_intake_order_stats(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                                          const int32_t* xs, int64_t cx, const int32_t* ys, int64_t cy,
                                          const int32_t* zs, int64_t cz, int64_t rank_lo, int64_t rank_hi,
                                          float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!src || !xs || !ys || !zs || !out || !workspace) return GTS_ERR_NULL;
  if (!volume_ok(X, Y, Z) || !crop_ok(X, Y, Z, cx, cy, cz) || workspace_bytes < kLayout.total) return GTS_ERR_SHAPE;
  const int64_t n = cx * cy * cz;
  if (rank_lo < 0 || rank_hi < rank_lo || rank_hi >= n) return GTS_ERR_SHAPE;
  if (dtype != kI16 && dtype != kF32) return GTS_ERR_ARGKIND;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  unsigned* hist = reinterpret_cast<unsigned*>(ws + kLayout.hist);
  SelectState* state = reinterpret_cast<SelectState*>(ws + kLayout.state);
  const int x = static_cast<int>(X), y = static_cast<int>(Y), z = static_cast<int>(Z);
  const int grid = grid_for(n);
  intake_select_init_kernel<<<1, kBlock, 0, st>>>(hist, state, static_cast<unsigned long long>(rank_lo),
                                                  static_cast<unsigned long long>(rank_hi));
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (dtype == kI16)
      intake_hist_kernel<int16_t><<<grid, kBlock, 0, st>>>(static_cast<const int16_t*>(src), x, y, z, xs,
                                                           static_cast<int>(cx), ys, static_cast<int>(cy), zs,
                                                           static_cast<unsigned>(n), state, hist, shift);
    else
      intake_hist_kernel<float><<<grid, kBlock, 0, st>>>(static_cast<const float*>(src), x, y, z, xs,
                                                         static_cast<int>(cx), ys, static_cast<int>(cy), zs,
                                                         static_cast<unsigned>(n), state, hist, shift);
    intake_select_step_kernel<<<1, kBlock, 0, st>>>(hist, state, shift, shift == 0 ? out : nullptr);
  }
  return launch_status();
}

extern "C" int32_t gts_intake_standardize(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                                          const int32_t* xs, int64_t cx, const int32_t* ys, int64_t cy,
                                          const int32_t* zs, int64_t cz, const float* params, float* out,
                                          void* stream) {
  using namespace gts;
  if (!src || !xs || !ys || !zs || !params || !out) return GTS_ERR_NULL;
  if (!volume_ok(X, Y, Z) || !crop_ok(X, Y, Z, cx, cy, cz)) return GTS_ERR_SHAPE;
  if (dtype != kI16 && dtype != kF32) return GTS_ERR_ARGKIND;
  StandardizeParams p;
  for (int c = 0; c < kChannels; ++c) {
    p.top[c] = params[c];
    p.mean[c] = params[kChannels + c];
    p.std[c] = params[2 * kChannels + c];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((cx + kTileX - 1) / kTileX), static_cast<unsigned>(cy),
                  static_cast<unsigned>((cz + kTileZ - 1) / kTileZ));
  const int x = static_cast<int>(X), y = static_cast<int>(Y), z = static_cast<int>(Z);
  if (dtype == kI16)
    intake_standardize_kernel<int16_t><<<grid, kBlock, 0, st>>>(static_cast<const int16_t*>(src), x, y, z, xs,
                                                                static_cast<int>(cx), ys, static_cast<int>(cy), zs,
                                                                static_cast<int>(cz), p, out);
  else
    intake_standardize_kernel<float><<<grid, kBlock, 0, st>>>(static_cast<const float*>(src), x, y, z, xs,
                                                              static_cast<int>(cx), ys, static_cast<int>(cy), zs,
                                                              static_cast<int>(cz), p, out);
  return launch_status();
}
