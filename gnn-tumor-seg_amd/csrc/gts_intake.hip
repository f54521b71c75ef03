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
//       and share one histogram while their prefixes agree (the select lives in gts_select.h, shared
//       with D2 of gts_dataset_stats.hip, which names its elements by a bit mask instead);
//   I3  fused gather + ((x / top_c) - mean_c) / std_c in IEEE float32 (-ffp-contract=off, correctly
//       rounded division) into C-order [cx, cy, cz, 4]: a 64 (x) x 16 (z) tile per workgroup is read
//       along x into LDS and written along z with one 16-byte store per voxel.
#include "gts_select.h"

namespace gts {
namespace {

constexpr int kTileX = 64, kTileZ = 16;

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
  mine = wave_sum(mine);
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

inline bool crop_ok(int64_t X, int64_t Y, int64_t Z, int64_t cx, int64_t cy, int64_t cz) {
  return cx >= 1 && cy >= 1 && cz >= 1 && cx <= X && cy <= Y && cz <= Z;
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_intake_occupancy(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                                        int32_t* flag_x, int32_t* flag_y, int32_t* flag_z,
                                        uint64_t* nonfinite, void* stream) {
  using namespace gts;
  if (!src || !flag_x || !flag_y || !flag_z || !nonfinite) return GTS_ERR_NULL;
  if (!volume_ok(X, Y, Z)) return GTS_ERR_SHAPE;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(flag_x, 0, X * 4, st) != hipSuccess || hipMemsetAsync(flag_y, 0, Y * 4, st) != hipSuccess ||
      hipMemsetAsync(flag_z, 0, Z * 4, st) != hipSuccess || hipMemsetAsync(nonfinite, 0, 8, st) != hipSuccess)
    return launch_status();
  const int x = static_cast<int>(X), y = static_cast<int>(Y), z = static_cast<int>(Z);
  auto* bad = reinterpret_cast<unsigned long long*>(nonfinite);
  const int grid = blocks_for(X * Y * Z, kBlock, kMaxBlocks);
  return with_scan_type(dtype, src, [&](auto* s) {
    intake_occupancy_kernel<<<grid, kBlock, 0, st>>>(s, x, y, z, flag_x, flag_y, flag_z, bad);
    return launch_status();
  });
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
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const CropSource source{xs, ys, zs, static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(X),
                          static_cast<int>(Y), static_cast<int>(Z)};
  const size_t vol = static_cast<size_t>(X * Y * Z);
  return with_scan_type(dtype, src, [&](auto* s) {
    run_select(s, vol, source, n, rank_lo, rank_hi, out, workspace, st);
    return launch_status();
  });
}

extern "C" int32_t gts_intake_standardize(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                                          const int32_t* xs, int64_t cx, const int32_t* ys, int64_t cy,
                                          const int32_t* zs, int64_t cz, const float* params, float* out,
                                          void* stream) {
  using namespace gts;
  if (!src || !xs || !ys || !zs || !params || !out) return GTS_ERR_NULL;
  if (!volume_ok(X, Y, Z) || !crop_ok(X, Y, Z, cx, cy, cz)) return GTS_ERR_SHAPE;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
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
  return with_scan_type(dtype, src, [&](auto* s) {
    intake_standardize_kernel<<<grid, kBlock, 0, st>>>(s, x, y, z, xs, static_cast<int>(cx), ys, static_cast<int>(cy), zs,
                                                       static_cast<int>(cz), p, out);
    return launch_status();
  });
}
