// F1: conform a scan to the pipeline's frame (LPS axis order and signs, 1 mm voxels) and carry label volumes
// back onto the scan's own grid.  What a user otherwise does on the host with np.transpose / np.flip and
// scipy.ndimage.map_coordinates in front of the reader (data_processing/nifti_io.py:42-57 of the reference).
//
// One gather, [C][Z][Y][X] x-fastest in and out.  Every output axis names the input axis it reads and carries
// three host-computed tables over its own extent: the two input indices a sample lies between and the
// float64 weight of the second.  The kernel divides nothing and rounds nothing but the final float32.
//
//   exact      out = in[idx0 ...], the stored dtype, bit for bit (pure reorientation, and the inverse map);
//   trilinear  the eight neighbours (idx0 | idx1 per axis) through gts_scan.h's trilinear8 (float64, along input
//              x, then y, then z; t == 0 gives the voxel itself), one rounding to float32;
//   nearest    t < 0.5 ? idx0 : idx1 per axis, int16.
//
// Memory access.  Whatever the mode, the eight (or one) reads of an output voxel lie on input rows, so the
// reads of neighbouring voxels ALONG THE INPUT'S x are the coalesced ones:
//   rows   the output's x reads the input's x: one lane per output voxel in linear order.  Reads and writes
//          both run along x (ascending, or descending for a flipped x).  An exact copy whose rows are whole
//          16-byte groups moves 16 bytes per lane, reversed in registers when x is flipped;
//   tiled  the output's x reads the input's y or z (4 of the 6 permutations): a 64 x 64 tile over (output x,
//          the output axis that reads input x).  Loading, a wave's lanes run along input x; the finished values
//          go through LDS; storing, the lanes run along output x (gts_scan.h's cross_tile64: one 32-bit word per
//          value, an int16 widened to int32, and the bank arithmetic of its pitch).
// Table entries are clamped to the input extent before use, so no table can make a read leave the volume.
#include "gts_scan.h"

namespace gts {
namespace {

constexpr int kModeExact = 0, kModeTrilinear = 1, kModeNearest = 2;

// Tables and extents ordered by INPUT axis j (0 = x, fastest): which output axis drives it, and that axis'
// tables.  t is unused (may be NULL) in exact mode, idx1 likewise.
struct ConformArgs {
  const int32_t* idx0[3];
  const int32_t* idx1[3];
  const double* t[3];
  int drive[3];  // output axis whose coordinate indexes input axis j's tables
  int in[3];     // input extents X, Y, Z
  int out[3];    // output extents OX, OY, OZ
  int channels;
};

__device__ __forceinline__ int pick(int axis, int o0, int o1, int o2) { return axis == 0 ? o0 : (axis == 1 ? o1 : o2); }
__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// The value of output voxel (o0, o1, o2) of channel c.
template <typename In, typename Out, int kMode>
__device__ __forceinline__ Out fetch(const In* __restrict__ src, const ConformArgs& p, int c, int o0, int o1, int o2) {
  const int ix = pick(p.drive[0], o0, o1, o2), iy = pick(p.drive[1], o0, o1, o2), iz = pick(p.drive[2], o0, o1, o2);
  const int X = p.in[0], Y = p.in[1], Z = p.in[2];
  const In* vol = src + static_cast<int64_t>(c) * Z * Y * X;
  if (kMode == kModeTrilinear) {
    const int x0 = clamp_index(p.idx0[0][ix], X), x1 = clamp_index(p.idx1[0][ix], X);
    const int y0 = clamp_index(p.idx0[1][iy], Y), y1 = clamp_index(p.idx1[1][iy], Y);
    const int z0 = clamp_index(p.idx0[2][iz], Z), z1 = clamp_index(p.idx1[2][iz], Z);
    const double tx = p.t[0][ix], ty = p.t[1][iy], tz = p.t[2][iz];
    return static_cast<Out>(static_cast<float>(trilinear8(vol, X, Y, x0, x1, y0, y1, z0, z1, tx, ty, tz)));
  }
  int x, y, z;
  if (kMode == kModeNearest) {
    x = p.t[0][ix] < 0.5 ? p.idx0[0][ix] : p.idx1[0][ix];
    y = p.t[1][iy] < 0.5 ? p.idx0[1][iy] : p.idx1[1][iy];
    z = p.t[2][iz] < 0.5 ? p.idx0[2][iz] : p.idx1[2][iz];
  } else {
    x = p.idx0[0][ix];
    y = p.idx0[1][iy];
    z = p.idx0[2][iz];
  }
  return static_cast<Out>(vol[(static_cast<int64_t>(clamp_index(z, Z)) * Y + clamp_index(y, Y)) * X + clamp_index(x, X)]);
}

// rows: one lane per output voxel, linear order.
template <typename In, typename Out, int kMode>
__global__ __launch_bounds__(kBlock) void conform_rows_kernel(const In* __restrict__ src, Out* __restrict__ dst,
                                                              const ConformArgs p, int64_t total) {
  const int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  if (i >= total) return;
  const int o0 = static_cast<int>(i % p.out[0]);
  const int64_t row = i / p.out[0];
  const int o1 = static_cast<int>(row % p.out[1]);
  const int64_t plane = row / p.out[1];
  const int o2 = static_cast<int>(plane % p.out[2]);
  dst[i] = fetch<In, Out, kMode>(src, p, static_cast<int>(plane / p.out[2]), o0, o1, o2);
}

// rows, exact, 16 bytes per lane: the host side has checked that the output's x reads the input's x, that both
// row lengths are whole groups of kVec values and that both volumes start on a 16-byte boundary.  A group whose
// x entries are the kVec consecutive indices of one aligned input group, ascending or descending, moves as one
// load and one store; any other group falls back to kVec single reads.
template <typename T>
__global__ __launch_bounds__(kBlock) void conform_rows_wide_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                                   const ConformArgs p, int64_t groups) {
  constexpr int kVec = 16 / static_cast<int>(sizeof(T));
  typedef T Group __attribute__((ext_vector_type(kVec)));
  const int64_t g = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  if (g >= groups) return;
  const int per_row = p.out[0] / kVec;
  const int o0 = static_cast<int>(g % per_row) * kVec;
  const int64_t row = g / per_row;
  const int o1 = static_cast<int>(row % p.out[1]);
  const int64_t plane = row / p.out[1];
  const int o2 = static_cast<int>(plane % p.out[2]);
  const int c = static_cast<int>(plane / p.out[2]);
  const int X = p.in[0], Y = p.in[1], Z = p.in[2];
  const int iy = pick(p.drive[1], o0, o1, o2), iz = pick(p.drive[2], o0, o1, o2);
  const int y = clamp_index(p.idx0[1][iy], Y), z = clamp_index(p.idx0[2][iz], Z);
  const T* in_row = src + ((static_cast<int64_t>(c) * Z + z) * Y + y) * X;
  int xs[kVec];
  bool up = true, down = true;
#pragma unroll
  for (int k = 0; k < kVec; ++k) {
    xs[k] = clamp_index(p.idx0[0][o0 + k], X);
    up = up && xs[k] == xs[0] + k;
    down = down && xs[k] == xs[0] - k;
  }
  Group v;
  if (up && xs[0] % kVec == 0) {
    v = *reinterpret_cast<const Group*>(in_row + xs[0]);
  } else if (down && xs[kVec - 1] % kVec == 0) {
    const Group w = *reinterpret_cast<const Group*>(in_row + xs[kVec - 1]);
#pragma unroll
    for (int k = 0; k < kVec; ++k) v[k] = w[kVec - 1 - k];
  } else {
#pragma unroll
    for (int k = 0; k < kVec; ++k) v[k] = in_row[xs[k]];
  }
  *reinterpret_cast<Group*>(dst + g * kVec) = v;
}

// tiled: the output's x reads input y or z; output axis ka (1 or 2) reads input x, kb is the third one.
// Block = one 64 x 64 tile over (output x, output ka) at one (kb, channel).
template <typename In, typename Out, int kMode>
__global__ __launch_bounds__(kBlock) void conform_tiled_kernel(const In* __restrict__ src, Out* __restrict__ dst,
                                                               const ConformArgs p, int ka, int tiles_x, int tiles_a) {
  int64_t b = blockIdx.x;
  const int tx0 = static_cast<int>(b % tiles_x) * kTile;
  b /= tiles_x;
  const int ta0 = static_cast<int>(b % tiles_a) * kTile;
  b /= tiles_a;
  const int OX = p.out[0], OA = ka == 1 ? p.out[1] : p.out[2], OB = ka == 1 ? p.out[2] : p.out[1];
  const int ob = static_cast<int>(b % OB);
  const int c = static_cast<int>(b / OB);
  using Word = decltype(Out{} + 0);  // float, or the int an int16 widens to
  cross_tile64<Word>(
      tx0, ta0, OX, OA,
      [&](int ox, int oa) { return fetch<In, Out, kMode>(src, p, c, ox, ka == 1 ? oa : ob, ka == 1 ? ob : oa); },
      [&](int ox, int oa, Word w) {
        const int o1 = ka == 1 ? oa : ob, o2 = ka == 1 ? ob : oa;
        dst[((static_cast<int64_t>(c) * p.out[2] + o2) * p.out[1] + o1) * OX + ox] = static_cast<Out>(w);
      });
}

template <typename In, typename Out, int kMode>
int launch(const void* src, void* dst, const ConformArgs& p, hipStream_t st) {
  const In* s = static_cast<const In*>(src);
  Out* d = static_cast<Out*>(dst);
  const int64_t per_channel = int64_t{p.out[0]} * p.out[1] * p.out[2];
  const int64_t total = per_channel * p.channels;
  if (p.drive[0] == 0) {
    constexpr int kVec = 16 / static_cast<int>(sizeof(In));
    const bool wide = kMode == kModeExact && p.in[0] % kVec == 0 && p.out[0] % kVec == 0 &&
                      reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
    if (wide) {
      const int64_t groups = total / kVec;
      conform_rows_wide_kernel<In><<<blocks_for(groups, kBlock), kBlock, 0, st>>>(
          s, reinterpret_cast<In*>(d), p, groups);
    } else {
      conform_rows_kernel<In, Out, kMode><<<blocks_for(total, kBlock), kBlock, 0, st>>>(s, d, p, total);
    }
    return launch_status();
  }
  const int ka = p.drive[0], kb = 3 - ka;
  const int tiles_x = (p.out[0] + kTile - 1) / kTile, tiles_a = (p.out[ka] + kTile - 1) / kTile;
  const int64_t blocks = int64_t{tiles_x} * tiles_a * p.out[kb] * p.channels;  // <= total < 2^31
  conform_tiled_kernel<In, Out, kMode><<<static_cast<unsigned>(blocks), kBlock, 0, st>>>(s, d, p, ka, tiles_x, tiles_a);
  return launch_status();
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_conform_gather(const void* src, int32_t dtype, int64_t C, int64_t X, int64_t Y, int64_t Z,
                                      int32_t axis0, int32_t axis1, int32_t axis2, int64_t OX, int64_t OY, int64_t OZ,
                                      const int32_t* idx0, const int32_t* idx1, const double* t, int32_t mode, void* dst,
                                      void* stream) {
  using namespace gts;
  if (mode != kModeExact && mode != kModeTrilinear && mode != kModeNearest) return GTS_ERR_ARGKIND;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  if (mode == kModeNearest && dtype != kI16) return GTS_ERR_ARGKIND;
  if (!src || !dst || !idx0) return GTS_ERR_NULL;
  if (mode != kModeExact && (!idx1 || !t)) return GTS_ERR_NULL;
  if (C < 0) return GTS_ERR_SHAPE;
  const int64_t in_dims[3] = {X, Y, Z}, out_dims[3] = {OX, OY, OZ};
  for (int k = 0; k < 3; ++k)
    if (!scan_extent_ok(in_dims[k]) || !scan_extent_ok(out_dims[k])) return GTS_ERR_SHAPE;
  const int32_t axes[3] = {axis0, axis1, axis2};
  int seen = 0;
  for (int k = 0; k < 3; ++k) {
    if (axes[k] < 0 || axes[k] > 2) return GTS_ERR_ARGKIND;
    seen |= 1 << axes[k];
  }
  if (seen != 7) return GTS_ERR_ARGKIND;
  if (C == 0) return GTS_OK;
  if (!scan_extents_ok(X, Y, Z) || !scan_extents_ok(OX, OY, OZ)) return GTS_ERR_SHAPE;
  int64_t all;  // a lane's linear index covers every channel: C volumes are one volume of C planes
  if (!volume_voxels(X * Y * Z, C, 1, false, &all) || !volume_voxels(OX * OY * OZ, C, 1, false, &all)) return GTS_ERR_SHAPE;
  ConformArgs p;
  int64_t at = 0;
  for (int k = 0; k < 3; ++k) {  // output axis k reads input axis axes[k]; its tables start at `at`
    const int j = axes[k];
    p.idx0[j] = idx0 + at;
    p.idx1[j] = idx1 ? idx1 + at : nullptr;
    p.t[j] = t ? t + at : nullptr;
    p.drive[j] = k;
    p.in[k] = static_cast<int>(in_dims[k]);
    p.out[k] = static_cast<int>(out_dims[k]);
    at += out_dims[k];
  }
  p.channels = static_cast<int>(C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == kModeNearest) return launch<int16_t, int16_t, kModeNearest>(src, dst, p, st);
  if (mode == kModeTrilinear)
    return dtype == kI16 ? launch<int16_t, float, kModeTrilinear>(src, dst, p, st)
                      : launch<float, float, kModeTrilinear>(src, dst, p, st);
  return dtype == kI16 ? launch<int16_t, int16_t, kModeExact>(src, dst, p, st)
                    : launch<float, float, kModeExact>(src, dst, p, st);
}
