// Training-time augmentation on the GPU: mirrored crops, per-modality intensity jitter and
// additive Gaussian noise, as two streaming kernels that write fresh outputs.
//
// A1 (augment_crop_kernel)      x [cx, cy, cz, C] channels-last, labels [V] int64:
//   x'[i, j, k, c] = x[i', j', k', c] * a_c + b_c + s_c * n(v, c)   (c < Ci)      x[i', j', k', c]   (c >= Ci)
//   labels'[v]     = labels[v']              i' = cx - 1 - i on a mirrored axis, v the linear index of the OUTPUT voxel
// A2 (augment_features_kernel)  feats [N, F], one (a, b) per (graph, modality), m(f) = f / (F / M):
//   out[r, f] = feats[r, f] * a_{g(r), m(f)} + b_{g(r), m(f)} + s * n(r, f)
//
// One thread owns four consecutive channels of one voxel (or features of one row): its store is one 16-byte access at
// 16 * thread, so the stores are coalesced whatever is mirrored; the mirror is on the read side, where a wave still
// reads whole 16-byte pieces of a few contiguous segments.  Where C % 4 != 0 (or a base is not 16-byte aligned) the
// same thread moves its channels float by float.
//
// Rounding: the affine is a multiply and then an add, each rounded to float32 (the library is built with
// -ffp-contract=off: no fma), which is what numpy's float32 `x * a + b` does.  A channel with a == 1 and b == 0 is
// copied and a channel with s == 0 adds nothing, so an identity plan returns its input bit for bit (-0.0 stays -0.0).
//
// Noise: Philox4x32-10, key (seed_lo, seed_hi), counter (idx_lo, idx_hi | (c / 4) << 24 | stream << 31, step_lo,
// step_hi); idx is the output voxel (stream 0, A1) or the row (stream 1, A2), below 2^56, and c < 512.  The four
// output words give the normals of channels 4 (c / 4) .. 4 (c / 4) + 3 by Box-Muller: from words (w0, w1)
//   u = ((w0 >> 8) + 1) 2^-24,  t = 2 pi (w1 >> 8) 2^-24,  r = sqrt(-2 ln u):   normal 0 = r cos t, normal 1 = r sin t
// and normals 2, 3 likewise from (w2, w3).  A value depends on (seed, step, idx, c) alone, not on the launch geometry.
//
// A3 (augment_spatial_kernel)  A1 with a rotation + zoom between the mirror and the affine: output
//   voxel o, mirrored to o', reads the source point p = c + M (o' - c), c = (n - 1) / 2, in float64 without fma:
//   p_a = c_a + ((M[a][0] d_0 + M[a][1] d_1) + M[a][2] d_2), clamped into [-2, n_a + 1]; f = floor(p), t = p - f.
//   Float channels: the eight corners (f_a | f_a + 1), 0.0 where any index leaves the crop, lerped along x, then y,
//   then z as a + (b - a) t in float64, rounded once to float32, then A1's affine and noise (v the OUTPUT voxel).
//   Labels: labels[floor(p + 0.5)], 0 outside the crop.
// A4 (augment_spatial_bwd_kernel)  the adjoint of A3's resample and mirror in gather form: one thread per (source
//   voxel q, four channels) walks the output voxels o' of the box c + M^-1 (q - c) +- (h + 1), h_a = sum_b |M^-1[a][b]|,
//   in ascending C-order, recomputes p(o') by A3's expression and adds w(o, q) dy[o] in float64, w the product of the
//   per-axis lerp weights (1 - t where f == q, t where f + 1 == q, else 0).  No atomics: two runs are bit-equal.
#include "gts_common.h"

#include <math.h>

namespace gts {
namespace {

constexpr int kMaxAugChannels = 512;     // (c / 4) << 24 must stay below bit 31 of counter word 1

struct PhiloxKey {
  uint32_t seed_lo, seed_hi, step_lo, step_hi;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// the four normals of channel group `group` at index `idx` of stream `stream` (0: A1 voxels, 1: A2 rows)
__device__ __forceinline__ void normals4(int64_t idx, int group, uint32_t stream, const PhiloxKey& key,
                                         float (&n)[4]) {
  const uint64_t u = static_cast<uint64_t>(idx);
  uint32_t w[4];
  philox4x32_10(static_cast<uint32_t>(u), static_cast<uint32_t>(u >> 32) | (static_cast<uint32_t>(group) << 24) |
                                              (stream << 31),
                key.step_lo, key.step_hi, key.seed_lo, key.seed_hi, w);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float uni = static_cast<float>((w[2 * p] >> 8) + 1u) * 0x1p-24f;
    const float theta = 6.283185307179586f * (static_cast<float>(w[2 * p + 1] >> 8) * 0x1p-24f);
    const float r = sqrtf(-2.0f * logf(uni));
    n[2 * p] = r * cosf(theta);
    n[2 * p + 1] = r * sinf(theta);
  }
}

__device__ __forceinline__ float affine(float x, float a, float b) { return (a == 1.0f && b == 0.0f) ? x : x * a + b; }

// A1.  VEC: C % 4 == 0 and both bases 16-byte aligned.  params: [ci][3] = (a, b, sigma) per image channel (device).
// Thread q < v_total * groups owns channels 4 g .. 4 g + 3 (below C) of output voxel v = q / groups; the threads with
// g == 0 also move the voxel's label.  Idx: the type the thread index is taken apart in, uint32_t where the whole
// launch has fewer than 2^32 threads (64-bit divisions cost this kernel more than its memory traffic), else int64_t.
template <bool VEC, typename Idx>
__global__ __launch_bounds__(kBlock) void augment_crop_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ labels, const float* __restrict__ params,
    float* __restrict__ x_out, int64_t* __restrict__ labels_out, int64_t cx, int64_t cy, int64_t cz, int channels,
    int ci, int groups, int flip_mask, PhiloxKey key) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= cx * cy * cz * groups) return;
  const Idx qv = static_cast<Idx>(q) / static_cast<Idx>(groups), qij = qv / static_cast<Idx>(cz),
            qi = qij / static_cast<Idx>(cy);
  const int64_t v = static_cast<int64_t>(qv), i = static_cast<int64_t>(qi);
  const int g = static_cast<int>(q - v * groups);
  const int64_t k = v - static_cast<int64_t>(qij) * cz, j = static_cast<int64_t>(qij) - i * cy;
  const int64_t si = (flip_mask & 1) ? cx - 1 - i : i, sj = (flip_mask & 2) ? cy - 1 - j : j,
                sk = (flip_mask & 4) ? cz - 1 - k : k;
  const int64_t sv = (si * cy + sj) * cz + sk;
  if (labels != nullptr && g == 0) labels_out[v] = labels[sv];
  if (x == nullptr) return;
  const int c0 = 4 * g;
  const int nc = channels - c0 < 4 ? channels - c0 : 4;
  const float* src = x + sv * channels + c0;
  float* dst = x_out + v * channels + c0;
  float val[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    const Vec<4> t = Vec<4>::load_nt(src);
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = t.v[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nc) val[c] = src[c];
  }
  if (c0 < ci) {        // image channels in this group: (a, b, sigma) each, channels past ci pass through
    float a[4], b[4], s[4];
    bool noisy = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool image = c0 + c < ci;
      const float* p = params + 3 * (image ? c0 + c : 0);
      a[c] = image ? p[0] : 1.0f;
      b[c] = image ? p[1] : 0.0f;
      s[c] = image ? p[2] : 0.0f;
      noisy = noisy || s[c] != 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = affine(val[c], a[c], b[c]);
    if (noisy) {
      float n[4];
      normals4(v, g, 0u, key, n);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (s[c] != 0.0f) val[c] = val[c] + s[c] * n[c];
    }
  }
  if constexpr (VEC) {
    Vec<4>{{val[0], val[1], val[2], val[3]}}.store_nt(dst);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nc) dst[c] = val[c];
  }
}

// A2.  row_ptr [n_graphs + 1] ascending from 0 to n_rows (device; checked by the caller on its host copy);
// params [n_graphs][modalities][2] = (a, b).  Thread q < n_rows * groups owns features 4 g .. 4 g + 3 of row q / groups.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void augment_features_kernel(
    const float* __restrict__ feats, const int64_t* __restrict__ row_ptr, const float* __restrict__ params,
    float* __restrict__ out, int64_t n_rows, int n_feats, int modalities, int n_graphs, int groups, float sigma,
    PhiloxKey key) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t r = q / groups;
  if (r >= n_rows) return;
  const int g = static_cast<int>(q - r * groups);
  // the graph that owns row r: the last one whose first row is <= r (graphs without rows own none)
  int lo = 0, hi = n_graphs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (row_ptr[mid] <= r) lo = mid; else hi = mid;
  }
  const float* graph_params = params + static_cast<int64_t>(lo) * modalities * 2;
  const int per_modality = n_feats / modalities;
  const int f0 = 4 * g;
  const int nf = n_feats - f0 < 4 ? n_feats - f0 : 4;
  const float* src = feats + r * n_feats + f0;
  float* dst = out + r * n_feats + f0;
  float val[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    const Vec<4> t = Vec<4>::load_nt(src);
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = t.v[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nf) val[c] = src[c];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int m = (c < nf ? f0 + c : f0) / per_modality;
    val[c] = affine(val[c], graph_params[2 * m], graph_params[2 * m + 1]);
  }
  if (sigma != 0.0f) {
    float n[4];
    normals4(r, g, 1u, key, n);
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = val[c] + sigma * n[c];
  }
  if constexpr (VEC) {
    Vec<4>{{val[0], val[1], val[2], val[3]}}.store_nt(dst);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nf) dst[c] = val[c];
  }
}

// The source point of mirrored output voxel (i, j, k): the one expression A3 and A4 share, so that A4's weights are
// those A3 used.  c = (n - 1) / 2 and d = o' - c are exact; the clamp keeps every later integer conversion in range
// (fmax / fmin also send a NaN to the bound) and moves no point that has a corner inside the crop.
struct SpatialMap {
  double m[9];
  double c[3];
};

__device__ __forceinline__ double source_coord(const SpatialMap& map, int a, double d0, double d1, double d2,
                                               int64_t extent) {
  const double p = map.c[a] + ((map.m[3 * a] * d0 + map.m[3 * a + 1] * d1) + map.m[3 * a + 2] * d2);
  return fmin(fmax(p, -2.0), static_cast<double>(extent) + 1.0);
}

// A3.  Ownership, VEC and Idx as A1; `map` travels by value in the kernel arguments.
template <bool VEC, typename Idx>
__global__ __launch_bounds__(kBlock) void augment_spatial_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ labels, const float* __restrict__ params,
    float* __restrict__ x_out, int64_t* __restrict__ labels_out, int64_t cx, int64_t cy, int64_t cz, int channels,
    int ci, int groups, int flip_mask, PhiloxKey key, SpatialMap map) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= cx * cy * cz * groups) return;
  const Idx qv = static_cast<Idx>(q) / static_cast<Idx>(groups), qij = qv / static_cast<Idx>(cz),
            qi = qij / static_cast<Idx>(cy);
  const int64_t v = static_cast<int64_t>(qv), i = static_cast<int64_t>(qi);
  const int g = static_cast<int>(q - v * groups);
  const int64_t k = v - static_cast<int64_t>(qij) * cz, j = static_cast<int64_t>(qij) - i * cy;
  const int64_t si = (flip_mask & 1) ? cx - 1 - i : i, sj = (flip_mask & 2) ? cy - 1 - j : j,
                sk = (flip_mask & 4) ? cz - 1 - k : k;
  const double d0 = static_cast<double>(si) - map.c[0], d1 = static_cast<double>(sj) - map.c[1],
               d2 = static_cast<double>(sk) - map.c[2];
  const double p0 = source_coord(map, 0, d0, d1, d2, cx), p1 = source_coord(map, 1, d0, d1, d2, cy),
               p2 = source_coord(map, 2, d0, d1, d2, cz);
  if (labels != nullptr && g == 0) {
    const int64_t mi = static_cast<int64_t>(floor(p0 + 0.5)), mj = static_cast<int64_t>(floor(p1 + 0.5)),
                  mk = static_cast<int64_t>(floor(p2 + 0.5));
    const bool inside = mi >= 0 && mi < cx && mj >= 0 && mj < cy && mk >= 0 && mk < cz;
    labels_out[v] = inside ? labels[(mi * cy + mj) * cz + mk] : 0;
  }
  if (x == nullptr) return;
  const int c0 = 4 * g;
  const int nc = channels - c0 < 4 ? channels - c0 : 4;
  const double f0 = floor(p0), f1 = floor(p1), f2 = floor(p2);
  const double t0 = p0 - f0, t1 = p1 - f1, t2 = p2 - f2;
  const int64_t fi = static_cast<int64_t>(f0), fj = static_cast<int64_t>(f1), fk = static_cast<int64_t>(f2);
  double along_y[2][4];      // [dz][c]: lerped along x, then y
#pragma unroll
  for (int dz = 0; dz < 2; ++dz) {
    double along_x[2][4];    // [dy][c]
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      float corner[2][4];
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int64_t ii = fi + dx, jj = fj + dy, kk = fk + dz;
#pragma unroll
        for (int c = 0; c < 4; ++c) corner[dx][c] = 0.0f;
        if (ii >= 0 && ii < cx && jj >= 0 && jj < cy && kk >= 0 && kk < cz) {      // zero border
          const float* src = x + ((ii * cy + jj) * cz + kk) * channels + c0;
          if constexpr (VEC) {
            const Vec<4> t = Vec<4>::load(src);
#pragma unroll
            for (int c = 0; c < 4; ++c) corner[dx][c] = t.v[c];
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (c < nc) corner[dx][c] = src[c];
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double a = static_cast<double>(corner[0][c]), b = static_cast<double>(corner[1][c]);
        along_x[dy][c] = a + (b - a) * t0;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) along_y[dz][c] = along_x[0][c] + (along_x[1][c] - along_x[0][c]) * t1;
  }
  float val[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) val[c] = static_cast<float>(along_y[0][c] + (along_y[1][c] - along_y[0][c]) * t2);
  float* dst = x_out + v * channels + c0;
  if (c0 < ci) {        // A1's affine and noise on the image channels of this group
    float a[4], b[4], s[4];
    bool noisy = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool image = c0 + c < ci;
      const float* p = params + 3 * (image ? c0 + c : 0);
      a[c] = image ? p[0] : 1.0f;
      b[c] = image ? p[1] : 0.0f;
      s[c] = image ? p[2] : 0.0f;
      noisy = noisy || s[c] != 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = affine(val[c], a[c], b[c]);
    if (noisy) {
      float n[4];
      normals4(v, g, 0u, key, n);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (s[c] != 0.0f) val[c] = val[c] + s[c] * n[c];
    }
  }
  if constexpr (VEC) {
    Vec<4>{{val[0], val[1], val[2], val[3]}}.store_nt(dst);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nc) dst[c] = val[c];
  }
}

// What A4 needs beside the map: M^-1 and the half extents h of the box of output voxels that can reach one source voxel.
struct SpatialInverse {
  double inv[9];
  double h[3];
};

// the weight axis a gives source index qa at source coordinate p
__device__ __forceinline__ double axis_weight(double p, double qa) {
  const double f = floor(p), t = p - f;
  return f == qa ? 1.0 - t : (f + 1.0 == qa ? t : 0.0);
}

// A4.  Thread q < v_total * groups owns channels 4 g .. 4 g + 3 of SOURCE voxel q / groups.  The box is clipped to the
// crop in float64 before it becomes integers; a candidate outside the footprint has weight exactly 0 and is skipped.
template <bool VEC, typename Idx>
__global__ __launch_bounds__(kBlock) void augment_spatial_bwd_kernel(
    const float* __restrict__ dy, float* __restrict__ dx, int64_t cx, int64_t cy, int64_t cz, int channels, int groups,
    int flip_mask, SpatialMap map, SpatialInverse back) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= cx * cy * cz * groups) return;
  const Idx qv = static_cast<Idx>(q) / static_cast<Idx>(groups), qij = qv / static_cast<Idx>(cz),
            qi = qij / static_cast<Idx>(cy);
  const int64_t v = static_cast<int64_t>(qv), i = static_cast<int64_t>(qi);
  const int g = static_cast<int>(q - v * groups);
  const int64_t k = v - static_cast<int64_t>(qij) * cz, j = static_cast<int64_t>(qij) - i * cy;
  const int c0 = 4 * g;
  const int nc = channels - c0 < 4 ? channels - c0 : 4;
  const int64_t extent[3] = {cx, cy, cz};
  const double qa[3] = {static_cast<double>(i), static_cast<double>(j), static_cast<double>(k)};
  const double e0 = qa[0] - map.c[0], e1 = qa[1] - map.c[1], e2 = qa[2] - map.c[2];
  int64_t lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double centre = map.c[a] + ((back.inv[3 * a] * e0 + back.inv[3 * a + 1] * e1) + back.inv[3 * a + 2] * e2);
    const double top = static_cast<double>(extent[a]) - 1.0;
    lo[a] = static_cast<int64_t>(fmin(fmax(ceil(centre - back.h[a]) - 1.0, 0.0), top + 1.0));
    hi[a] = static_cast<int64_t>(fmax(fmin(floor(centre + back.h[a]) + 1.0, top), -1.0));
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t oi = lo[0]; oi <= hi[0]; ++oi) {
    const double d0 = static_cast<double>(oi) - map.c[0];
    const int64_t yi = (flip_mask & 1) ? cx - 1 - oi : oi;
    for (int64_t oj = lo[1]; oj <= hi[1]; ++oj) {
      const double d1 = static_cast<double>(oj) - map.c[1];
      const int64_t yj = (flip_mask & 2) ? cy - 1 - oj : oj;
      for (int64_t ok = lo[2]; ok <= hi[2]; ++ok) {
        const double d2 = static_cast<double>(ok) - map.c[2];
        const double w0 = axis_weight(source_coord(map, 0, d0, d1, d2, cx), qa[0]);
        if (w0 == 0.0) continue;
        const double w1 = axis_weight(source_coord(map, 1, d0, d1, d2, cy), qa[1]);
        if (w1 == 0.0) continue;
        const double w2 = axis_weight(source_coord(map, 2, d0, d1, d2, cz), qa[2]);
        const double w = (w0 * w1) * w2;
        if (w == 0.0) continue;
        const int64_t yk = (flip_mask & 4) ? cz - 1 - ok : ok;
        const float* src = dy + ((yi * cy + yj) * cz + yk) * channels + c0;
        if constexpr (VEC) {
          const Vec<4> t = Vec<4>::load(src);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = acc[c] + w * static_cast<double>(t.v[c]);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < nc) acc[c] = acc[c] + w * static_cast<double>(src[c]);
        }
      }
    }
  }
  float* dst = dx + v * channels + c0;
  if constexpr (VEC) {
    Vec<4>{{static_cast<float>(acc[0]), static_cast<float>(acc[1]), static_cast<float>(acc[2]),
            static_cast<float>(acc[3])}}.store_nt(dst);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nc) dst[c] = static_cast<float>(acc[c]);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline PhiloxKey philox_key(uint64_t seed, uint64_t step) {
  return PhiloxKey{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(step),
                   static_cast<uint32_t>(step >> 32)};
}


constexpr double kMaxSpatialReach = 8.0;      // the largest h_a A4 walks: a box of at most 19^3 candidates

// Reads the HOST matrix M [3][3]: GTS_ERR_ARGKIND for a non-finite entry, a singular M (no finite inverse) or a half
// extent h_a = sum_b |M^-1[a][b]| above kMaxSpatialReach; else the map for extents (cx, cy, cz) and M^-1 with h.
inline int spatial_setup(const double* matrix, int64_t cx, int64_t cy, int64_t cz, SpatialMap* map,
                         SpatialInverse* back) {
  for (int e = 0; e < 9; ++e) {
    if (!isfinite(matrix[e])) return GTS_ERR_ARGKIND;
    map->m[e] = matrix[e];
  }
  map->c[0] = static_cast<double>(cx - 1) / 2.0;
  map->c[1] = static_cast<double>(cy - 1) / 2.0;
  map->c[2] = static_cast<double>(cz - 1) / 2.0;
  const double* m = matrix;
  const double cof[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                         m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                         m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
  const double det = (m[0] * cof[0] + m[1] * cof[3]) + m[2] * cof[6];
  if (!isfinite(det) || det == 0.0) return GTS_ERR_ARGKIND;
  for (int a = 0; a < 3; ++a) {
    back->h[a] = 0.0;
    for (int b = 0; b < 3; ++b) {
      back->inv[3 * a + b] = cof[3 * a + b] / det;
      if (!isfinite(back->inv[3 * a + b])) return GTS_ERR_ARGKIND;
      back->h[a] += fabs(back->inv[3 * a + b]);
    }
    if (!(back->h[a] <= kMaxSpatialReach)) return GTS_ERR_ARGKIND;
  }
  return GTS_OK;
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_augment_crop_f32(const float* x, const int64_t* labels, const float* params, float* x_out,
                                        int64_t* labels_out, int64_t cx, int64_t cy, int64_t cz, int64_t channels,
                                        int64_t image_channels, int32_t flip_mask, uint64_t seed, uint64_t step,
                                        void* stream) {
  using namespace gts;
  if (x == nullptr && labels == nullptr) return GTS_ERR_NULL;
  if ((x != nullptr && x_out == nullptr) || (labels != nullptr && labels_out == nullptr)) return GTS_ERR_NULL;
  if (cx < 0 || cy < 0 || cz < 0 || channels < 0 || image_channels < 0) return GTS_ERR_SHAPE;
  if (flip_mask < 0 || flip_mask > 7) return GTS_ERR_ARGKIND;
  if (x != nullptr && (channels < 1 || channels > kMaxAugChannels || image_channels > channels)) return GTS_ERR_SHAPE;
  if (x != nullptr && image_channels > 0 && params == nullptr) return GTS_ERR_NULL;
  if (x == nullptr && image_channels != 0) return GTS_ERR_SHAPE;
  // extents below 2^31 each, the voxel count below 2^56 (the counter's index field) and the grid below 2^31 blocks
  const int64_t lim = (1LL << 31) - 1;
  if (cx > lim || cy > lim || cz > lim) return GTS_ERR_SHAPE;
  if (cx == 0 || cy == 0 || cz == 0) return GTS_OK;
  if (cx > (1LL << 56) / cy / cz) return GTS_ERR_SHAPE;
  const int64_t voxels = cx * cy * cz;
  const int64_t groups = x != nullptr ? (channels + 3) / 4 : 1;
  if (voxels > (lim * kBlock) / groups) return GTS_ERR_SHAPE;
  const unsigned blocks = static_cast<unsigned>((voxels * groups + kBlock - 1) / kBlock);
  const bool vec = x != nullptr && channels % 4 == 0 && aligned16(x) && aligned16(x_out);
  const PhiloxKey key = philox_key(seed, step);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool narrow = voxels * groups < (1LL << 32);
  const int c = static_cast<int>(channels), ci = static_cast<int>(image_channels), gr = static_cast<int>(groups);
#define GTS_AUGMENT_CROP(VEC, IDX) \
  augment_crop_kernel<VEC, IDX><<<blocks, kBlock, 0, st>>>(x, labels, params, x_out, labels_out, cx, cy, cz, c, ci, gr, \
                                                           flip_mask, key)
  if (vec && narrow) GTS_AUGMENT_CROP(true, uint32_t);
  else if (vec) GTS_AUGMENT_CROP(true, int64_t);
  else if (narrow) GTS_AUGMENT_CROP(false, uint32_t);
  else GTS_AUGMENT_CROP(false, int64_t);
#undef GTS_AUGMENT_CROP
  return launch_status();
}

extern "C" int32_t gts_augment_features_f32(const float* feats, const int64_t* row_ptr, const int64_t* row_ptr_host,
                                            const float* params, float* out, int64_t n_rows, int64_t n_feats,
                                            int64_t modalities, int64_t n_graphs, double sigma, uint64_t seed,
                                            uint64_t step, void* stream) {
  using namespace gts;
  if (!row_ptr || !row_ptr_host || !params) return GTS_ERR_NULL;
  if (n_rows < 0 || n_feats < 1 || n_feats > kMaxAugChannels || modalities < 1 || n_graphs < 1 ||
      n_graphs >= (1LL << 31))
    return GTS_ERR_SHAPE;
  if (n_feats % modalities != 0) return GTS_ERR_SHAPE;
  if (!(sigma >= 0.0) || !isfinite(sigma)) return GTS_ERR_ARGKIND;
  if (row_ptr_host[0] != 0 || row_ptr_host[n_graphs] != n_rows) return GTS_ERR_SHAPE;
  for (int64_t b = 0; b < n_graphs; ++b)
    if (row_ptr_host[b + 1] < row_ptr_host[b]) return GTS_ERR_SHAPE;
  if (n_rows == 0) return GTS_OK;
  if (!feats || !out) return GTS_ERR_NULL;
  const int64_t groups = (n_feats + 3) / 4;
  const int64_t lim = (1LL << 31) - 1;
  if (n_rows >= (1LL << 56) || n_rows > (lim * kBlock) / groups) return GTS_ERR_SHAPE;
  const unsigned blocks = static_cast<unsigned>((n_rows * groups + kBlock - 1) / kBlock);
  const bool vec = n_feats % 4 == 0 && aligned16(feats) && aligned16(out);
  const PhiloxKey key = philox_key(seed, step);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    augment_features_kernel<true><<<blocks, kBlock, 0, st>>>(feats, row_ptr, params, out, n_rows,
                                                             static_cast<int>(n_feats), static_cast<int>(modalities),
                                                             static_cast<int>(n_graphs), static_cast<int>(groups),
                                                             static_cast<float>(sigma), key);
  else
    augment_features_kernel<false><<<blocks, kBlock, 0, st>>>(feats, row_ptr, params, out, n_rows,
                                                              static_cast<int>(n_feats), static_cast<int>(modalities),
                                                              static_cast<int>(n_graphs), static_cast<int>(groups),
                                                              static_cast<float>(sigma), key);
  return launch_status();
}

extern "C" int32_t gts_augment_spatial_f32(const float* x, const int64_t* labels, const float* params,
                                           const double* matrix, float* x_out, int64_t* labels_out, int64_t cx,
                                           int64_t cy, int64_t cz, int64_t channels, int64_t image_channels,
                                           int32_t flip_mask, uint64_t seed, uint64_t step, void* stream) {
  using namespace gts;
  if (x == nullptr && labels == nullptr) return GTS_ERR_NULL;
  if ((x != nullptr && x_out == nullptr) || (labels != nullptr && labels_out == nullptr)) return GTS_ERR_NULL;
  if (matrix == nullptr) return GTS_ERR_NULL;
  if (cx < 0 || cy < 0 || cz < 0 || channels < 0 || image_channels < 0) return GTS_ERR_SHAPE;
  if (flip_mask < 0 || flip_mask > 7) return GTS_ERR_ARGKIND;
  if (x != nullptr && (channels < 1 || channels > kMaxAugChannels || image_channels > channels)) return GTS_ERR_SHAPE;
  if (x != nullptr && image_channels > 0 && params == nullptr) return GTS_ERR_NULL;
  if (x == nullptr && image_channels != 0) return GTS_ERR_SHAPE;
  const int64_t lim = (1LL << 31) - 1;
  if (cx > lim || cy > lim || cz > lim) return GTS_ERR_SHAPE;
  SpatialMap map;
  SpatialInverse back;
  if (const int bad = spatial_setup(matrix, cx, cy, cz, &map, &back)) return bad;
  if (cx == 0 || cy == 0 || cz == 0) return GTS_OK;
  if (cx > (1LL << 56) / cy / cz) return GTS_ERR_SHAPE;
  const int64_t voxels = cx * cy * cz;
  const int64_t groups = x != nullptr ? (channels + 3) / 4 : 1;
  if (voxels > (lim * kBlock) / groups) return GTS_ERR_SHAPE;
  const unsigned blocks = static_cast<unsigned>((voxels * groups + kBlock - 1) / kBlock);
  const bool vec = x != nullptr && channels % 4 == 0 && aligned16(x) && aligned16(x_out);
  const PhiloxKey key = philox_key(seed, step);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool narrow = voxels * groups < (1LL << 32);
  const int c = static_cast<int>(channels), ci = static_cast<int>(image_channels), gr = static_cast<int>(groups);
#define GTS_AUGMENT_SPATIAL(VEC, IDX) \
  augment_spatial_kernel<VEC, IDX><<<blocks, kBlock, 0, st>>>(x, labels, params, x_out, labels_out, cx, cy, cz, c, ci, \
                                                              gr, flip_mask, key, map)
  if (vec && narrow) GTS_AUGMENT_SPATIAL(true, uint32_t);
  else if (vec) GTS_AUGMENT_SPATIAL(true, int64_t);
  else if (narrow) GTS_AUGMENT_SPATIAL(false, uint32_t);
  else GTS_AUGMENT_SPATIAL(false, int64_t);
#undef GTS_AUGMENT_SPATIAL
  return launch_status();
}

extern "C" int32_t gts_augment_spatial_bwd_f32(const float* dy, const double* matrix, float* dx, int64_t cx, int64_t cy,
                                               int64_t cz, int64_t channels, int32_t flip_mask, void* stream) {
  using namespace gts;
  if (dy == nullptr || matrix == nullptr || dx == nullptr) return GTS_ERR_NULL;
  if (cx < 0 || cy < 0 || cz < 0 || channels < 1 || channels > kMaxAugChannels) return GTS_ERR_SHAPE;
  if (flip_mask < 0 || flip_mask > 7) return GTS_ERR_ARGKIND;
  const int64_t lim = (1LL << 31) - 1;
  if (cx > lim || cy > lim || cz > lim) return GTS_ERR_SHAPE;
  SpatialMap map;
  SpatialInverse back;
  if (const int bad = spatial_setup(matrix, cx, cy, cz, &map, &back)) return bad;
  if (cx == 0 || cy == 0 || cz == 0) return GTS_OK;
  if (cx > (1LL << 56) / cy / cz) return GTS_ERR_SHAPE;
  const int64_t voxels = cx * cy * cz;
  const int64_t groups = (channels + 3) / 4;
  if (voxels > (lim * kBlock) / groups) return GTS_ERR_SHAPE;
  const unsigned blocks = static_cast<unsigned>((voxels * groups + kBlock - 1) / kBlock);
  const bool vec = channels % 4 == 0 && aligned16(dy) && aligned16(dx);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool narrow = voxels * groups < (1LL << 32);
  const int c = static_cast<int>(channels), gr = static_cast<int>(groups);
#define GTS_AUGMENT_SPATIAL_BWD(VEC, IDX) \
  augment_spatial_bwd_kernel<VEC, IDX><<<blocks, kBlock, 0, st>>>(dy, dx, cx, cy, cz, c, gr, flip_mask, map, back)
  if (vec && narrow) GTS_AUGMENT_SPATIAL_BWD(true, uint32_t);
  else if (vec) GTS_AUGMENT_SPATIAL_BWD(true, int64_t);
  else if (narrow) GTS_AUGMENT_SPATIAL_BWD(false, uint32_t);
  else GTS_AUGMENT_SPATIAL_BWD(false, int64_t);
#undef GTS_AUGMENT_SPATIAL_BWD
  return launch_status();
}
