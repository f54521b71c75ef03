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

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline PhiloxKey philox_key(uint64_t seed, uint64_t step) {
  return PhiloxKey{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(step),
                   static_cast<uint32_t>(step >> 32)};
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
