// G1-G8: supervoxel graph construction from an MRI volume (reference mri2graph/graphgen.py,
// skimage <= 0.18 SLIC restated in DESIGN.md "Graph generation").
//
// Determinism: every floating-point sum whose order matters is formed by ONE lane in a fixed
// order (Gaussian taps, distances, SLIC colour sums in raster order, quantile interpolation).
// Atomics appear only on integers (counts, coordinate sums, bounding boxes, bitmaps) and as
// atomicMin on the bit pattern of a non-negative double, all of which are order-independent.
// The library is compiled with -ffp-contract=off: no FMA contraction changes a rounding.
#include <math.h>
#include <string.h>

#include "gts_common.h"

namespace gts {
namespace {

constexpr int kGgBlock = 256;
constexpr int kStatsCap = 4096;   // segments up to this many voxels are sorted in LDS (16 KiB)
constexpr int kSlicMaxC = 8;      // channels the SLIC update kernel stages per voxel
constexpr int kScanBlock = 1024;

inline unsigned grid_for(int64_t n, int block) {
  const int64_t g = (n + block - 1) / block;
  return static_cast<unsigned>(g < 1 ? 1 : g);
}

// scipy.ndimage 'reflect' (d c b a | a b c d | d c b a), any line length
__device__ __forceinline__ int64_t reflect_index(int64_t i, int64_t n) {
  const int64_t period = 2 * n;
  i %= period;
  if (i < 0) i += period;
  return i >= n ? period - 1 - i : i;
}

// ---- G1: one separable Gaussian pass along one spatial axis --------------------------------
// scipy ni_filters.c NI_Correlate1D, symmetric branch: centre tap first, then the pairs
// (v[i-j] + v[i+j]) * w[j] for j = radius .. 1, accumulated in fp64.
__global__ void gaussian_pass_kernel(const double* __restrict__ in, double* __restrict__ out,
                                     const double* __restrict__ w, int radius, double scale,
                                     int64_t total, int64_t stride, int64_t len) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t p = (idx / stride) % len;
  const int64_t base = idx - p * stride;
  double acc = in[idx] * w[0];
  for (int j = radius; j >= 1; --j) {
    const double a = in[base + reflect_index(p - j, len) * stride];
    const double b = in[base + reflect_index(p + j, len) * stride];
    acc += (a + b) * w[j];
  }
  out[idx] = acc * scale;
}

// ---- G2: SLIC assignment ---------------------------------------------------------------------
struct SlicGeom {
  int D, H, W, C;
  int sz, sy, sx;
  double spatial_weight;
};

// skimage _slic.pyx: window [trunc(max(c - 2s, 0)), trunc(min(c + 2s + 1, dim)))
__device__ __forceinline__ void slic_window(double c, int s, int dim, int& lo, int& hi) {
  double a = c - static_cast<double>(2 * s);
  lo = static_cast<int>(a > 0.0 ? a : 0.0);
  double b = c + static_cast<double>(2 * s);
  b = b + 1.0;
  hi = static_cast<int>(b < static_cast<double>(dim) ? b : static_cast<double>(dim));
}

// dist = ((cz-z)^2 + (cy-y)^2 + (cx-x)^2) * spatial_weight + sum_c (I - colour_c)^2, c ascending
__device__ __forceinline__ double slic_distance(const double* __restrict__ img, const double* ce,
                                                const SlicGeom& g, int z, int y, int x, int64_t v) {
  const double dz = ce[0] - z, dy = ce[1] - y, dx = ce[2] - x;
  double d = dz * dz + dy * dy;
  d = d + dx * dx;
  d = d * g.spatial_weight;
  double col = 0.0;
  const double* px = img + v * g.C;
#pragma unroll
  for (int c = 0; c < kSlicMaxC; ++c) {
    if (c < g.C) {
      const double t = px[c] - ce[3 + c];
      col += t * t;
    }
  }
  return d + col;
}

// pass A (want_min = 1): best[v] = min over windows of the distance's bit pattern (a
// non-negative double orders like its bits).  Pass B (want_min = 0): among the centres that
// reach best[v], winner[v] = the lowest index — skimage's strict '<' over ascending k.
__global__ void slic_window_kernel(const double* __restrict__ img, const double* __restrict__ centres,
                                   SlicGeom g, unsigned long long* __restrict__ best,
                                   unsigned* __restrict__ winner, int want_min) {
  const int k = blockIdx.x;
  const int nf = 3 + g.C;
  double ce[3 + kSlicMaxC];
#pragma unroll
  for (int i = 0; i < 3 + kSlicMaxC; ++i) ce[i] = i < nf ? centres[static_cast<int64_t>(k) * nf + i] : 0.0;
  if (!(ce[0] == ce[0])) return;  // emptied segment: 0/0 centre, never captures again
  int z0, z1, y0, y1, x0, x1;
  slic_window(ce[0], g.sz, g.D, z0, z1);
  slic_window(ce[1], g.sy, g.H, y0, y1);
  slic_window(ce[2], g.sx, g.W, x0, x1);
  const int nz = z1 - z0, ny = y1 - y0, nx = x1 - x0;
  if (nz <= 0 || ny <= 0 || nx <= 0) return;
  const int64_t n = static_cast<int64_t>(nz) * ny * nx;
  for (int64_t t = threadIdx.x; t < n; t += blockDim.x) {
    const int x = x0 + static_cast<int>(t % nx);
    const int y = y0 + static_cast<int>((t / nx) % ny);
    const int z = z0 + static_cast<int>(t / (static_cast<int64_t>(nx) * ny));
    const int64_t v = (static_cast<int64_t>(z) * g.H + y) * g.W + x;
    const double d = slic_distance(img, ce, g, z, y, x, v);
    const unsigned long long key = static_cast<unsigned long long>(__double_as_longlong(d));
    if (want_min) {
      atomicMin(best + v, key);
    } else if (key == best[v]) {
      atomicMin(winner + v, static_cast<unsigned>(k));
    }
  }
}

// a voxel inside no window keeps its previous label
__global__ void slic_finalize_kernel(const unsigned* __restrict__ winner, int32_t* __restrict__ labels,
                                     int64_t n_vox) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const unsigned w = winner[v];
  if (w != 0xFFFFFFFFu) labels[v] = static_cast<int32_t>(w);
}

// ---- G3: SLIC centre update ------------------------------------------------------------------
__global__ void bbox_init_kernel(int32_t* bbox, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t* b = bbox + 6 * static_cast<int64_t>(i);
  b[0] = b[2] = b[4] = INT32_MAX;
  b[1] = b[3] = b[5] = -1;
}

__global__ void bbox_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ bbox, SlicGeom g,
                            int n_centres) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t n_vox = static_cast<int64_t>(g.D) * g.H * g.W;
  if (v >= n_vox) return;
  const int k = labels[v];
  if (k < 0 || k >= n_centres) return;
  const int x = static_cast<int>(v % g.W), y = static_cast<int>((v / g.W) % g.H),
            z = static_cast<int>(v / (static_cast<int64_t>(g.W) * g.H));
  int32_t* b = bbox + 6 * static_cast<int64_t>(k);
  atomicMin(b + 0, z); atomicMax(b + 1, z);
  atomicMin(b + 2, y); atomicMax(b + 3, y);
  atomicMin(b + 4, x); atomicMax(b + 5, x);
}

// One wave per segment walks the segment's bounding box in raster order.  Matching lanes stage
// their colours in LDS at their rank inside the 64-voxel run; lane 0 adds them in that order,
// so the colour sums are the raster-order sums of skimage's update loop.  Counts and coordinate
// sums are integers (exact in any order).
__global__ void __launch_bounds__(kWave) slic_update_kernel(const double* __restrict__ img,
                                                             const int32_t* __restrict__ labels,
                                                             const int32_t* __restrict__ bbox,
                                                             double* __restrict__ centres, SlicGeom g) {
  __shared__ double stage[kWave * kSlicMaxC];
  const int k = blockIdx.x;
  const int lane = threadIdx.x;
  const int nf = 3 + g.C;
  const int32_t* b = bbox + 6 * static_cast<int64_t>(k);
  const int z0 = b[0], z1 = b[1], y0 = b[2], y1 = b[3], x0 = b[4], x1 = b[5];
  long long cnt = 0, sz = 0, sy = 0, sx = 0;
  double col[kSlicMaxC];
  for (int c = 0; c < kSlicMaxC; ++c) col[c] = 0.0;
  for (int z = z0; z <= z1; ++z) {
    for (int y = y0; y <= y1; ++y) {
      const int64_t row = (static_cast<int64_t>(z) * g.H + y) * g.W;
      for (int xb = x0; xb <= x1; xb += kWave) {
        const int x = xb + lane;
        const bool hit = x <= x1 && labels[row + x] == k;
        const unsigned long long mask = __ballot(hit);
        if (hit) {
          cnt += 1; sz += z; sy += y; sx += x;
          const int rank = __popcll(mask & ((1ull << lane) - 1ull));
          const double* px = img + (row + x) * g.C;
#pragma unroll
          for (int c = 0; c < kSlicMaxC; ++c)
            if (c < g.C) stage[rank * kSlicMaxC + c] = px[c];
        }
        __syncthreads();
        if (lane == 0) {
          const int m = __popcll(mask);
          for (int r = 0; r < m; ++r)
#pragma unroll
            for (int c = 0; c < kSlicMaxC; ++c)
              if (c < g.C) col[c] += stage[r * kSlicMaxC + c];
        }
        __syncthreads();
      }
    }
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off);
    sz += __shfl_down(sz, off);
    sy += __shfl_down(sy, off);
    sx += __shfl_down(sx, off);
  }
  if (lane == 0) {
    double* ce = centres + static_cast<int64_t>(k) * nf;
    const double n = static_cast<double>(cnt);  // 0 -> 0/0: the segment is dead from now on
    ce[0] = static_cast<double>(sz) / n;
    ce[1] = static_cast<double>(sy) / n;
    ce[2] = static_cast<double>(sx) / n;
#pragma unroll
    for (int c = 0; c < kSlicMaxC; ++c)
      if (c < g.C) ce[3 + c] = col[c] / n;
  }
}

// ---- shared: exclusive scan of <= 32767 int32 in one workgroup -------------------------------
__device__ void block_exclusive_scan(const int32_t* in, int32_t* out, int n, int32_t* total) {
  __shared__ int32_t part[kScanBlock];
  const int t = threadIdx.x;
  const int per = (n + kScanBlock - 1) / kScanBlock;
  const int lo = min(n, t * per), hi = min(n, lo + per);
  int32_t s = 0;
  for (int i = lo; i < hi; ++i) s += in[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < kScanBlock; off <<= 1) {
    const int32_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int32_t run = part[t] - s;
  for (int i = lo; i < hi; ++i) {
    const int32_t x = in[i];
    out[i] = run;
    run += x;
  }
  if (t == kScanBlock - 1 && total) *total = part[t];
  __syncthreads();
}

// ---- G5: supervoxel statistics ---------------------------------------------------------------
__global__ void count_labels_kernel(const int32_t* __restrict__ part, int64_t n_vox, int n_sv,
                                    int32_t* __restrict__ counts) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const int k = part[v];
  if (k >= 0 && k < n_sv) atomicAdd(counts + k, 1);
}

__global__ void __launch_bounds__(kScanBlock) scan_kernel(const int32_t* in, int32_t* out, int n,
                                                          int32_t* total) {
  block_exclusive_scan(in, out, n, total);
}

// voxel ids bucketed by label (order inside a bucket is arbitrary: only multisets are used)
__global__ void bucket_kernel(const int32_t* __restrict__ part, int64_t n_vox, int n_sv,
                              const int32_t* __restrict__ offs, int32_t* __restrict__ cursor,
                              int32_t* __restrict__ bucket) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const int k = part[v];
  if (k < 0 || k >= n_sv) return;
  bucket[offs[k] + atomicAdd(cursor + k, 1)] = static_cast<int32_t>(v);
}

// Ascending bitonic sort of a[0..n) for any n: the first step of every merge compares i with its
// mirror i ^ (k - 1), the later ones i with i ^ j, so every comparator puts the minimum at the
// lower index and the virtual +inf tail past n never moves — comparators that reach it are skipped.
__device__ void block_sort(float* a, int n) {
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int k = 2; k <= p2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < p2; i += blockDim.x) {
        const int l = (j == (k >> 1)) ? (i ^ (k - 1)) : (i ^ j);
        if (l > i && l < n) {
          const float x = a[i], y = a[l];
          if (y < x) {
            a[i] = y;
            a[l] = x;
          }
        }
      }
      __threadfence_block();
      __syncthreads();
    }
  }
}

// numpy 2.2 _quantile(method='linear') + _lerp on float32 data: b - a is a float32 subtraction,
// the interpolation is fp64; t >= 0.5 interpolates from the upper neighbour.
__device__ double quantile_linear(const float* a, int n, double q) {
  const double vi = static_cast<double>(n - 1) * q;
  if (vi >= static_cast<double>(n - 1)) return static_cast<double>(a[n - 1]);
  const double prev = floor(vi);
  const int p = static_cast<int>(prev);
  const double t = vi - prev;
  const float lo = a[p], hi = a[p + 1];
  const float diff = hi - lo;
  if (t >= 0.5) return static_cast<double>(hi) - static_cast<double>(diff) * (1.0 - t);
  return static_cast<double>(lo) + static_cast<double>(diff) * t;
}

__global__ void __launch_bounds__(kGgBlock) sv_stats_kernel(
    const float* __restrict__ img, const int16_t* __restrict__ vox_labels, const int32_t* __restrict__ bucket,
    const int32_t* __restrict__ offs, const int32_t* __restrict__ counts, float* __restrict__ spill, int H, int W,
    int C, double* __restrict__ feats, double* __restrict__ centroids, int32_t* __restrict__ sv_labels) {
  __shared__ float lds[kStatsCap];
  __shared__ unsigned long long csum[3];
  const int k = blockIdx.x;
  const int n = counts[k];
  const int off = offs[k];
  double* f = feats + static_cast<int64_t>(k) * 5 * C;
  if (n == 0) {  // scipy labeled_comprehension's default; never reached for SLIC output
    if (threadIdx.x < 5 * C) f[threadIdx.x] = -1.0;
    if (threadIdx.x < 3) centroids[3 * static_cast<int64_t>(k) + threadIdx.x] = NAN;
    if (threadIdx.x == 0) sv_labels[k] = -1;
    return;
  }
  float* buf = n <= kStatsCap ? lds : spill + off;
  if (threadIdx.x < 3) csum[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long s0 = 0, s1 = 0, s2 = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int64_t v = bucket[off + i];
    s2 += static_cast<unsigned long long>(v % W);
    s1 += static_cast<unsigned long long>((v / W) % H);
    s0 += static_cast<unsigned long long>(v / (static_cast<int64_t>(W) * H));
  }
  atomicAdd(&csum[0], s0);
  atomicAdd(&csum[1], s1);
  atomicAdd(&csum[2], s2);
  const double q[5] = {0.1, 0.25, 0.5, 0.75, 0.9};
  for (int c = 0; c <= C; ++c) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int64_t v = bucket[off + i];
      buf[i] = c < C ? img[v * C + c] : (vox_labels ? static_cast<float>(vox_labels[v]) : 0.0f);
    }
    __threadfence_block();
    __syncthreads();
    block_sort(buf, n);
    if (threadIdx.x == 0) {
      if (c < C) {
        for (int j = 0; j < 5; ++j) f[c * 5 + j] = quantile_linear(buf, n, q[j]);
      } else {  // mode: the longest run of the sorted labels, the smallest value among ties
        float best = buf[0];
        int best_n = 0, run = 0;
        for (int i = 0; i < n; ++i) {
          run = (i > 0 && buf[i] == buf[i - 1]) ? run + 1 : 1;
          if (run > best_n) {
            best_n = run;
            best = buf[i];
          }
        }
        sv_labels[k] = static_cast<int32_t>(best);
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  if (threadIdx.x < 3)
    centroids[3 * static_cast<int64_t>(k) + threadIdx.x] =
        static_cast<double>(csum[threadIdx.x]) / static_cast<double>(n);
}

// ---- G6: discard empty supervoxels + renumber ------------------------------------------------
__global__ void __launch_bounds__(kScanBlock) discard_scan_kernel(const double* __restrict__ feats, int n_sv,
                                                                  int n_feat, int32_t* __restrict__ keep,
                                                                  int32_t* __restrict__ remap,
                                                                  int32_t* __restrict__ n_nodes) {
  __shared__ double red[kScanBlock];
  double m = INFINITY;
  for (int i = threadIdx.x; i < n_sv; i += blockDim.x) m = fmin(m, feats[static_cast<int64_t>(i) * n_feat + 4]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int off = kScanBlock / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  const double thr = red[0] + 0.01;
  for (int i = threadIdx.x; i < n_sv; i += blockDim.x)
    keep[i] = (feats[static_cast<int64_t>(i) * n_feat + 4] < thr) ? 0 : 1;
  __syncthreads();
  block_exclusive_scan(keep, remap, n_sv, n_nodes);
  for (int i = threadIdx.x; i < n_sv; i += blockDim.x)
    if (!keep[i]) remap[i] = -1;
}

__global__ void discard_gather_kernel(const double* __restrict__ feats, const double* __restrict__ centroids,
                                      const int32_t* __restrict__ sv_labels, const int32_t* __restrict__ remap,
                                      int n_sv, int n_feat, double* __restrict__ node_feats,
                                      double* __restrict__ node_centroids, int32_t* __restrict__ node_labels) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sv) return;
  const int r = remap[i];
  if (r < 0) return;
  for (int j = 0; j < n_feat; ++j)
    node_feats[static_cast<int64_t>(r) * n_feat + j] = feats[static_cast<int64_t>(i) * n_feat + j];
  for (int j = 0; j < 3; ++j) node_centroids[3 * static_cast<int64_t>(r) + j] = centroids[3 * static_cast<int64_t>(i) + j];
  node_labels[r] = sv_labels[i];
}

__global__ void remap_partition_kernel(const int32_t* __restrict__ part, const int32_t* __restrict__ remap,
                                       int64_t n_vox, int n_sv, int16_t* __restrict__ out) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const int k = part[v];
  out[v] = static_cast<int16_t>((k >= 0 && k < n_sv) ? remap[k] : -1);
}

// ---- G7: k nearest j > i per row ---------------------------------------------------------------
// One lane per row walks j = i+1 .. n-1 in order and keeps the k best (distance, j) in registers;
// strict '<' keeps the lower j first among equal distances.  Distance = scipy cdist's
// sqrt((d0^2 + d1^2) + d2^2) with the correctly rounded fp64 square root.
// KM: compile-time slot count >= k (8, 16 or 32), so the kept lists stay in registers at the sizes used.
template <int KM>
__global__ void knn_candidates_kernel(const double* __restrict__ pos, int n, int k, int32_t* __restrict__ cand) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double bd[KM];
  int bj[KM];
#pragma unroll
  for (int t = 0; t < KM; ++t) {
    bd[t] = INFINITY;
    bj[t] = -1;
  }
  const double zi = pos[3 * static_cast<int64_t>(i)], yi = pos[3 * static_cast<int64_t>(i) + 1],
               xi = pos[3 * static_cast<int64_t>(i) + 2];
  for (int j = i + 1; j < n; ++j) {
    const double dz = zi - pos[3 * static_cast<int64_t>(j)];
    const double dy = yi - pos[3 * static_cast<int64_t>(j) + 1];
    const double dx = xi - pos[3 * static_cast<int64_t>(j) + 2];
    double d2 = dz * dz + dy * dy;
    d2 = d2 + dx * dx;
    const double d = sqrt(d2);
    double worst = INFINITY;  // distance in slot k-1 (+inf while fewer than k are kept)
#pragma unroll
    for (int t = 0; t < KM; ++t)
      if (t == k - 1) worst = bd[t];
    if (!(d < worst)) continue;
    // insertion inside slots [0, k): entries with a larger distance move one slot down
    bool placed = false;
#pragma unroll
    for (int t = KM - 1; t >= 0; --t) {
      if (t < k && !placed) {
        if (t > 0 && bd[t - 1] > d) {
          bd[t] = bd[t - 1];
          bj[t] = bj[t - 1];
        } else {
          bd[t] = d;
          bj[t] = j;
          placed = true;
        }
      }
    }
  }
  for (int t = 0; t < k; ++t) {
    int val = -1;
#pragma unroll
    for (int u = 0; u < KM; ++u)
      if (u == t) val = bj[u];
    cand[static_cast<int64_t>(i) * k + t] = val;
  }
}

// ---- G8: face-adjacent supervoxels as a bitmap --------------------------------------------------
__device__ __forceinline__ void set_bit(uint32_t* bm, int words, int a, int b) {
  atomicOr(bm + static_cast<int64_t>(a) * words + (b >> 5), 1u << (b & 31));
}

__global__ void touching_mark_kernel(const int16_t* __restrict__ part, int D, int H, int W, int n,
                                     uint32_t* __restrict__ bm, int words) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t n_vox = static_cast<int64_t>(D) * H * W;
  if (v < n) set_bit(bm, words, static_cast<int>(v), static_cast<int>(v));  // self-loops
  if (v >= n_vox) return;
  const int a = part[v];
  if (a < 0 || a >= n) return;
  const int x = static_cast<int>(v % W), y = static_cast<int>((v / W) % H),
            z = static_cast<int>(v / (static_cast<int64_t>(W) * H));
  const int64_t nb[3] = {z + 1 < D ? v + static_cast<int64_t>(W) * H : -1, y + 1 < H ? v + W : -1,
                         x + 1 < W ? v + 1 : -1};
  for (int d = 0; d < 3; ++d) {
    if (nb[d] < 0) continue;
    const int b = part[nb[d]];
    if (b == a || b < 0 || b >= n) continue;
    set_bit(bm, words, a, b);
    set_bit(bm, words, b, a);
  }
}

__global__ void touching_count_kernel(const uint32_t* __restrict__ bm, int n, int words, int32_t* __restrict__ deg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int s = 0;
  for (int w = 0; w < words; ++w) s += __popc(bm[static_cast<int64_t>(i) * words + w]);
  deg[i] = s;
}

__global__ void touching_emit_kernel(const uint32_t* __restrict__ bm, int n, int words,
                                     const int32_t* __restrict__ indptr, int32_t* __restrict__ cols) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t o = indptr[i];
  for (int w = 0; w < words; ++w) {
    uint32_t m = bm[static_cast<int64_t>(i) * words + w];
    while (m) {
      const int b = __ffs(m) - 1;
      cols[o++] = w * 32 + b;
      m &= m - 1;
    }
  }
}

bool vox_ok(int64_t d, int64_t h, int64_t w, int64_t c) {
  if (d <= 0 || h <= 0 || w <= 0 || c <= 0) return false;
  if (d > INT32_MAX || h > INT32_MAX || w > INT32_MAX) return false;
  const double v = static_cast<double>(d) * h * w * c;
  return v < 2147483647.0;
}

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace
}  // namespace gts

using namespace gts;

extern "C" int32_t gts_gg_gaussian_f64(const double* in, double* out, double* tmp, const double* weights,
                                       int32_t radius, double scale, int64_t d, int64_t h, int64_t w, int64_t c,
                                       void* stream) {
  if (!in || !out || !tmp || !weights) return GTS_ERR_NULL;
  if (!vox_ok(d, h, w, c) || radius < 0 || radius > GTS_GG_MAX_RADIUS) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t total = d * h * w * c;
  const unsigned grid = grid_for(total, kGgBlock);
  // axis 0: in -> out, axis 1: out -> tmp, axis 2: tmp -> out (scaled)
  gaussian_pass_kernel<<<grid, kGgBlock, 0, st>>>(in, out, weights, radius, 1.0, total, h * w * c, d);
  gaussian_pass_kernel<<<grid, kGgBlock, 0, st>>>(out, tmp, weights, radius, 1.0, total, w * c, h);
  gaussian_pass_kernel<<<grid, kGgBlock, 0, st>>>(tmp, out, weights, radius, scale, total, c, w);
  return launch_status();
}

static SlicGeom make_geom(int64_t d, int64_t h, int64_t w, int64_t c, int32_t sz, int32_t sy, int32_t sx,
                          double spatial_weight) {
  SlicGeom g;
  g.D = static_cast<int>(d); g.H = static_cast<int>(h); g.W = static_cast<int>(w); g.C = static_cast<int>(c);
  g.sz = sz; g.sy = sy; g.sx = sx;
  g.spatial_weight = spatial_weight;
  return g;
}

extern "C" int32_t gts_gg_slic_assign_f64(const double* img, const double* centres, int32_t n_centres, int64_t d,
                                          int64_t h, int64_t w, int64_t c, int32_t step_z, int32_t step_y,
                                          int32_t step_x, double spatial_weight, int32_t* labels,
                                          uint64_t* best, uint32_t* winner, void* stream) {
  if (!img || !centres || !labels || !best || !winner) return GTS_ERR_NULL;
  if (!vox_ok(d, h, w, c) || c > kSlicMaxC || n_centres <= 0 || step_z < 1 || step_y < 1 || step_x < 1)
    return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_vox = d * h * w;
  const SlicGeom g = make_geom(d, h, w, c, step_z, step_y, step_x, spatial_weight);
  if (const hipError_t e = hipMemsetAsync(best, 0xFF, n_vox * sizeof(uint64_t), st)) return static_cast<int32_t>(e);
  if (const hipError_t e = hipMemsetAsync(winner, 0xFF, n_vox * sizeof(uint32_t), st)) return static_cast<int32_t>(e);
  auto* b = reinterpret_cast<unsigned long long*>(best);
  slic_window_kernel<<<n_centres, kGgBlock, 0, st>>>(img, centres, g, b, winner, 1);
  slic_window_kernel<<<n_centres, kGgBlock, 0, st>>>(img, centres, g, b, winner, 0);
  slic_finalize_kernel<<<grid_for(n_vox, kGgBlock), kGgBlock, 0, st>>>(winner, labels, n_vox);
  return launch_status();
}

extern "C" int32_t gts_gg_slic_update_f64(const double* img, const int32_t* labels, double* centres,
                                          int32_t n_centres, int64_t d, int64_t h, int64_t w, int64_t c,
                                          int32_t* bbox, void* stream) {
  if (!img || !labels || !centres || !bbox) return GTS_ERR_NULL;
  if (!vox_ok(d, h, w, c) || c > kSlicMaxC || n_centres <= 0) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_vox = d * h * w;
  const SlicGeom g = make_geom(d, h, w, c, 1, 1, 1, 0.0);
  bbox_init_kernel<<<grid_for(n_centres, kGgBlock), kGgBlock, 0, st>>>(bbox, n_centres);
  bbox_kernel<<<grid_for(n_vox, kGgBlock), kGgBlock, 0, st>>>(labels, bbox, g, n_centres);
  slic_update_kernel<<<n_centres, kWave, 0, st>>>(img, labels, bbox, centres, g);
  return launch_status();
}

extern "C" int32_t gts_gg_enforce_connectivity(const int32_t* labels, int32_t* out, int64_t d, int64_t h, int64_t w,
                                               int64_t min_size, int64_t max_size, int64_t* queue,
                                               int32_t* n_labels) {
  if (!labels || !out || !queue || !n_labels) return GTS_ERR_NULL;
  if (!vox_ok(d, h, w, 1) || max_size < 1 || min_size < 0) return GTS_ERR_SHAPE;
  const int64_t n_vox = d * h * w, hw = h * w;
  static const int ddx[6] = {1, -1, 0, 0, 0, 0}, ddy[6] = {0, 0, 1, -1, 0, 0}, ddz[6] = {0, 0, 0, 0, 1, -1};
  for (int64_t v = 0; v < n_vox; ++v) out[v] = -1;
  int32_t current = 0, max_label = -1;
  for (int64_t v = 0; v < n_vox; ++v) {
    if (out[v] >= 0) continue;
    int32_t adjacent = 0;
    const int32_t label = labels[v];
    out[v] = current;
    int64_t size = 1, visited = 0;
    queue[0] = v;
    while (visited < size && size < max_size) {
      const int64_t q = queue[visited];
      const int64_t qz = q / hw, qy = (q / w) % h, qx = q % w;
      for (int i = 0; i < 6; ++i) {
        const int64_t zz = qz + ddz[i], yy = qy + ddy[i], xx = qx + ddx[i];
        if (xx < 0 || xx >= w || yy < 0 || yy >= h || zz < 0 || zz >= d) continue;
        const int64_t u = zz * hw + yy * w + xx;
        if (labels[u] == label && out[u] == -1) {
          out[u] = current;
          queue[size++] = u;
          if (size >= max_size) break;
        } else if (out[u] >= 0 && out[u] != current) {
          adjacent = out[u];
        }
      }
      ++visited;
    }
    if (size < min_size) {
      for (int64_t i = 0; i < size; ++i) out[queue[i]] = adjacent;
    } else {
      ++current;
    }
  }
  for (int64_t v = 0; v < n_vox; ++v) max_label = out[v] > max_label ? out[v] : max_label;
  *n_labels = max_label + 1;
  return GTS_OK;
}

extern "C" int64_t gts_gg_sv_stats_workspace(int64_t n_vox, int32_t n_sv) {
  if (n_vox < 0 || n_sv < 0) return GTS_ERR_SHAPE;
  return align256(3 * static_cast<int64_t>(n_sv) * 4) + align256(n_vox * 4) + align256(n_vox * 4);
}

extern "C" int32_t gts_gg_sv_stats(const int32_t* partition, const float* intensities, const int16_t* vox_labels,
                                   int64_t d, int64_t h, int64_t w, int64_t c, int32_t n_sv, double* feats,
                                   double* centroids, int32_t* sv_labels, void* scratch, void* stream) {
  if (!partition || !intensities || !feats || !centroids || !sv_labels || !scratch) return GTS_ERR_NULL;
  if (!vox_ok(d, h, w, c) || n_sv <= 0 || n_sv > GTS_GG_MAX_SV || 5 * c > kGgBlock) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_vox = d * h * w;
  char* s = static_cast<char*>(scratch);
  int32_t* counts = reinterpret_cast<int32_t*>(s);
  int32_t* offs = counts + n_sv;
  int32_t* cursor = offs + n_sv;
  s += align256(3 * static_cast<int64_t>(n_sv) * 4);
  int32_t* bucket = reinterpret_cast<int32_t*>(s);
  s += align256(n_vox * 4);
  float* spill = reinterpret_cast<float*>(s);
  if (const hipError_t e = hipMemsetAsync(counts, 0, 3 * static_cast<size_t>(n_sv) * 4, st)) return static_cast<int32_t>(e);
  const unsigned gv = grid_for(n_vox, kGgBlock);
  count_labels_kernel<<<gv, kGgBlock, 0, st>>>(partition, n_vox, n_sv, counts);
  scan_kernel<<<1, kScanBlock, 0, st>>>(counts, offs, n_sv, nullptr);
  bucket_kernel<<<gv, kGgBlock, 0, st>>>(partition, n_vox, n_sv, offs, cursor, bucket);
  sv_stats_kernel<<<n_sv, kGgBlock, 0, st>>>(intensities, vox_labels, bucket, offs, counts, spill,
                                             static_cast<int>(h), static_cast<int>(w), static_cast<int>(c), feats,
                                             centroids, sv_labels);
  return launch_status();
}

extern "C" int32_t gts_gg_discard_f64(const double* feats, const double* centroids, const int32_t* sv_labels,
                                      int32_t n_sv, int32_t n_feat, const int32_t* partition, int64_t n_vox,
                                      int32_t* remap, int32_t* keep, double* node_feats, double* node_centroids,
                                      int32_t* node_labels, int16_t* new_partition, int32_t* n_nodes, void* stream) {
  if (!feats || !centroids || !sv_labels || !partition || !remap || !keep || !node_feats || !node_centroids ||
      !node_labels || !new_partition || !n_nodes)
    return GTS_ERR_NULL;
  if (n_sv <= 0 || n_sv > GTS_GG_MAX_SV || n_feat < 5 || n_vox <= 0 || n_vox > INT32_MAX) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  discard_scan_kernel<<<1, kScanBlock, 0, st>>>(feats, n_sv, n_feat, keep, remap, n_nodes);
  discard_gather_kernel<<<grid_for(n_sv, kGgBlock), kGgBlock, 0, st>>>(feats, centroids, sv_labels, remap, n_sv,
                                                                       n_feat, node_feats, node_centroids, node_labels);
  remap_partition_kernel<<<grid_for(n_vox, kGgBlock), kGgBlock, 0, st>>>(partition, remap, n_vox, n_sv, new_partition);
  return launch_status();
}

extern "C" int32_t gts_gg_knn_candidates_f64(const double* positions, int32_t n, int32_t k, int32_t* cand,
                                             void* stream) {
  if (!positions || !cand) return GTS_ERR_NULL;
  if (n <= 0 || n > GTS_GG_MAX_SV || k < 1 || k > GTS_GG_MAX_K) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (k <= 8)
    knn_candidates_kernel<8><<<grid_for(n, 64), 64, 0, st>>>(positions, n, k, cand);
  else if (k <= 16)
    knn_candidates_kernel<16><<<grid_for(n, 64), 64, 0, st>>>(positions, n, k, cand);
  else
    knn_candidates_kernel<GTS_GG_MAX_K><<<grid_for(n, 64), 64, 0, st>>>(positions, n, k, cand);
  return launch_status();
}

extern "C" int32_t gts_gg_knn_greedy(const int32_t* cand, int32_t n, int32_t k, int32_t* picks, int32_t* got,
                                     int64_t* n_edges) {
  if (!cand || !picks || !got || !n_edges) return GTS_ERR_NULL;
  if (n <= 0 || n > GTS_GG_MAX_SV || k < 1 || k > GTS_GG_MAX_K) return GTS_ERR_SHAPE;
  for (int64_t i = 0; i < static_cast<int64_t>(n) * k; ++i) {
    const int32_t j = cand[i];
    if (j < -1 || j >= n || (j >= 0 && j <= i / k)) return GTS_ERR_SHAPE;
  }
  // got[i] = rows i' < i that already picked i: sum(adjacency_matrix[i]) in the reference loop
  memset(got, 0, static_cast<size_t>(n) * sizeof(int32_t));
  int64_t e = 0;
  for (int32_t i = 0; i < n; ++i) {
    const int32_t need = k - got[i];
    for (int32_t t = 0; t < k; ++t) {
      const int32_t j = cand[static_cast<int64_t>(i) * k + t];
      const bool take = t < need && j >= 0;
      picks[static_cast<int64_t>(i) * k + t] = take ? j : -1;
      if (take) {
        ++got[j];
        ++e;
      }
    }
  }
  *n_edges = e;
  return GTS_OK;
}

extern "C" int64_t gts_gg_touching_workspace(int32_t n) {
  if (n <= 0 || n > GTS_GG_MAX_SV) return GTS_ERR_SHAPE;
  return align256(static_cast<int64_t>(n) * ((n + 31) / 32) * 4) + align256(static_cast<int64_t>(n) * 4);
}

extern "C" int32_t gts_gg_touching_count_i16(const int16_t* partition, int64_t d, int64_t h, int64_t w, int32_t n,
                                             void* scratch, int32_t* indptr, void* stream) {
  if (!partition || !scratch || !indptr) return GTS_ERR_NULL;
  if (!vox_ok(d, h, w, 1) || n <= 0 || n > GTS_GG_MAX_SV) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int words = (n + 31) / 32;
  const int64_t bm_bytes = static_cast<int64_t>(n) * words * 4;
  uint32_t* bm = static_cast<uint32_t*>(scratch);
  int32_t* deg = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + align256(bm_bytes));
  if (const hipError_t e = hipMemsetAsync(bm, 0, bm_bytes, st)) return static_cast<int32_t>(e);
  const int64_t n_vox = d * h * w;
  touching_mark_kernel<<<grid_for(n_vox > n ? n_vox : n, kGgBlock), kGgBlock, 0, st>>>(
      partition, static_cast<int>(d), static_cast<int>(h), static_cast<int>(w), n, bm, words);
  touching_count_kernel<<<grid_for(n, kGgBlock), kGgBlock, 0, st>>>(bm, n, words, deg);
  scan_kernel<<<1, kScanBlock, 0, st>>>(deg, indptr, n, indptr + n);
  return launch_status();
}

extern "C" int32_t gts_gg_touching_emit(const void* scratch, int32_t n, const int32_t* indptr, int32_t* cols,
                                        void* stream) {
  if (!scratch || !indptr || !cols) return GTS_ERR_NULL;
  if (n <= 0 || n > GTS_GG_MAX_SV) return GTS_ERR_SHAPE;
  touching_emit_kernel<<<grid_for(n, kGgBlock), kGgBlock, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint32_t*>(scratch), n, (n + 31) / 32, indptr, cols);
  return launch_status();
}
