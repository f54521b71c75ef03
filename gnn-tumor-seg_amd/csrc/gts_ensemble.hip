// E1/E2: the two voxel passes of ensemble prediction (gts/ensemble.py): several weight sets and
// mirrored views are averaged as class probabilities before the arg-max.
//
//   softmax_accumulate   (E1) acc[r, :] (+)= sum over sets s of softmax(set_s[r, :]), rows x classes fp32 row-major.
//                        Stable softmax (row maximum subtracted, denominator summed in class order); the sets are
//                        added in ascending s, each one plain fp32 add onto the running value, so how a list of
//                        sets is split over calls changes no bit.  Up to kMaxSets pointers travel by value in the
//                        kernel arguments; the entry point chunks longer lists.
//   argmax_scatter_rows  (E2) K17 for channels-last rows: out[xs[i], ys[j], zs[k]] = relabel[argmax_c
//                        scores[(i * cy + j) * cz + k, c]], first maximum.
//
// Both stream their operands once: one thread per row, consecutive threads on consecutive rows, 16 B per lane
// and tensor at the 4 classes the networks use.  E1 moves (n_sets + 2) * rows * classes * 4 bytes (n_sets + 1
// when it overwrites), E2 rows * (classes * 4 + 2).  No atomics, no LDS.
#include "gts_common.h"

namespace gts {
namespace {

constexpr int kMaxSets = 8;     // pointers per launch
constexpr int kMaxClasses = 8;  // row width of the generic loop

struct LogitSets {
  const float* p[kMaxSets];
};

// softmax of x[0..classes) added onto a[0..classes): one sequence of operations for both row layouts
template <int C>
__device__ __forceinline__ void add_softmax(const float (&x)[C], float (&a)[C], int classes) {
  float m = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c)
    if (c < classes) m = fmaxf(m, x[c]);
  float e[C];
  float denom = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (c < classes) e[c] = expf(x[c] - m), denom += e[c];
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (c < classes) a[c] += e[c] / denom;
}

template <bool WIDE>  // WIDE: classes == 4 and every pointer 16-byte aligned
__global__ __launch_bounds__(kBlock) void softmax_accumulate_kernel(LogitSets sets, int n_sets,
                                                                    float* __restrict__ acc, int64_t rows,
                                                                    int classes, int overwrite) {
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < rows;
       r += static_cast<int64_t>(gridDim.x) * kBlock) {
    if constexpr (WIDE) {
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      if (!overwrite) {
        const float4 t = *reinterpret_cast<const float4*>(acc + 4 * r);
        a[0] = t.x, a[1] = t.y, a[2] = t.z, a[3] = t.w;
      }
#pragma unroll
      for (int s = 0; s < kMaxSets; ++s) {  // unrolled: sets.p is only ever indexed by constants
        if (s < n_sets) {
          const Vec<4> v = Vec<4>::load_nt(sets.p[s] + 4 * r);
          add_softmax<4>(v.v, a, 4);
        }
      }
      *reinterpret_cast<float4*>(acc + 4 * r) = make_float4(a[0], a[1], a[2], a[3]);
    } else {
      float* row = acc + r * classes;
      float a[kMaxClasses];
#pragma unroll
      for (int c = 0; c < kMaxClasses; ++c) a[c] = (!overwrite && c < classes) ? row[c] : 0.f;
#pragma unroll
      for (int s = 0; s < kMaxSets; ++s) {
        if (s < n_sets) {
          const float* src = sets.p[s] + r * classes;
          float x[kMaxClasses];
#pragma unroll
          for (int c = 0; c < kMaxClasses; ++c) x[c] = c < classes ? src[c] : 0.f;
          add_softmax<kMaxClasses>(x, a, classes);
        }
      }
#pragma unroll
      for (int c = 0; c < kMaxClasses; ++c)
        if (c < classes) row[c] = a[c];
    }
  }
}

struct RowsBox {
  const int32_t* xs;
  const int32_t* ys;
  const int32_t* zs;
  int cx, cy, cz;    // cropped extents
  int dim_y, dim_z;  // full extents of the two inner axes
};

template <bool WIDE>  // WIDE: n_classes == 4 and scores 16-byte aligned
__global__ __launch_bounds__(kBlock) void argmax_scatter_rows_kernel(const float* __restrict__ scores,
                                                                     const int16_t* __restrict__ relabel,
                                                                     int16_t* __restrict__ out, RowsBox box,
                                                                     int n_classes) {
  const int64_t n_crop = static_cast<int64_t>(box.cx) * box.cy * box.cz;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < n_crop;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    int label = 0;
    if constexpr (WIDE) {
      const Vec<4> v = Vec<4>::load_nt(scores + 4 * t);
      float best = v.v[0];
#pragma unroll
      for (int c = 1; c < 4; ++c)
        if (best < v.v[c]) best = v.v[c], label = c;  // first maximum, like torch.argmax
    } else {
      const float* row = scores + t * n_classes;
      float best = row[0];
      for (int c = 1; c < n_classes; ++c) {
        const float val = row[c];
        if (best < val) best = val, label = c;
      }
    }
    if (relabel != nullptr) label = relabel[label];
    const int k = static_cast<int>(t % box.cz);
    const int64_t ij = t / box.cz;
    const int j = static_cast<int>(ij % box.cy), i = static_cast<int>(ij / box.cy);
    out[(static_cast<int64_t>(box.xs[i]) * box.dim_y + box.ys[j]) * box.dim_z + box.zs[k]] =
        static_cast<int16_t>(label);
  }
}

inline unsigned row_grid(int64_t rows) {
  const int64_t blocks = (rows + kBlock - 1) / kBlock;
  return static_cast<unsigned>(blocks > 8192 ? 8192 : blocks);
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_softmax_accumulate_f32(const float* const* sets, int64_t n_sets, float* acc, int64_t rows,
                                              int64_t classes, int32_t overwrite, void* stream) {
  using namespace gts;
  if (n_sets < 1 || n_sets > (1 << 20) || rows < 0 || classes < 1 || classes > kMaxClasses ||
      rows > (INT64_C(1) << 40))
    return GTS_ERR_SHAPE;
  if (rows == 0) return GTS_OK;
  if (!sets || !acc) return GTS_ERR_NULL;
  uintptr_t bits = reinterpret_cast<uintptr_t>(acc);
  for (int64_t s = 0; s < n_sets; ++s) {
    if (!sets[s]) return GTS_ERR_NULL;
    bits |= reinterpret_cast<uintptr_t>(sets[s]);
  }
  const bool wide = classes == 4 && (bits & 15) == 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int64_t first = 0; first < n_sets; first += kMaxSets) {
    LogitSets chunk{};
    const int n = static_cast<int>(n_sets - first < kMaxSets ? n_sets - first : kMaxSets);
    for (int s = 0; s < n; ++s) chunk.p[s] = sets[first + s];
    const int fresh = (overwrite != 0 && first == 0) ? 1 : 0;
    if (wide)
      softmax_accumulate_kernel<true><<<row_grid(rows), kBlock, 0, st>>>(chunk, n, acc, rows, 4, fresh);
    else
      softmax_accumulate_kernel<false><<<row_grid(rows), kBlock, 0, st>>>(chunk, n, acc, rows,
                                                                          static_cast<int>(classes), fresh);
    const int status = launch_status();
    if (status != GTS_OK) return status;
  }
  return GTS_OK;
}

extern "C" int32_t gts_argmax_scatter_rows_i16(const float* scores, const int16_t* relabel, const int32_t* xs,
                                               const int32_t* ys, const int32_t* zs, int16_t* out, int64_t cx,
                                               int64_t cy, int64_t cz, int64_t dim_y, int64_t dim_z,
                                               int64_t n_classes, void* stream) {
  using namespace gts;
  if (cx < 0 || cy < 0 || cz < 0 || cx > 32768 || cy > 32768 || cz > 32768 || dim_y < 1 || dim_z < 1 ||
      dim_y > 32768 || dim_z > 32768 || cy > dim_y || cz > dim_z || n_classes < 1 || n_classes > 1024)
    return GTS_ERR_SHAPE;
  const int64_t n_crop = cx * cy * cz;
  if (n_crop == 0) return GTS_OK;
  if (!scores || !xs || !ys || !zs || !out) return GTS_ERR_NULL;
  const RowsBox box{xs, ys, zs, static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(cz),
                    static_cast<int>(dim_y), static_cast<int>(dim_z)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_classes == 4 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0)
    argmax_scatter_rows_kernel<true><<<row_grid(n_crop), kBlock, 0, st>>>(scores, relabel, out, box, 4);
  else
    argmax_scatter_rows_kernel<false><<<row_grid(n_crop), kBlock, 0, st>>>(scores, relabel, out, box,
                                                                           static_cast<int>(n_classes));
  return launch_status();
}
