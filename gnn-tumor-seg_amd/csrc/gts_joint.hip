// K16/K17: device glue between the GNN and the refinement CNN of the joint predictor
// (/root/reference/scripts/generate_joint_predictions.py:59-73, model/cnn_model.py:85-88).
//
//   crop_concat     cnn_in[c, i, j, k] = c < Ci ? img[xs[i], ys[j], zs[k], c]
//                                               : table_plus_bg[svs[xs[i], ys[j], zs[k]]][c - Ci]
//                   i.e. torch.cat([img, node_logits_plus_bg[svs]], -1)[np.ix_(xs, ys, zs)]
//                   .movedim(-1, 0) in one pass: the [X,Y,Z,4] voxel-logit volume and the
//                   [X,Y,Z,8] concatenation are never materialised.
//   argmax_scatter  out[xs[i], ys[j], zs[k]] = argmax_c scores[c, i, j, k]  (first maximum)
//                   i.e. brain_volume_preds[crop] = argmax(refined_logits, 0).
//
//   crop_concat_rows      (J1) crop_concat in channels-last: x[t, :] = [img[v_t, :], row(svs[v_t])], the layout
//                         the HIP convolutions (C1-C5) read: the input of the joint TRAINING step.
//   crop_concat_rows_bwd  (J2) its adjoint with respect to the table: d_table[n, :] = sum of dx[t, Ci:] over the
//                         crop voxels t that took table row n.  One wave per node walks the node's voxel list
//                         (raster order, built once per sample), lane-strided partial sums, then a fixed
//                         shuffle tree: no float atomics, the same bits on every run.
//
// K16 / K17 / J1 are HBM-bound copies over the cropped box.  One thread per cropped voxel, consecutive
// threads along k (the contiguous axis of img / svs and of every channel plane), so channel-plane
// accesses are fully coalesced and the channels-last reads are 16 B per lane.
#include "gts_common.h"

namespace gts {
namespace {

struct Box {
  const int32_t* xs;
  const int32_t* ys;
  const int32_t* zs;
  int cx, cy, cz;      // cropped extents
  int dim_y, dim_z;    // full extents of the two inner axes
};

__device__ __forceinline__ int64_t source_voxel(const Box& b, int64_t t) {
  const int k = static_cast<int>(t % b.cz);
  const int64_t ij = t / b.cz;
  const int j = static_cast<int>(ij % b.cy), i = static_cast<int>(ij / b.cy);
  return (static_cast<int64_t>(b.xs[i]) * b.dim_y + b.ys[j]) * b.dim_z + b.zs[k];
}

template <int CI, int CT>  // 0 = runtime width
__global__ __launch_bounds__(kBlock) void crop_concat_kernel(
    const float* __restrict__ img, const int16_t* __restrict__ svs, const float* __restrict__ table,
    const float* __restrict__ bg_row, float* __restrict__ out, Box box, int n_rows, int ci_rt,
    int ct_rt) {
  const int ci = CI ? CI : ci_rt, ct = CT ? CT : ct_rt;
  const int64_t n_crop = static_cast<int64_t>(box.cx) * box.cy * box.cz;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < n_crop;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t v = source_voxel(box, t);
    const int id = svs[v];
    const int r = id < 0 ? id + n_rows + 1 : id;  // numpy: table_plus_bg[id]
    const float* row = (r < 0 || r >= n_rows) ? bg_row : table + static_cast<size_t>(r) * ct;
    if constexpr (CI == 4 && CT == 4) {
      const float4 a = *reinterpret_cast<const float4*>(img + 4 * v);
      const float4 b = *reinterpret_cast<const float4*>(row);
      out[t] = a.x, out[n_crop + t] = a.y, out[2 * n_crop + t] = a.z, out[3 * n_crop + t] = a.w;
      out[4 * n_crop + t] = b.x, out[5 * n_crop + t] = b.y;
      out[6 * n_crop + t] = b.z, out[7 * n_crop + t] = b.w;
    } else {
      for (int c = 0; c < ci; ++c) out[c * n_crop + t] = img[static_cast<size_t>(v) * ci + c];
      for (int c = 0; c < ct; ++c) out[(ci + c) * n_crop + t] = row[c];
    }
  }
}

__global__ __launch_bounds__(kBlock) void argmax_scatter_kernel(
    const float* __restrict__ scores, const int16_t* __restrict__ relabel,
    int16_t* __restrict__ out, Box box, int n_classes) {
  const int64_t n_crop = static_cast<int64_t>(box.cx) * box.cy * box.cz;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < n_crop;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    float best = scores[t];
    int label = 0;
    for (int c = 1; c < n_classes; ++c) {
      const float val = scores[c * n_crop + t];
      if (best < val) best = val, label = c;  // first maximum, like torch.argmax
    }
    if (relabel != nullptr) label = relabel[label];
    out[source_voxel(box, t)] = static_cast<int16_t>(label);
  }
}

template <int CI, int CT>  // 0 = runtime width
__global__ __launch_bounds__(kBlock) void crop_concat_rows_kernel(
    const float* __restrict__ img, const int16_t* __restrict__ svs, const float* __restrict__ table,
    const float* __restrict__ bg_row, float* __restrict__ out, Box box, int n_rows, int ci_rt,
    int ct_rt) {
  const int ci = CI ? CI : ci_rt, ct = CT ? CT : ct_rt;
  const int64_t n_crop = static_cast<int64_t>(box.cx) * box.cy * box.cz;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; t < n_crop;
       t += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t v = source_voxel(box, t);
    const int id = svs[v];
    const int r = id < 0 ? id + n_rows + 1 : id;  // numpy: table_plus_bg[id]
    const float* row = (r < 0 || r >= n_rows) ? bg_row : table + static_cast<size_t>(r) * ct;
    float* o = out + static_cast<size_t>(t) * (ci + ct);
    if constexpr (CI == 4 && CT == 4) {
      reinterpret_cast<float4*>(o)[0] = *reinterpret_cast<const float4*>(img + 4 * v);
      reinterpret_cast<float4*>(o)[1] = *reinterpret_cast<const float4*>(row);
    } else {
      for (int c = 0; c < ci; ++c) o[c] = img[static_cast<size_t>(v) * ci + c];
      for (int c = 0; c < ct; ++c) o[ci + c] = row[c];
    }
  }
}

struct RowsBwd {
  const float* dx;          // [n_crop, stride]; columns off .. off + ct are summed
  const int32_t* list_ptr;  // [n_rows + 1] extents of every node's voxel list
  const int32_t* list_vox;  // linear index into the full volume, raster order inside a node
  const int32_t* inv_x;     // full plane index -> crop index, or -1 outside the box
  const int32_t* inv_y;
  const int32_t* inv_z;
  float* d_table;           // [n_rows, ct]
  int cx, cy, cz, dim_x, dim_y, dim_z, n_rows, stride, off, ct;
};

// crop row of full-volume voxel v, or -1 when v lies outside the box (or outside the volume)
__device__ __forceinline__ int64_t crop_row(const RowsBwd& a, int v) {
  const int plane = a.dim_y * a.dim_z;
  if (v < 0) return -1;
  const int x = v / plane, yz = v - x * plane;
  if (x >= a.dim_x) return -1;
  const int y = yz / a.dim_z, z = yz - y * a.dim_z;
  const int i = a.inv_x[x], j = a.inv_y[y], k = a.inv_z[z];
  if (static_cast<unsigned>(i) >= static_cast<unsigned>(a.cx) ||
      static_cast<unsigned>(j) >= static_cast<unsigned>(a.cy) ||
      static_cast<unsigned>(k) >= static_cast<unsigned>(a.cz))
    return -1;
  return (static_cast<int64_t>(i) * a.cy + j) * a.cz + k;
}

// lane 0 ends with the lanes' values added in one fixed tree (strides 32, 16, ..., 1)
__device__ __forceinline__ float wave_tree_sum(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;
}

template <int CT>  // 4: one 16-byte load per voxel; 0: runtime width, one channel at a time
__global__ __launch_bounds__(kBlock) void crop_concat_rows_bwd_kernel(RowsBwd a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int waves = gridDim.x * kWavesPerBlock;
  for (int node = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; node < a.n_rows; node += waves) {
    const int begin = a.list_ptr[node], end = a.list_ptr[node + 1];
    if constexpr (CT == 4) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int e = begin + lane; e < end; e += kWave) {
        const int64_t t = crop_row(a, a.list_vox[e]);
        if (t < 0) continue;
        const float4 g = *reinterpret_cast<const float4*>(a.dx + t * a.stride + a.off);
        acc.x += g.x, acc.y += g.y, acc.z += g.z, acc.w += g.w;
      }
      acc.x = wave_tree_sum(acc.x), acc.y = wave_tree_sum(acc.y);
      acc.z = wave_tree_sum(acc.z), acc.w = wave_tree_sum(acc.w);
      if (lane == 0) *reinterpret_cast<float4*>(a.d_table + static_cast<size_t>(node) * 4) = acc;
    } else {
      for (int c = 0; c < a.ct; ++c) {
        float acc = 0.f;
        for (int e = begin + lane; e < end; e += kWave) {
          const int64_t t = crop_row(a, a.list_vox[e]);
          if (t >= 0) acc += a.dx[t * a.stride + a.off + c];
        }
        acc = wave_tree_sum(acc);
        if (lane == 0) a.d_table[static_cast<size_t>(node) * a.ct + c] = acc;
      }
    }
  }
}

inline unsigned crop_grid(int64_t n_crop) {
  const int64_t blocks = (n_crop + kBlock - 1) / kBlock;
  return static_cast<unsigned>(blocks > 8192 ? 8192 : blocks);
}

inline bool bad_box(int64_t cx, int64_t cy, int64_t cz, int64_t dim_y, int64_t dim_z) {
  return cx < 0 || cy < 0 || cz < 0 || cx > 32768 || cy > 32768 || cz > 32768 || dim_y < 1 ||
         dim_z < 1 || dim_y > 32768 || dim_z > 32768 || cy > dim_y || cz > dim_z;
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_crop_concat_f32(const float* img, const int16_t* svs, const float* table,
                                       const float* bg_row, const int32_t* xs, const int32_t* ys,
                                       const int32_t* zs, float* out, int64_t cx, int64_t cy,
                                       int64_t cz, int64_t dim_y, int64_t dim_z, int64_t n_rows,
                                       int64_t img_channels, int64_t row_channels, void* stream) {
  using namespace gts;
  if (bad_box(cx, cy, cz, dim_y, dim_z) || n_rows < 0 || n_rows > 32768 || img_channels < 0 ||
      row_channels < 1 || img_channels > 64 || row_channels > 64)
    return GTS_ERR_SHAPE;
  const int64_t n_crop = cx * cy * cz;
  if (n_crop == 0) return GTS_OK;
  if (!svs || !bg_row || !xs || !ys || !zs || !out || (img_channels > 0 && !img) ||
      (n_rows > 0 && !table))
    return GTS_ERR_NULL;
  const Box box{xs, ys, zs, static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(cz),
                static_cast<int>(dim_y), static_cast<int>(dim_z)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool wide = img_channels == 4 && row_channels == 4 &&
                    ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(table) |
                      reinterpret_cast<uintptr_t>(bg_row)) & 15) == 0;
  if (wide)
    crop_concat_kernel<4, 4><<<crop_grid(n_crop), kBlock, 0, st>>>(
        img, svs, table, bg_row, out, box, static_cast<int>(n_rows), 4, 4);
  else
    crop_concat_kernel<0, 0><<<crop_grid(n_crop), kBlock, 0, st>>>(
        img, svs, table, bg_row, out, box, static_cast<int>(n_rows), static_cast<int>(img_channels),
        static_cast<int>(row_channels));
  return launch_status();
}

extern "C" int32_t gts_argmax_scatter_i16(const float* scores, const int16_t* relabel,
                                          const int32_t* xs, const int32_t* ys, const int32_t* zs,
                                          int16_t* out, int64_t cx, int64_t cy, int64_t cz,
                                          int64_t dim_y, int64_t dim_z, int64_t n_classes,
                                          void* stream) {
  using namespace gts;
  if (bad_box(cx, cy, cz, dim_y, dim_z) || n_classes < 1 || n_classes > 1024) return GTS_ERR_SHAPE;
  const int64_t n_crop = cx * cy * cz;
  if (n_crop == 0) return GTS_OK;
  if (!scores || !xs || !ys || !zs || !out) return GTS_ERR_NULL;
  const Box box{xs, ys, zs, static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(cz),
                static_cast<int>(dim_y), static_cast<int>(dim_z)};
  argmax_scatter_kernel<<<crop_grid(n_crop), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      scores, relabel, out, box, static_cast<int>(n_classes));
  return launch_status();
}

extern "C" int32_t gts_crop_concat_rows_f32(const float* img, const int16_t* svs, const float* table,
                                            const float* bg_row, const int32_t* xs, const int32_t* ys,
                                            const int32_t* zs, float* out, int64_t cx, int64_t cy,
                                            int64_t cz, int64_t dim_y, int64_t dim_z, int64_t n_rows,
                                            int64_t img_channels, int64_t row_channels, void* stream) {
  using namespace gts;
  if (bad_box(cx, cy, cz, dim_y, dim_z) || n_rows < 0 || n_rows > 32768 || img_channels < 0 ||
      row_channels < 1 || img_channels > 64 || row_channels > 64)
    return GTS_ERR_SHAPE;
  const int64_t n_crop = cx * cy * cz;
  if (n_crop == 0) return GTS_OK;
  if (!svs || !bg_row || !xs || !ys || !zs || !out || (img_channels > 0 && !img) ||
      (n_rows > 0 && !table))
    return GTS_ERR_NULL;
  const Box box{xs, ys, zs, static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(cz),
                static_cast<int>(dim_y), static_cast<int>(dim_z)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool wide = img_channels == 4 && row_channels == 4 &&
                    ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(table) |
                      reinterpret_cast<uintptr_t>(bg_row) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  if (wide)
    crop_concat_rows_kernel<4, 4><<<crop_grid(n_crop), kBlock, 0, st>>>(
        img, svs, table, bg_row, out, box, static_cast<int>(n_rows), 4, 4);
  else
    crop_concat_rows_kernel<0, 0><<<crop_grid(n_crop), kBlock, 0, st>>>(
        img, svs, table, bg_row, out, box, static_cast<int>(n_rows), static_cast<int>(img_channels),
        static_cast<int>(row_channels));
  return launch_status();
}

extern "C" int32_t gts_crop_concat_rows_bwd_f32(const float* dx, const int32_t* list_ptr, const int32_t* list_vox,
                                                const int32_t* inv_x, const int32_t* inv_y, const int32_t* inv_z,
                                                float* d_table, int64_t cx, int64_t cy, int64_t cz, int64_t dim_x,
                                                int64_t dim_y, int64_t dim_z, int64_t n_rows, int64_t img_channels,
                                                int64_t row_channels, void* stream) {
  using namespace gts;
  if (bad_box(cx, cy, cz, dim_y, dim_z) || dim_x < 1 || dim_x > 32768 || cx > dim_x ||
      dim_x * dim_y * dim_z >= (1LL << 31) || n_rows < 0 || n_rows > 32768 || img_channels < 0 ||
      row_channels < 1 || img_channels > 64 || row_channels > 64)
    return GTS_ERR_SHAPE;
  if (n_rows == 0) return GTS_OK;
  const int64_t n_crop = cx * cy * cz;
  if (!list_ptr || !list_vox || !inv_x || !inv_y || !inv_z || !d_table || (n_crop > 0 && !dx))
    return GTS_ERR_NULL;
  const RowsBwd a{dx, list_ptr, list_vox, inv_x, inv_y, inv_z, d_table,
                  static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(cz), static_cast<int>(dim_x),
                  static_cast<int>(dim_y), static_cast<int>(dim_z), static_cast<int>(n_rows),
                  static_cast<int>(img_channels + row_channels), static_cast<int>(img_channels),
                  static_cast<int>(row_channels)};
  const int64_t blocks = (n_rows + kWavesPerBlock - 1) / kWavesPerBlock;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool wide = row_channels == 4 && img_channels % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(d_table)) & 15) == 0;
  if (wide)
    crop_concat_rows_bwd_kernel<4><<<static_cast<unsigned>(blocks), kBlock, 0, st>>>(a);
  else
    crop_concat_rows_bwd_kernel<0><<<static_cast<unsigned>(blocks), kBlock, 0, st>>>(a);
  return launch_status();
}
