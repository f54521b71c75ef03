// L1-L3: the device half of the BraTS 2023 lesion-wise Dice / HD95 (gts/lesionwise.py).  What a
// user otherwise does on the host with scipy's binary_dilation, two ndimage.label calls and one np.isin per
// lesion.  The components themselves come from C1-C3 and the per-lesion HD95 from H1-H5, both unchanged.
//
//   L1  region dilation: the region mask of an int16 label volume is packed to bits along Z (one 64-voxel
//       word per wave ballot), then every output word is the OR of the (2n+1)^2 neighbouring rows' words,
//       each dilated along Z by rho(dx, dy) = min(n, 2n - |dx| - |dy|) with the carries of the two adjacent
//       words.  Rows are staged in LDS; rows and words outside the volume are zero, so nothing wraps and the
//       result is clipped at every face.  n iterations of scipy's generate_binary_structure(3, 2) in one pass.
//       The result is written as an int16 0/1 volume, which C1-C3 take as they are.
//   L2  lesion and match tables.  Every root voxel of D (a lesion) and of P (a predicted component) takes a
//       dense slot from an atomic cursor; then one pass over the voxels adds, per lesion, |G_k|, |P n G_k| and
//       the box of G_k, per component its size and box, and appends the (component root, lesion root) pair of
//       a voxel of P n D that has no such voxel among its 13 preceding 26-neighbours.  Two voxels that append
//       are never 26-adjacent, and no two roots are, so ceil(X/2) * ceil(Y/2) * ceil(Z/2) bounds every list:
//       the buffers are sized for the worst case and cannot overflow.  A last pass packs the three lists into
//       one block for a single copy.  Slot order is arrival order; every row carries its root, the host sorts
//       by it, and no value depends on the order.
//   L3  lesion masks: M_k (the predicted voxels whose root is in a sorted list) and G_k (the truth region
//       voxels whose D root is the lesion's) as label 3 over a box of the volume, the input pair of H1.
//
// Integer arithmetic and integer atomics (add, max) only: identical results on every run.  The region rule
// (in_region, the one H1 uses), the volume limit, the per-key wave loop of L2 and L2's bound are the shared headers'.
#include "gts_lesions.h"

namespace gts {
namespace {

constexpr int kRowInts = 9;  // root | count | tp | x_hi x_lo y_hi y_lo z_hi z_lo
constexpr int kTileX = 8, kTileY = 8, kTileW = 4;  // L1: rows and words of one workgroup, kBlock in all
constexpr int kMaxDilation = 3;
constexpr int kMaxBlocks = 1 << 20;  // grid cap of the strided kernels
typedef unsigned long long word_t;

static_assert(kTileX * kTileY * kTileW == kBlock, "one thread per output word");

// L1, packing.  Wave u owns word u = (row, w): voxels z = 64 w + lane of the row.
__global__ __launch_bounds__(kBlock) void lesion_pack_kernel(const int16_t* __restrict__ lab,
                                                             word_t* __restrict__ bits, int64_t words, int W, int Z,
                                                             int region) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t u = int64_t{blockIdx.x} * kWavesPerBlock + threadIdx.x / kWave; u < words;
       u += int64_t{gridDim.x} * kWavesPerBlock) {
    const int64_t row = u / W;
    const int64_t z = (u % W) * kWave + lane;
    const bool on = z < Z && in_region(lab[row * Z + z], region);
    const word_t mask = __ballot(on);
    if (lane == 0) bits[u] = mask;
  }
}

// L1, dilation by the footprint { o : max |o_i| <= N, sum |o_i| <= 2 N }.
template <int N>
__global__ __launch_bounds__(kBlock) void lesion_dilate_kernel(const word_t* __restrict__ bits,
                                                               int16_t* __restrict__ out, int X, int Y, int Z, int W,
                                                               int tiles_y, int tiles_w, int64_t tiles) {
  constexpr int SX = kTileX + 2 * N, SY = kTileY + 2 * N, SW = kTileW + 2;
  __shared__ word_t rows[SX][SY][SW];
  __shared__ word_t result[kBlock];
  const int tid = threadIdx.x;
  const int tw = tid % kTileW, ty = (tid / kTileW) % kTileY, tx = tid / (kTileW * kTileY);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int w0 = static_cast<int>(tile % tiles_w) * kTileW;
    const int y0 = static_cast<int>((tile / tiles_w) % tiles_y) * kTileY;
    const int x0 = static_cast<int>(tile / (int64_t{tiles_w} * tiles_y)) * kTileX;
    for (int e = tid; e < SX * SY * SW; e += kBlock) {
      const int lw = e % SW, ly = (e / SW) % SY, lx = e / (SW * SY);
      const int64_t gx = int64_t{x0} - N + lx, gy = int64_t{y0} - N + ly, gw = int64_t{w0} - 1 + lw;
      const bool inside = gx >= 0 && gx < X && gy >= 0 && gy < Y && gw >= 0 && gw < W;
      rows[lx][ly][lw] = inside ? bits[(gx * Y + gy) * W + gw] : 0;
    }
    __syncthreads();
    // per Z radius: the OR of the rows that reach this far (below, own and above word)
    word_t lo[N + 1], mid[N + 1], hi[N + 1];
#pragma unroll
    for (int s = 0; s <= N; ++s) lo[s] = mid[s] = hi[s] = 0;
#pragma unroll
    for (int dx = -N; dx <= N; ++dx) {
#pragma unroll
      for (int dy = -N; dy <= N; ++dy) {
        const int reach = 2 * N - (dx < 0 ? -dx : dx) - (dy < 0 ? -dy : dy);
        const int rho = reach < N ? reach : N;
        const word_t* t = &rows[tx + N + dx][ty + N + dy][tw];
        lo[rho] |= t[0];
        mid[rho] |= t[1];
        hi[rho] |= t[2];
      }
    }
    word_t acc = 0;
#pragma unroll
    for (int s = N; s >= 1; --s) {  // a row that reaches s also reaches s - 1
      acc |= (mid[s] << s) | (mid[s] >> s) | (lo[s] >> (kWave - s)) | (hi[s] << (kWave - s));
      lo[s - 1] |= lo[s];
      mid[s - 1] |= mid[s];
      hi[s - 1] |= hi[s];
    }
    acc |= mid[0];
    result[tid] = acc;
    __syncthreads();
    // one wave per word: 64 consecutive int16 of a row
    const int lane = tid & (kWave - 1);
    for (int u = tid / kWave; u < kBlock; u += kWavesPerBlock) {
      const int gw = w0 + u % kTileW, gy = y0 + (u / kTileW) % kTileY, gx = x0 + u / (kTileW * kTileY);
      const int64_t z = int64_t{gw} * kWave + lane;
      if (gx < X && gy < Y && gw < W && z < Z)
        out[(int64_t{gx} * Y + gy) * Z + z] = static_cast<int16_t>((result[u] >> lane) & 1ull);
    }
    __syncthreads();
  }
}

// L2, slots.  cursors: {lesions, components, pairs}.
__global__ __launch_bounds__(kBlock) void lesion_slots_kernel(const int* __restrict__ roots_p,
                                                              const int* __restrict__ roots_d, int* __restrict__ slot_p,
                                                              int* __restrict__ slot_d, int* __restrict__ lesions,
                                                              int* __restrict__ comps, int* cursors, int64_t n,
                                                              int cap) {
  const int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  if (i >= n) return;
  if (roots_d[i] == i + 1) {
    const int s = atomicAdd(&cursors[0], 1);
    slot_d[i] = s;
    if (s < cap) lesions[int64_t{s} * kRowInts] = static_cast<int>(i) + 1;
  }
  if (roots_p[i] == i + 1) {
    const int s = atomicAdd(&cursors[1], 1);
    slot_p[i] = s;
    if (s < cap) comps[int64_t{s} * kRowInts] = static_cast<int>(i) + 1;
  }
}

// The lanes that are `on` add one to column 1 of row `slot` of `table` (and `tp` to column 2) and raise its
// box by their own.  Lanes of one slot are summed in the wave first: a large lesion would otherwise put
// eight atomics per voxel on one row.
__device__ __forceinline__ void wave_add_rows(int* table, bool on, int slot, bool tp, const int (&box)[6], int lane) {
  wave_for_each_key(on, slot, [&](int key, word_t same, bool mine) {
    const int count = __popcll(same);
    const int hits = __popcll(__ballot(mine && tp));
    int top[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      int v = mine ? box[k] : 0;
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {
        const int other = __shfl_xor(v, off, kWave);
        v = other > v ? other : v;
      }
      top[k] = v;
    }
    if (lane == 0) {
      int* row = table + int64_t{key} * kRowInts;
      atomicAdd(row + 1, count);
      if (hits) atomicAdd(row + 2, hits);
#pragma unroll
      for (int k = 0; k < 6; ++k) atomicMax(row + 3 + k, top[k]);
    }
  });
}

// L2, the tables.  Box entries are kept as maxima of coordinate + 1 and of extent - coordinate, so a cleared
// row is an empty box.
__global__ __launch_bounds__(kBlock) void lesion_tables_kernel(const int16_t* __restrict__ truth,
                                                               const int* __restrict__ roots_p,
                                                               const int* __restrict__ roots_d,
                                                               const int* __restrict__ slot_p,
                                                               const int* __restrict__ slot_d, int* lesions, int* comps,
                                                               int* __restrict__ pairs, int* cursors, int64_t n, int X,
                                                               int Y, int Z, int region, int cap) {
  const int64_t i64 = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const bool inside = i64 < n;
  const int i = inside ? static_cast<int>(i64) : 0;
  const int yz = Y * Z;  // < 2^31: a factor of n
  const auto [x, y, z] = split_xyz(i, Y, Z);
  const int rp = inside ? roots_p[i] : 0;
  const int rd = inside ? roots_d[i] : 0;
  const bool g = inside && rd != 0 && in_region(truth[i], region);
  const int box[6] = {x + 1, X - x, y + 1, Y - y, z + 1, Z - z};
  const int sd = g ? slot_d[rd - 1] : 0, sp = rp != 0 ? slot_p[rp - 1] : 0;  // < cap for the roots of C1-C3
  if (__ballot(g)) wave_add_rows(lesions, g && sd < cap, sd, rp != 0, box, lane);
  if (__ballot(rp != 0)) wave_add_rows(comps, rp != 0 && sp < cap, sp, false, box, lane);
  if (rp == 0 || rd == 0) return;
  // the pair (rp, rd): 26-adjacent voxels of P share rp and those of D share rd, so a preceding neighbour
  // in both carries this very pair
  bool seen = false;
  for (int dx = -1; dx <= 0 && !seen; ++dx) {
    if (x + dx < 0) continue;
    for (int dy = -1; dy <= (dx < 0 ? 1 : 0) && !seen; ++dy) {
      if (y + dy < 0 || y + dy >= Y) continue;
      const int last = (dx < 0 || dy < 0) ? 1 : -1;
      for (int dz = -1; dz <= last; ++dz) {
        if (z + dz < 0 || z + dz >= Z) continue;
        const int j = i + dx * yz + dy * Z + dz;
        if (roots_p[j] != 0 && roots_d[j] != 0) {
          seen = true;
          break;
        }
      }
    }
  }
  if (seen) return;
  const int s = atomicAdd(&cursors[2], 1);
  if (s < cap) {
    pairs[2 * int64_t{s}] = rp;
    pairs[2 * int64_t{s} + 1] = rd;
  }
}

// L2, packing: out = {lesions, components, pairs, 0} | lesion rows | component rows | pairs
__global__ __launch_bounds__(kBlock) void lesion_pack_tables_kernel(const int* __restrict__ lesions,
                                                                    const int* __restrict__ comps,
                                                                    const int* __restrict__ pairs,
                                                                    const int* __restrict__ cursors,
                                                                    int* __restrict__ out, int cap) {
  const int n_l = cursors[0] < cap ? cursors[0] : cap, n_c = cursors[1] < cap ? cursors[1] : cap;
  const int n_p = cursors[2] < cap ? cursors[2] : cap;  // never more (see above); the clamp keeps `out` safe regardless
  const int64_t a = int64_t{n_l} * kRowInts, b = int64_t{n_c} * kRowInts, c = 2 * int64_t{n_p};
  for (int64_t e = int64_t{blockIdx.x} * kBlock + threadIdx.x; e < 4 + a + b + c; e += int64_t{gridDim.x} * kBlock) {
    int v;
    if (e < 4)
      v = e < 3 ? cursors[e] : 0;
    else if (e < 4 + a)
      v = lesions[e - 4];
    else if (e < 4 + a + b)
      v = comps[e - 4 - a];
    else
      v = pairs[e - 4 - a - b];
    out[e] = v;
  }
}

// L3.  One lane per voxel of the box; matched: ascending component roots.
__global__ __launch_bounds__(kBlock) void lesion_masks_kernel(const int16_t* __restrict__ truth,
                                                              const int* __restrict__ roots_p,
                                                              const int* __restrict__ roots_d,
                                                              const int* __restrict__ matched, int n_matched,
                                                              int lesion_root, int region, int Y, int Z, int x0, int y0,
                                                              int z0, int cy, int cz, int64_t count,
                                                              int16_t* __restrict__ mask_m,
                                                              int16_t* __restrict__ mask_g) {
  const int64_t e = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  if (e >= count) return;
  const auto at = split_xyz(e, cy, cz);  // inside the box
  const int64_t i = ((x0 + at.x) * Y + y0 + at.y) * Z + z0 + at.z;
  const int rp = roots_p[i];
  bool member = false;
  if (rp != 0) {
    int lo = 0, hi = n_matched;  // first entry >= rp
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (matched[mid] < rp)
        lo = mid + 1;
      else
        hi = mid;
    }
    member = lo < n_matched && matched[lo] == rp;
  }
  mask_m[e] = member ? 3 : 0;
  mask_g[e] = roots_d[i] == lesion_root && in_region(truth[i], region) ? 3 : 0;
}

// every extent >= 1: the dilation tiles and the 2 x 2 x 2 cells below have no empty case
inline bool lesion_voxels(int64_t X, int64_t Y, int64_t Z, int64_t* n) { return volume_voxels(X, Y, Z, false, n); }

inline int64_t lesion_words(int64_t X, int64_t Y, int64_t Z) { return X * Y * ((Z + kWave - 1) / kWave); }

// L2: cursors | slot_p int32[n] | slot_d int32[n] | lesion rows | component rows | pairs
inline int64_t lesion_tables_bytes(int64_t n, int64_t cells) {
  return kHeaderBytes + 2 * round256(4 * n) + 2 * round256(4 * kRowInts * cells) + round256(8 * cells);
}

template <int N>
void launch_dilate(const word_t* bits, int16_t* out, int X, int Y, int Z, int W, hipStream_t st) {
  const int tiles_y = (Y + kTileY - 1) / kTileY, tiles_w = (W + kTileW - 1) / kTileW;
  const int64_t tiles = int64_t{(X + kTileX - 1) / kTileX} * tiles_y * tiles_w;
  lesion_dilate_kernel<N><<<blocks_for(tiles, 1, kMaxBlocks), kBlock, 0, st>>>(bits, out, X, Y, Z, W, tiles_y, tiles_w,
                                                                               tiles);
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_lesionwise_workspace(int64_t X, int64_t Y, int64_t Z) {
  int64_t n;
  if (!gts::lesion_voxels(X, Y, Z, &n)) return 0;
  const int64_t dilate = gts::round256(8 * gts::lesion_words(X, Y, Z));
  const int64_t tables = gts::lesion_tables_bytes(n, gts::lesion_rows(X, Y, Z, 26));
  return dilate > tables ? dilate : tables;
}

extern "C" int64_t gts_lesionwise_table_ints(int64_t X, int64_t Y, int64_t Z) {
  int64_t n;
  if (!gts::lesion_voxels(X, Y, Z, &n)) return 0;
  return 4 + (2 * gts::kRowInts + 2) * gts::lesion_rows(X, Y, Z, 26);
}

extern "C" int32_t gts_lesionwise_dilate_i16(const int16_t* labels, int64_t X, int64_t Y, int64_t Z, int32_t region,
                                             int32_t dilation, int16_t* mask_out, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!labels || !mask_out || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!lesion_voxels(X, Y, Z, &n)) return GTS_ERR_SHAPE;
  if (region < 0 || region > 2 || dilation < 0 || dilation > kMaxDilation) return GTS_ERR_ARGKIND;
  const int64_t words = lesion_words(X, Y, Z);
  if (workspace_bytes < 8 * words) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  word_t* bits = static_cast<word_t*>(workspace);
  const int W = static_cast<int>((Z + kWave - 1) / kWave);
  lesion_pack_kernel<<<blocks_for(words, kWavesPerBlock, kMaxBlocks), kBlock, 0, st>>>(labels, bits, words, W,
                                                                                      static_cast<int>(Z), region);
  const int x = static_cast<int>(X), y = static_cast<int>(Y), z = static_cast<int>(Z);
  switch (dilation) {
    case 0: launch_dilate<0>(bits, mask_out, x, y, z, W, st); break;
    case 1: launch_dilate<1>(bits, mask_out, x, y, z, W, st); break;
    case 2: launch_dilate<2>(bits, mask_out, x, y, z, W, st); break;
    default: launch_dilate<3>(bits, mask_out, x, y, z, W, st); break;
  }
  return launch_status();
}

extern "C" int32_t gts_lesionwise_tables_i16(const int16_t* truth, const int32_t* pred_roots,
                                             const int32_t* dilated_roots, int64_t X, int64_t Y, int64_t Z,
                                             int32_t region, int32_t* tables_out, int64_t tables_ints, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!truth || !pred_roots || !dilated_roots || !tables_out || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!lesion_voxels(X, Y, Z, &n)) return GTS_ERR_SHAPE;
  if (region < 0 || region > 2) return GTS_ERR_ARGKIND;
  const int64_t cells = lesion_rows(X, Y, Z, 26);  // roots, and appended pairs, are pairwise not 26-adjacent
  if (workspace_bytes < lesion_tables_bytes(n, cells) || tables_ints < 4 + (2 * kRowInts + 2) * cells)
    return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  int* cursors = reinterpret_cast<int*>(ws);
  int* slot_p = reinterpret_cast<int*>(ws + kHeaderBytes);
  int* slot_d = reinterpret_cast<int*>(ws + kHeaderBytes + round256(4 * n));
  char* rows = ws + kHeaderBytes + 2 * round256(4 * n);
  const int64_t row_bytes = round256(4 * kRowInts * cells);
  int* lesions = reinterpret_cast<int*>(rows);
  int* comps = reinterpret_cast<int*>(rows + row_bytes);
  int* pairs = reinterpret_cast<int*>(rows + 2 * row_bytes);

  if (hipMemsetAsync(cursors, 0, kHeaderBytes, st) != hipSuccess) return launch_status();
  if (hipMemsetAsync(rows, 0, 2 * row_bytes, st) != hipSuccess) return launch_status();
  const int blocks = blocks_for(n, kBlock);
  const int cap = static_cast<int>(cells);
  lesion_slots_kernel<<<blocks, kBlock, 0, st>>>(pred_roots, dilated_roots, slot_p, slot_d, lesions, comps, cursors, n,
                                                 cap);
  lesion_tables_kernel<<<blocks, kBlock, 0, st>>>(truth, pred_roots, dilated_roots, slot_p, slot_d, lesions, comps,
                                                  pairs, cursors, n, static_cast<int>(X), static_cast<int>(Y),
                                                  static_cast<int>(Z), region, cap);
  lesion_pack_tables_kernel<<<1024, kBlock, 0, st>>>(lesions, comps, pairs, cursors, tables_out, cap);
  return launch_status();
}

extern "C" int32_t gts_lesionwise_masks_i16(const int16_t* truth, const int32_t* pred_roots,
                                            const int32_t* dilated_roots, int64_t X, int64_t Y, int64_t Z,
                                            int32_t region, int32_t lesion_root, const int32_t* matched_roots,
                                            int64_t n_matched, const int64_t* box, int16_t* mask_m, int16_t* mask_g,
                                            void* stream) {
  using namespace gts;
  if (!truth || !pred_roots || !dilated_roots || !box || !mask_m || !mask_g || (n_matched > 0 && !matched_roots))
    return GTS_ERR_NULL;
  int64_t n;
  if (!lesion_voxels(X, Y, Z, &n) || n_matched < 0 || n_matched > n || lesion_root < 1 || lesion_root > n)
    return GTS_ERR_SHAPE;
  if (region < 0 || region > 2) return GTS_ERR_ARGKIND;
  const int64_t extent[3] = {X, Y, Z};
  for (int a = 0; a < 3; ++a)
    if (box[2 * a] < 0 || box[2 * a] >= box[2 * a + 1] || box[2 * a + 1] > extent[a]) return GTS_ERR_SHAPE;
  const int64_t cx = box[1] - box[0], cy = box[3] - box[2], cz = box[5] - box[4];
  const int64_t count = cx * cy * cz;  // <= n
  lesion_masks_kernel<<<blocks_for(count, kBlock), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      truth, pred_roots, dilated_roots, matched_roots, static_cast<int>(n_matched), lesion_root, region,
      static_cast<int>(Y), static_cast<int>(Z), static_cast<int>(box[0]), static_cast<int>(box[2]),
      static_cast<int>(box[4]), static_cast<int>(cy), static_cast<int>(cz), count, mask_m, mask_g);
  return launch_status();
}
