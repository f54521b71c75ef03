// C1-C5: 3-D connected components of a label volume's foreground (label != 0) on the device, and the
// clean-up of a predicted segmentation built on them: whole-tumour components below a voxel count are
// dropped, and an implausibly small enhancing-tumour total is relabelled.  What a user otherwise does on
// the host with scipy.ndimage.label + np.bincount.
//
// A lock-free union-find over int32 parents indexed by the voxel's linear index (X * Y * Z < 2^31).
// parent[v] <= v at all times, so every walk goes strictly downward and ends; roots only ever move to
// smaller indices, so the root of a finished component is its smallest linear index whatever the order
// the unions ran in.  No workgroup ever waits for another: a union retries only while ITS OWN pair of
// roots keeps changing, and every retry strictly lowers the larger of the two.
//
//   C1  init: parent[v] = first voxel of v's run along Z inside its wave (found with a ballot), -1 for
//       background; the size table is cleared;
//   C2  merge: a voxel unites with the backward half of its neighbourhood (3 of 6, 13 of 26).  The
//       neighbours are taken line by line: with the Z runs already joined, a voxel whose predecessor in
//       the line is foreground only has to unite with what the predecessor could not see;
//   C3  flatten: roots[v] = 1 + find(v) (0 for background), parents compressed in place;
//   C4  sizes: an int32 count per root; a wave walks 1024 consecutive voxels and adds one total per
//       stretch of equal roots, so a large component does not serialise an atomic per voxel;
//   C5  filter: counts (components, removed components, removed voxels, surviving ET voxels), then the
//       output volume.  Two launches, because the ET rule needs the count over the whole volume first.
//
// Every result is an integer that does not depend on scheduling.  The volume limit, the workspace rounding
// and the wave and workgroup counting idioms of C4 and C5 are gts_volume.h's.
#include "gts_volume.h"

namespace gts {
namespace {

constexpr int kBackground = -1;
constexpr int kSizeChunks = 16;     // C4: 64-voxel chunks one wave walks
constexpr int kCountBlocks = 2048;  // C5: grid cap of the counting pass

// Parents change under the merge pass's feet.  A value read late is still an ancestor-or-self that was
// valid once (links are only ever replaced by the thread that then unites the old target with the new
// one), so staleness costs steps, never correctness; the agent-scope load keeps the CU's L1 out of it.
__device__ __forceinline__ int load_parent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int find_root(const int* parent, int v) {
  for (int p = load_parent(parent + v); p != v; p = load_parent(parent + v)) v = p;
  return v;
}

// Find both roots, point the larger at the smaller.  atomicMin returns what the parent really was: when
// that is not the root we believed in, someone else linked it first, the link we may just have replaced
// is re-established by going on from the value returned.  max(a, b) falls in every round.
__device__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

// C1.  One lane per voxel; the 64 voxels of a wave are consecutive linear indices.
__global__ __launch_bounds__(kBlock) void components_init_kernel(const int16_t* __restrict__ lab,
                                                                 int* __restrict__ parent, int* __restrict__ sizes,
                                                                 int64_t n, int Z) {
  const int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const bool inside = i < n;
  const bool fg = inside && lab[i] != 0;
  const unsigned long long mask = __ballot(fg);
  const bool start = fg && (lane == 0 || i % Z == 0 || !((mask >> (lane - 1)) & 1ull));
  const unsigned long long starts = __ballot(start);
  if (!inside) return;
  int p = kBackground;
  if (fg) {
    const int head = 63 - __clzll(static_cast<long long>(starts & (~0ull >> (63 - lane))));
    p = static_cast<int>(i) - (lane - head);
  }
  parent[i] = p;
  if (sizes) sizes[i] = 0;
}

// Unite voxel i (at depth z of its line, `prev`: its predecessor in the line is foreground) with the
// foreground it touches in the line whose voxel at the same depth is nb.  kDiag: the line's voxels at
// z - 1 and z + 1 touch i too (26-connectivity).  Runs along Z are one set already (C1, and the wave-seam
// union of C2), which is what lets a voxel with a foreground predecessor skip what that one covers.
template <bool kDiag>
__device__ __forceinline__ void unite_with_line(const int16_t* __restrict__ lab, int* parent, int i, int nb, int z,
                                                int Z, bool prev) {
  const bool centre = lab[nb] != 0;
  if (!kDiag) {
    if (centre && !(prev && lab[nb - 1] != 0)) unite(parent, i, nb);
    return;
  }
  const bool right = z + 1 < Z && lab[nb + 1] != 0;
  if (prev) {  // the predecessor touches nb - 1 and nb; nb + 1 is new unless nb joins it to them
    if (right && !centre) unite(parent, i, nb + 1);
    return;
  }
  if (centre) {  // nb - 1 and nb + 1 are in nb's run
    unite(parent, i, nb);
    return;
  }
  if (z > 0 && lab[nb - 1] != 0) unite(parent, i, nb - 1);
  if (right) unite(parent, i, nb + 1);
}

// C2.
template <bool kDiag>
__global__ __launch_bounds__(kBlock) void components_merge_kernel(const int16_t* __restrict__ lab, int* parent,
                                                                  int64_t n, int Y, int Z) {
  const int64_t i64 = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  if (i64 >= n || lab[i64] == 0) return;
  const int i = static_cast<int>(i64);
  const int yz = Y * Z;  // < 2^31: a factor of n
  const auto [x, y, z] = split_xyz(i, Y, Z);
  const bool prev = z > 0 && lab[i - 1] != 0;
  if (prev && (i & (kWave - 1)) == 0) unite(parent, i, i - 1);  // a run that C1 saw cut at the wave's edge
  if (y > 0) unite_with_line<kDiag>(lab, parent, i, i - Z, z, Z, prev);
  if (x > 0) {
    unite_with_line<kDiag>(lab, parent, i, i - yz, z, Z, prev);
    if (kDiag) {
      if (y > 0) unite_with_line<true>(lab, parent, i, i - yz - Z, z, Z, prev);
      if (y + 1 < Y) unite_with_line<true>(lab, parent, i, i - yz + Z, z, Z, prev);
    }
  }
}

// C3.  Nothing unites any more: every parent read is an ancestor, the only fixed point of a set is its
// root, and storing the root over a parent another lane is about to read only shortens that lane's walk.
__global__ __launch_bounds__(kBlock) void components_flatten_kernel(int* parent, int* __restrict__ roots, int64_t n) {
  const int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  if (i >= n) return;
  int v = parent[i];
  if (v < 0) {
    roots[i] = 0;
    return;
  }
  for (int p = parent[v]; p != v; p = parent[v]) v = p;
  parent[i] = v;
  roots[i] = v + 1;
}

// C4.  Wave w walks voxels [w * 1024, (w + 1) * 1024).  Per chunk the lanes are grouped by root with
// ballots; the running (root, count) pair is wave-uniform and goes to memory when the root changes.
__global__ __launch_bounds__(kBlock) void components_sizes_kernel(const int* __restrict__ roots,
                                                                  int* __restrict__ sizes, int64_t n) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = int64_t{blockIdx.x} * kWavesPerBlock + threadIdx.x / kWave;
  const int64_t base = wave * kWave * kSizeChunks;
  int run_root = 0, run_count = 0;
  for (int c = 0; c < kSizeChunks && base + c * kWave < n; ++c) {
    const int64_t i = base + c * kWave + lane;
    const int r = i < n ? roots[i] : 0;
    wave_for_each_key(r != 0, r, [&](int key, unsigned long long same, bool) {
      const int count = __popcll(same);
      if (key == run_root) {
        run_count += count;
      } else {
        if (run_count && lane == 0) atomicAdd(&sizes[run_root - 1], run_count);
        run_root = key;
        run_count = count;
      }
    });
  }
  if (run_count && lane == 0) atomicAdd(&sizes[run_root - 1], run_count);
}

// C5, counting.  counters: {components, components removed, voxels removed, surviving ET voxels}.
__global__ __launch_bounds__(kBlock) void components_count_kernel(const int16_t* __restrict__ lab,
                                                                  const int* __restrict__ roots,
                                                                  const int* __restrict__ sizes,
                                                                  unsigned long long* __restrict__ counters, int64_t n,
                                                                  int64_t min_voxels, int et_label, int et_on) {
  unsigned mine[4] = {0, 0, 0, 0};
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < n; i += int64_t{gridDim.x} * kBlock) {
    const int r = roots[i];
    if (r == 0) continue;
    const bool small = sizes[r - 1] < min_voxels;
    const bool is_root = r == i + 1;
    mine[0] += is_root;
    mine[1] += is_root && small;
    mine[2] += small;
    mine[3] += et_on && !small && lab[i] == et_label;
  }
  block_add_counters(mine, counters);
}

// C5, output.  in and out may be one buffer: a lane reads and writes its own voxel only.
__global__ __launch_bounds__(kBlock) void components_apply_kernel(const int16_t* in, int16_t* out,
                                                                  const int* __restrict__ roots,
                                                                  const int* __restrict__ sizes,
                                                                  const unsigned long long* __restrict__ counters,
                                                                  long long* __restrict__ stats, int64_t n,
                                                                  int64_t min_voxels, int et_label,
                                                                  int64_t et_min_voxels, int et_replacement) {
  const int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  const long long n_et = static_cast<long long>(counters[3]);
  const bool relabel = n_et > 0 && n_et < et_min_voxels;
  if (i == 0) {
    stats[0] = static_cast<long long>(counters[0]);
    stats[1] = static_cast<long long>(counters[1]);
    stats[2] = static_cast<long long>(counters[2]);
    stats[3] = relabel ? n_et : 0;
  }
  if (i >= n) return;
  int16_t v = in[i];
  const int r = roots[i];
  if (r != 0) {
    if (sizes[r - 1] < min_voxels)
      v = 0;
    else if (relabel && v == et_label)
      v = static_cast<int16_t>(et_replacement);
  }
  out[i] = v;
}

// an empty volume is a volume: the entry points return at once
inline bool components_voxels(int64_t X, int64_t Y, int64_t Z, int64_t* n) { return volume_voxels(X, Y, Z, true, n); }

// header (the four counters) | parent int32[n] | roots int32[n] | sizes int32[n]
inline int64_t components_bytes(int64_t n) { return kHeaderBytes + 3 * round256(4 * n); }

// C1-C3 into roots (int32[n]); sizes (may be NULL) is cleared on the way
int components_label(const int16_t* lab, int64_t n, int Y, int Z, int connectivity, int* parent, int* roots, int* sizes,
                     hipStream_t st) {
  const int blocks = blocks_for(n, kBlock);
  components_init_kernel<<<blocks, kBlock, 0, st>>>(lab, parent, sizes, n, Z);
  if (connectivity == 26)
    components_merge_kernel<true><<<blocks, kBlock, 0, st>>>(lab, parent, n, Y, Z);
  else
    components_merge_kernel<false><<<blocks, kBlock, 0, st>>>(lab, parent, n, Y, Z);
  components_flatten_kernel<<<blocks, kBlock, 0, st>>>(parent, roots, n);
  return launch_status();
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_components_workspace(int64_t X, int64_t Y, int64_t Z) {
  int64_t n;
  if (!gts::components_voxels(X, Y, Z, &n) || n == 0) return 0;
  return gts::components_bytes(n);
}

extern "C" int32_t gts_components_roots_i16(const int16_t* labels, int64_t X, int64_t Y, int64_t Z,
                                            int32_t connectivity, int32_t* roots_out, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!labels || !roots_out || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!components_voxels(X, Y, Z, &n) || (connectivity != 6 && connectivity != 26)) return GTS_ERR_SHAPE;
  if (n == 0) return GTS_OK;
  if (workspace_bytes < components_bytes(n)) return GTS_ERR_SHAPE;
  int* parent = reinterpret_cast<int*>(static_cast<char*>(workspace) + kHeaderBytes);
  return components_label(labels, n, static_cast<int>(Y), static_cast<int>(Z), connectivity, parent, roots_out, nullptr,
                          static_cast<hipStream_t>(stream));
}

extern "C" int32_t gts_components_filter_i16(const int16_t* labels_in, int64_t X, int64_t Y, int64_t Z,
                                             int32_t connectivity, int64_t min_voxels, int32_t et_label,
                                             int64_t et_min_voxels, int32_t et_replacement, int16_t* labels_out,
                                             int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!labels_in || !labels_out || !stats || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!components_voxels(X, Y, Z, &n) || (connectivity != 6 && connectivity != 26)) return GTS_ERR_SHAPE;
  if (n == 0) return GTS_OK;
  if (workspace_bytes < components_bytes(n)) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(ws);
  int* parent = reinterpret_cast<int*>(ws + kHeaderBytes);
  int* roots = reinterpret_cast<int*>(ws + kHeaderBytes + round256(4 * n));
  int* sizes = reinterpret_cast<int*>(ws + kHeaderBytes + 2 * round256(4 * n));

  if (hipMemsetAsync(ws, 0, kHeaderBytes, st) != hipSuccess) return launch_status();
  const int status = components_label(labels_in, n, static_cast<int>(Y), static_cast<int>(Z), connectivity, parent,
                                      roots, sizes, st);
  if (status != GTS_OK) return status;
  components_sizes_kernel<<<blocks_for(n, int64_t{kBlock} * kSizeChunks), kBlock, 0, st>>>(roots, sizes, n);
  components_count_kernel<<<blocks_for(n, kBlock, kCountBlocks), kBlock, 0, st>>>(
      labels_in, roots, sizes, counters, n, min_voxels, et_label, et_min_voxels > 0 ? 1 : 0);
  components_apply_kernel<<<blocks_for(n, kBlock), kBlock, 0, st>>>(labels_in, labels_out, roots, sizes, counters,
                                                     reinterpret_cast<long long*>(stats), n, min_voxels, et_label,
                                                     et_min_voxels, et_replacement);
  return launch_status();
}
