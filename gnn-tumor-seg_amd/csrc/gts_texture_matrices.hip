// X4-X6: the device half of the per-lesion run-length, size-zone, dependence and neighbourhood-difference tables
// (GLRLM, GLSZM, GLDM, NGTDM; gts/texture.py).  They run after X2 of gts_texture.hip and read what it
// left: the lesions' compact voxel lists, a uint8 level per listed voxel and the level volume.  The level volume is
// defined on listed voxels only, so a neighbour's root is tested before its level is read.
//
// Definitions (index space; DIRECTIONS and the levels are X1-X3's).  The 26-neighbourhood of p is the up-to-26 voxels
// p + delta, delta in {-1, 0, 1}^3 \ {0}, inside the volume and of p's root.
//   runs     runs[l][d][g][r - 1] = the maximal sets p, p + delta_d, .. p + (r - 1) delta_d of voxels of lesion l
//            that all have level g.
//   zones    a zone is a 26-connected set of voxels of one lesion at one level (26 whatever formed the lesions); one
//            record (lesion, level, size) per zone, in arrival order: the host sorts and counts.
//   gldm     gldm[l][g][k - 1] = voxels of lesion l at level g with dependence k = 1 + the neighbours q of p with
//            |g(p) - g(q)| <= alpha.
//   ngtdm    with m(p) the size of p's neighbourhood and S(p) the sum of g(q) + 1 over it: n[l][g][m] counts the
//            voxels, s[l][g][m] sums |(g + 1) m - S(p)| over them.
//
//   X4  work units (lesion, direction, chunk), X3's.  First pass: a listed voxel whose predecessor p - delta is inside
//       the volume, of its root and at its level is no run start and stores 0; a run start walks forward to the end of
//       its run (the volume's edge at the latest) and stores the length beside the list, uint16 [13][n_listed]; the
//       longest run goes to the head by one atomic max per wave.  The host sizes the table from it.  Second pass: the
//       stored lengths are counted, those up to kRunTile in an LDS tile [levels][kRunTile] that is flushed where it is
//       not zero, longer ones (one per kRunTile voxels at most) by a global atomic each.
//   X5  a lock-free union-find in the scheme of C1-C3 over int32 parents indexed by the voxel, parent[v] <= v always.
//       init: parent[p] = the start of p's run along Z of equal root and level, at most kZoneBack voxels back (a
//       longer run is a chain of such hops: every voxel still reaches the run's first).  merge: p unites with its 12
//       backward neighbours outside its own Z line that are of its root and level.  flatten: parent[p] = its root,
//       and the root's size grows by one atomic per (wave, root).  records: every root takes a slot from a cursor.
//       Every walk and every retry is counted against a limit of n_listed steps, which a well-formed forest cannot
//       reach; one that does adds to head word 1, stops, and the host refuses the result.
//   X6  work units (lesion, chunk).  One gather of the 26 neighbours per listed voxel feeds three LDS tiles
//       [levels][27] (dependence, neighbourhood size, difference sum: below 2048 * 26 * 127 per chunk, so uint32),
//       flushed where not zero into an int64 table.
//
// Integer atomics and plain vector stores only: identical results on every run and at every grid_blocks.
#include "gts_texture.h"

namespace gts {
namespace {

constexpr int kRunTile = 64;                          // run lengths 1 .. kRunTile are counted in LDS
constexpr int kZoneBack = 63;                         // X5 init looks at most this far back along Z
constexpr int kNeighbours = GTS_TEXTURE_NEIGHBOURS;   // 26
constexpr int kColumns = kNeighbours + 1;             // dependence 1 .. 27, neighbourhood size 0 .. 26
constexpr int kMaxRun = GTS_TEXTURE_MAX_RUN;
constexpr int kRecord = GTS_TEXTURE_ZONE_RECORD_I32;
// head words of X4's and X5's int64 heads
enum { hLongest = 0, hZones = 0, hLost = 1 };

static_assert(kMaxRun == kMmMaxExtent && kMaxRun <= 65535, "a run ends at the volume's edge and fits uint16");
static_assert(kMaxLevels * kRunTile * 4 <= 48 * 1024, "the run tile leaves LDS for a second workgroup per CU");
static_assert(3 * kMaxLevels * kColumns * 4 <= 48 * 1024, "so do the three neighbourhood tiles");
static_assert(int64_t{kChunk} * kNeighbours * (kMaxLevels - 1) < (int64_t{1} << 32), "a chunk's difference sum");

__device__ __forceinline__ bool inside(int x, int y, int z, const Vol& v) {
  return x >= 0 && x < v.X && y >= 0 && y < v.Y && z >= 0 && z < v.Z;
}

// the fields of work unit w that the kernels share; false: the unit lies outside the plan and is skipped.  Uniform
// over the workgroup.
struct Unit {
  int l, root, n_levels;
  int64_t first, last;
};

__device__ __forceinline__ bool unit_of(int l, int c, const int* __restrict__ segments,
                                        const int64_t* __restrict__ plan, int L, int64_t n_listed, int G, Unit* u) {
  if (l < 0 || l >= L || c < 0) return false;
  const int64_t begin = segments[l], end = segments[l + 1], first = begin + int64_t{c} * kChunk;
  const int64_t* row = plan + int64_t{l} * kPlanRow;
  u->l = l;
  u->n_levels = static_cast<int>(row[pLevels]);
  u->root = static_cast<int>(row[pRoot]);
  u->first = first;
  u->last = first + kChunk < end ? first + kChunk : end;
  return begin >= 0 && end <= n_listed && first < end && u->n_levels >= 1 && u->n_levels <= G;
}

// ------------------------------------------------------------------ X4: runs
__global__ __launch_bounds__(kBlock) void texture_run_length_kernel(
    const int* __restrict__ roots, const int* __restrict__ work, int64_t n_work, const int* __restrict__ segments,
    const int64_t* __restrict__ plan, int L, const int* __restrict__ list, const uint8_t* __restrict__ levels,
    int64_t n_listed, const uint8_t* __restrict__ level_volume, uint16_t* __restrict__ run_length, int64_t* head,
    Vol v) {
  unsigned longest = 0;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int d = work[3 * w + 1];
    Unit u;
    if (d < 0 || d >= kDirections ||
        !unit_of(work[3 * w], work[3 * w + 2], segments, plan, L, n_listed, kMaxLevels, &u))
      continue;
    const int dx = kOffsets[d][0], dy = kOffsets[d][1], dz = kOffsets[d][2];
    const int64_t step = (int64_t{dx} * v.Y + dy) * v.Z + dz;
    for (int64_t k = u.first + threadIdx.x; k < u.last; k += kBlock) {
      const int p = list[k];
      unsigned r = 0;
      if (p >= 0 && p < v.n) {
        const auto [x, y, z] = split_xyz(p, v.Y, v.Z);
        const int g = levels[k];
        const bool follows = inside(x - dx, y - dy, z - dz, v) && roots[p - step] == u.root &&
                             level_volume[p - step] == g;
        if (!follows) {
          r = 1;
          int qx = x + dx, qy = y + dy, qz = z + dz;
          int64_t q = p + step;
          // every step leaves one plane of the volume behind: at most 4097 of them
          while (inside(qx, qy, qz, v) && roots[q] == u.root && level_volume[q] == g) {
            ++r;
            qx += dx, qy += dy, qz += dz;
            q += step;
          }
        }
      }
      run_length[int64_t{d} * n_listed + k] = static_cast<uint16_t>(r);
      longest = r > longest ? r : longest;
    }
  }
  longest = wave_reduce(longest, [](unsigned a, unsigned b) { return a > b ? a : b; });
  if ((threadIdx.x & (kWave - 1)) == 0 && longest)
    atomicMax(reinterpret_cast<u64*>(head + hLongest), static_cast<u64>(longest));
}

__global__ __launch_bounds__(kBlock) void texture_run_count_kernel(
    const int* __restrict__ work, int64_t n_work, const int* __restrict__ segments, const int64_t* __restrict__ plan,
    int L, const uint8_t* __restrict__ levels, const uint16_t* __restrict__ run_length, int64_t n_listed, int* runs,
    int G, int R) {
  __shared__ unsigned tile[kMaxLevels * kRunTile];
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int d = work[3 * w + 1];
    Unit u;
    if (d < 0 || d >= kDirections || !unit_of(work[3 * w], work[3 * w + 2], segments, plan, L, n_listed, G, &u))
      continue;
    const int cells = u.n_levels * kRunTile;
    for (int e = threadIdx.x; e < cells; e += kBlock) tile[e] = 0;
    __syncthreads();
    int* out = runs + (int64_t{u.l} * kDirections + d) * G * R;
    for (int64_t k = u.first + threadIdx.x; k < u.last; k += kBlock) {
      const int r = run_length[int64_t{d} * n_listed + k], g = levels[k];
      if (r < 1 || r > R || g >= u.n_levels) continue;  // 0: no run starts here; the rest cannot happen after X4's pass
      if (r <= kRunTile) {
        atomicAdd(&tile[g * kRunTile + r - 1], 1u);
      } else {
        atomicAdd(&out[int64_t{g} * R + r - 1], 1);
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += kBlock) {
      const int g = e / kRunTile, r = e % kRunTile;
      if (tile[e] && r < R) atomicAdd(&out[int64_t{g} * R + r], static_cast<int>(tile[e]));
    }
    __syncthreads();  // the tile is free for the next unit
  }
}

// ------------------------------------------------------------------ X5: zones
// C1-C3's reads of a parent that may change under the pass's feet (gts_components.hip)
__device__ __forceinline__ int load_parent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// C2's find with a count of its steps: a parent outside [0, v] or more than `limit` steps sets *lost and ends the walk
__device__ __forceinline__ int find_root(const int* parent, int v, int limit, bool* lost) {
  for (int s = 0; s <= limit; ++s) {
    const int p = load_parent(parent + v);
    if (p == v) return v;
    if (p < 0 || p > v) break;
    v = p;
  }
  *lost = true;
  return v;
}

// C2's unite with a count of its rounds
__device__ void unite(int* parent, int a, int b, int limit, bool* lost) {
  for (int round = 0; round <= limit; ++round) {
    a = find_root(parent, a, limit, lost);
    b = find_root(parent, b, limit, lost);
    if (*lost || a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
  *lost = true;
}

// what the four passes of X5 know of listed position k; false beyond the list or outside the plan
struct Listed {
  int l, p, root, g;
};

__device__ __forceinline__ bool listed_at(int64_t k, const int* __restrict__ segments,
                                          const int64_t* __restrict__ plan, int L, const int* __restrict__ list,
                                          const uint8_t* __restrict__ levels, int64_t n_listed, int64_t n, Listed* a) {
  if (k >= n_listed) return false;
  a->l = lesion_of(segments, L, k);
  a->p = list[k];
  a->root = static_cast<int>(plan[int64_t{a->l} * kPlanRow + pRoot]);
  a->g = levels[k];
  return a->p >= 0 && a->p < n && k < segments[a->l + 1];
}

__global__ __launch_bounds__(kBlock) void texture_zone_init_kernel(
    const int* __restrict__ roots, const int* __restrict__ segments, const int64_t* __restrict__ plan, int L,
    const int* __restrict__ list, const uint8_t* __restrict__ levels, int64_t n_listed,
    const uint8_t* __restrict__ level_volume, int* __restrict__ parent, int* __restrict__ size, Vol v) {
  for (int64_t k = int64_t{blockIdx.x} * kBlock + threadIdx.x; k < n_listed; k += int64_t{gridDim.x} * kBlock) {
    Listed a;
    if (!listed_at(k, segments, plan, L, list, levels, n_listed, v.n, &a)) continue;
    const int z = a.p % v.Z;
    int back = 0;
    while (back < kZoneBack && back < z && roots[a.p - back - 1] == a.root && level_volume[a.p - back - 1] == a.g)
      ++back;
    parent[a.p] = a.p - back;
    size[a.p] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void texture_zone_merge_kernel(
    const int* __restrict__ roots, const int* __restrict__ segments, const int64_t* __restrict__ plan, int L,
    const int* __restrict__ list, const uint8_t* __restrict__ levels, int64_t n_listed,
    const uint8_t* __restrict__ level_volume, int* parent, int64_t* head, Vol v) {
  const int limit = static_cast<int>(n_listed);
  for (int64_t k = int64_t{blockIdx.x} * kBlock + threadIdx.x; k < n_listed; k += int64_t{gridDim.x} * kBlock) {
    Listed a;
    if (!listed_at(k, segments, plan, L, list, levels, n_listed, v.n, &a)) continue;
    const auto [x, y, z] = split_xyz(a.p, v.Y, v.Z);
    bool lost = false;
    for (int d = 1; d < kDirections && !lost; ++d) {  // direction 0 is the Z line itself: joined by init
      const int dx = kOffsets[d][0], dy = kOffsets[d][1], dz = kOffsets[d][2];
      if (!inside(x - dx, y - dy, z - dz, v)) continue;
      const int q = a.p - ((dx * v.Y + dy) * v.Z + dz);
      if (roots[q] == a.root && level_volume[q] == a.g) unite(parent, a.p, q, limit, &lost);
    }
    if (lost) atomicAdd(reinterpret_cast<u64*>(head + hLost), 1ull);
  }
}

__global__ __launch_bounds__(kBlock) void texture_zone_size_kernel(
    const int* __restrict__ segments, const int64_t* __restrict__ plan, int L, const int* __restrict__ list,
    const uint8_t* __restrict__ levels, int64_t n_listed, int* parent, int* size, int64_t* head, int64_t n) {
  const int limit = static_cast<int>(n_listed);
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t base = int64_t{blockIdx.x} * kBlock; base < n_listed; base += int64_t{gridDim.x} * kBlock) {
    Listed a;
    bool on = listed_at(base + threadIdx.x, segments, plan, L, list, levels, n_listed, n, &a);
    bool lost = false;
    const int r = on ? find_root(parent, a.p, limit, &lost) : 0;
    if (lost) atomicAdd(reinterpret_cast<u64*>(head + hLost), 1ull);
    on = on && !lost;
    if (on) parent[a.p] = r;  // nothing unites any more: as C3
    wave_for_each_key(on, r, [&](int key, u64 same, bool) {
      if (lane == 0) atomicAdd(&size[key], __popcll(same));
    });
  }
}

__global__ __launch_bounds__(kBlock) void texture_zone_record_kernel(
    const int* __restrict__ segments, const int64_t* __restrict__ plan, int L, const int* __restrict__ list,
    const uint8_t* __restrict__ levels, int64_t n_listed, const int* __restrict__ parent,
    const int* __restrict__ size, int* __restrict__ records, int64_t* head, int64_t n) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t base = int64_t{blockIdx.x} * kBlock; base < n_listed; base += int64_t{gridDim.x} * kBlock) {
    Listed a;
    const bool on = listed_at(base + threadIdx.x, segments, plan, L, list, levels, n_listed, n, &a);
    const bool is_root = on && parent[a.p] == a.p;
    const u64 heads = __ballot(is_root);
    u64 at = 0;
    if (lane == 0 && heads) at = atomicAdd(reinterpret_cast<u64*>(head + hZones), static_cast<u64>(__popcll(heads)));
    at = __shfl(at, 0, kWave) + static_cast<u64>(__popcll(heads & ((u64{1} << lane) - 1)));
    if (is_root && at < static_cast<u64>(n_listed)) {  // there are no more zones than listed voxels
      int* rec = records + at * kRecord;
      rec[0] = a.l;
      rec[1] = a.g;
      rec[2] = size[a.p];
    }
  }
}

// ------------------------------------------------------------------ X6: the 26-neighbourhood
__global__ __launch_bounds__(kBlock) void texture_neighbourhood_kernel(
    const int* __restrict__ roots, const int* __restrict__ work, int64_t n_work, const int* __restrict__ segments,
    const int64_t* __restrict__ plan, int L, const int* __restrict__ list, const uint8_t* __restrict__ levels,
    int64_t n_listed, const uint8_t* __restrict__ level_volume, int alpha, int64_t* table, int G, Vol v) {
  __shared__ unsigned tile[3 * kMaxLevels * kColumns];
  const int64_t family = int64_t{L} * G * kColumns;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    Unit u;
    if (!unit_of(work[2 * w], work[2 * w + 1], segments, plan, L, n_listed, G, &u)) continue;
    const int cells = u.n_levels * kColumns;
    for (int e = threadIdx.x; e < 3 * cells; e += kBlock) tile[e] = 0;
    __syncthreads();
    for (int64_t k = u.first + threadIdx.x; k < u.last; k += kBlock) {
      const int p = list[k], g = levels[k];
      if (p < 0 || p >= v.n || g >= u.n_levels) continue;
      const auto [x, y, z] = split_xyz(p, v.Y, v.Z);
      int m = 0, sum = 0, alike = 0;
      for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dz = -1; dz <= 1; ++dz) {
            if ((dx == 0 && dy == 0 && dz == 0) || !inside(x + dx, y + dy, z + dz, v)) continue;
            const int64_t q = p + (int64_t{dx} * v.Y + dy) * v.Z + dz;
            if (roots[q] != u.root) continue;  // the same root, not merely the same mask
            const int gq = level_volume[q];
            ++m;
            sum += gq + 1;
            alike += (g > gq ? g - gq : gq - g) <= alpha;
          }
      const int gap = (g + 1) * m - sum;
      atomicAdd(&tile[g * kColumns + alike], 1u);
      atomicAdd(&tile[cells + g * kColumns + m], 1u);
      if (gap) atomicAdd(&tile[2 * cells + g * kColumns + m], static_cast<unsigned>(gap < 0 ? -gap : gap));
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * cells; e += kBlock)
      if (tile[e])
        atomicAdd(reinterpret_cast<u64*>(table + (e / cells) * family + int64_t{u.l} * G * kColumns + e % cells),
                  static_cast<u64>(tile[e]));
    __syncthreads();  // the tiles are free for the next unit
  }
}

// ------------------------------------------------------------------ host
// int32 words of runs [L][13][G][R]; 0 outside the limits or above the byte cap
inline int64_t run_words(int64_t lesions, int64_t levels, int64_t longest) {
  if (lesions < 1 || lesions > INT32_MAX || levels < 1 || levels > kMaxLevels || longest < 1 || longest > kMaxRun)
    return 0;
  const int64_t words = lesions * kDirections * levels * longest;  // < 2^31 * 13 * 128 * 4097 < 2^63
  return 4 * words <= int64_t{GTS_TEXTURE_MAX_TABLE_BYTES} ? words : 0;
}

// int64 entries of gldm, ngtdm_n, ngtdm_s, each [L][G][27]
inline int64_t neighbourhood_i64s(int64_t lesions, int64_t levels) {
  if (lesions < 1 || lesions > INT32_MAX || levels < 1 || levels > kMaxLevels) return 0;
  const int64_t entries = 3 * lesions * levels * kColumns;
  return 8 * entries <= int64_t{GTS_TEXTURE_MAX_TABLE_BYTES} ? entries : 0;
}

inline bool lists_ok(int64_t n, int64_t lesions, int64_t n_listed) {
  return lesions >= 1 && lesions <= n && n_listed >= 1 && n_listed <= n;
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_texture_run_words(int64_t lesions, int64_t max_levels, int64_t longest) {
  return gts::run_words(lesions, max_levels, longest);
}

extern "C" int64_t gts_texture_neighbourhood_i64s(int64_t lesions, int64_t max_levels) {
  return gts::neighbourhood_i64s(lesions, max_levels);
}

extern "C" int32_t gts_texture_run_lengths(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, const int32_t* work,
                                           int64_t n_work, const int32_t* segments, const int64_t* plan,
                                           int64_t lesions, const int32_t* list, const uint8_t* levels,
                                           int64_t n_listed, uint16_t* run_length, int64_t run_length_words,
                                           int64_t* head, const void* workspace, int64_t workspace_bytes,
                                           int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !work || !segments || !plan || !list || !levels || !run_length || !head || !workspace)
    return GTS_ERR_NULL;
  int64_t n;
  if (!texture_voxels(X, Y, Z, &n) || !lists_ok(n, lesions, n_listed) || n_work < 1 || n_work > INT32_MAX)
    return GTS_ERR_SHAPE;
  if (!grid_ok(grid_blocks)) return GTS_ERR_SHAPE;
  if (workspace_bytes < texture_bytes(n) || run_length_words < kDirections * n_listed) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TextureBuffers b = texture_buffers(const_cast<void*>(workspace), n);
  const Vol v = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), n};
  if (hipMemsetAsync(head, 0, 8 * kHead, st) != hipSuccess) return launch_status();
  texture_run_length_kernel<<<grid_for(n_work, 1, grid_blocks), kBlock, 0, st>>>(
      roots, work, n_work, segments, plan, static_cast<int>(lesions), list, levels, n_listed, b.level_volume,
      run_length, head, v);
  return launch_status();
}

extern "C" int32_t gts_texture_runs(const int32_t* work, int64_t n_work, const int32_t* segments, const int64_t* plan,
                                    int64_t lesions, const uint8_t* levels, const uint16_t* run_length,
                                    int64_t n_listed, int32_t* table, int64_t table_words, int64_t max_levels,
                                    int64_t longest, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!work || !segments || !plan || !levels || !run_length || !table) return GTS_ERR_NULL;
  if (lesions < 1 || lesions > INT32_MAX || n_listed < 1 || n_listed > INT32_MAX || n_work < 1 ||
      n_work > INT32_MAX || max_levels < 1 || max_levels > kMaxLevels || longest < 1 || longest > kMaxRun)
    return GTS_ERR_SHAPE;
  if (!grid_ok(grid_blocks)) return GTS_ERR_SHAPE;
  const int64_t words = run_words(lesions, max_levels, longest);
  if (words == 0 || table_words < words) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(table, 0, 4 * words, st) != hipSuccess) return launch_status();
  texture_run_count_kernel<<<grid_for(n_work, 1, grid_blocks), kBlock, 0, st>>>(
      work, n_work, segments, plan, static_cast<int>(lesions), levels, run_length, n_listed, table,
      static_cast<int>(max_levels), static_cast<int>(longest));
  return launch_status();
}

extern "C" int32_t gts_texture_zones(const int32_t* roots, int64_t X, int64_t Y, int64_t Z, const int32_t* segments,
                                     const int64_t* plan, int64_t lesions, const int32_t* list, const uint8_t* levels,
                                     int64_t n_listed, int32_t* scratch, int64_t scratch_words, int32_t* records,
                                     int64_t records_words, int64_t* head, const void* workspace,
                                     int64_t workspace_bytes, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !segments || !plan || !list || !levels || !scratch || !records || !head || !workspace)
    return GTS_ERR_NULL;
  int64_t n;
  if (!texture_voxels(X, Y, Z, &n) || !lists_ok(n, lesions, n_listed)) return GTS_ERR_SHAPE;
  if (!grid_ok(grid_blocks)) return GTS_ERR_SHAPE;
  if (workspace_bytes < texture_bytes(n) || scratch_words < 2 * n || records_words < kRecord * n_listed)
    return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TextureBuffers b = texture_buffers(const_cast<void*>(workspace), n);
  const Vol v = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), n};
  const int L = static_cast<int>(lesions);
  int *parent = scratch, *size = scratch + n;
  if (hipMemsetAsync(head, 0, 8 * kHead, st) != hipSuccess) return launch_status();
  const int grid = grid_for(n_listed, kBlock, grid_blocks);
  texture_zone_init_kernel<<<grid, kBlock, 0, st>>>(roots, segments, plan, L, list, levels, n_listed, b.level_volume,
                                                    parent, size, v);
  texture_zone_merge_kernel<<<grid, kBlock, 0, st>>>(roots, segments, plan, L, list, levels, n_listed, b.level_volume,
                                                     parent, head, v);
  texture_zone_size_kernel<<<grid, kBlock, 0, st>>>(segments, plan, L, list, levels, n_listed, parent, size, head, n);
  texture_zone_record_kernel<<<grid, kBlock, 0, st>>>(segments, plan, L, list, levels, n_listed, parent, size, records,
                                                      head, n);
  return launch_status();
}

extern "C" int32_t gts_texture_neighbourhood(const int32_t* roots, int64_t X, int64_t Y, int64_t Z,
                                             const int32_t* work, int64_t n_work, const int32_t* segments,
                                             const int64_t* plan, int64_t lesions, const int32_t* list,
                                             const uint8_t* levels, int64_t n_listed, int32_t alpha, int64_t* table,
                                             int64_t table_i64s, int64_t max_levels, const void* workspace,
                                             int64_t workspace_bytes, int64_t grid_blocks, void* stream) {
  using namespace gts;
  if (!roots || !work || !segments || !plan || !list || !levels || !table || !workspace) return GTS_ERR_NULL;
  int64_t n;
  if (!texture_voxels(X, Y, Z, &n) || !lists_ok(n, lesions, n_listed) || n_work < 1 || n_work > INT32_MAX)
    return GTS_ERR_SHAPE;
  if (alpha < 0) return GTS_ERR_ARGKIND;
  if (!grid_ok(grid_blocks)) return GTS_ERR_SHAPE;
  const int64_t entries = neighbourhood_i64s(lesions, max_levels);
  if (workspace_bytes < texture_bytes(n) || entries == 0 || table_i64s < entries) return GTS_ERR_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TextureBuffers b = texture_buffers(const_cast<void*>(workspace), n);
  const Vol v = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z), n};
  if (hipMemsetAsync(table, 0, 8 * entries, st) != hipSuccess) return launch_status();
  texture_neighbourhood_kernel<<<grid_for(n_work, 1, grid_blocks), kBlock, 0, st>>>(
      roots, work, n_work, segments, plan, static_cast<int>(lesions), list, levels, n_listed, b.level_volume, alpha,
      table, static_cast<int>(max_levels), v);
  return launch_status();
}
