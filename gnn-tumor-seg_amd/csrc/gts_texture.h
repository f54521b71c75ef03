// What the two texture sources share (X1-X3, gts_texture.hip; X4-X6, gts_texture_matrices.hip): the constants of
// include/gts_hip.h under their short names, the plan's fields, the 13 directions, the workspace's layout and the
// lesion of a listed position.  Included by those two sources only, each of which gets its own copy.
#pragma once
#include "gts_lesions.h"
#include "gts_scan.h"

namespace gts {
namespace {

constexpr int kHead = GTS_TEXTURE_HEAD_I64;
constexpr int kCountRow = GTS_TEXTURE_COUNT_ROW_I64;
constexpr int kRangeRow = GTS_TEXTURE_RANGE_ROW_I64;
constexpr int kPlanRow = GTS_TEXTURE_PLAN_I64;
constexpr int kMaxLevels = GTS_TEXTURE_MAX_LEVELS;
constexpr int kChunk = GTS_TEXTURE_CHUNK;
constexpr int kDirections = GTS_TEXTURE_DIRECTIONS;
typedef unsigned long long u64;

static_assert(kChunk % kBlock == 0, "a chunk is a whole number of passes of the workgroup");
static_assert(kMaxLevels <= 256, "a level is stored as uint8");

// plan row fields
enum { pLo = 0, pHi = 1, pLevels = 2, pRoot = 3 };

__constant__ int kOffsets[kDirections][3] = {{0, 0, 1},  {0, 1, -1}, {0, 1, 0},  {0, 1, 1}, {1, -1, -1},
                                             {1, -1, 0}, {1, -1, 1}, {1, 0, -1}, {1, 0, 0}, {1, 0, 1},
                                             {1, 1, -1}, {1, 1, 0},  {1, 1, 1}};

struct Vol {
  int X, Y, Z;
  int64_t n;
};

// the lesion of listed position k: the last l with segments[l] <= k
__device__ __forceinline__ int lesion_of(const int* __restrict__ segments, int L, int64_t k) {
  int lo = 0, hi = L - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (segments[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

inline bool texture_voxels(int64_t X, int64_t Y, int64_t Z, int64_t* n) {
  return volume_voxels(X, Y, Z, false, n) && X <= kMmMaxExtent && Y <= kMmMaxExtent && Z <= kMmMaxExtent;
}

// header | slot int32[n] | level volume uint8[n]
inline int64_t texture_bytes(int64_t n) { return kHeaderBytes + round256(4 * n) + round256(n); }

struct TextureBuffers {
  int* slot;
  uint8_t* level_volume;
};

inline TextureBuffers texture_buffers(void* workspace, int64_t n) {
  char* ws = static_cast<char*>(workspace) + kHeaderBytes;
  return {reinterpret_cast<int*>(ws), reinterpret_cast<uint8_t*>(ws + round256(4 * n))};
}

}  // namespace
}  // namespace gts
