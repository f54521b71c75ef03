// Pieces the clustered kernels share (gts_spmm_cluster.hip: K1 / K2 at F = 256; gts_gat_cluster.hip: the GATConv
// aggregation over the same schedule records): record layout, LDS-DMA gathers, counted waits, count-specialised loops,
// the per-XCD unit dealer and the persistent launch.
#pragma once
#include <algorithm>

#include "gts_rows.h"

namespace gts {
namespace {

constexpr int kF = 256;          // feature width the clustered kernels are built for
constexpr int kHalfBytes = 512;  // one column half of a row
constexpr int kArgHalfBytes = 128;
constexpr unsigned kRsrcFlags = 0x00020000;
constexpr int kRecRegs = 8;      // a record is at most 64 * kRecRegs words
constexpr int kMaxRing = 6;

__host__ __device__ inline int pad4(int words) { return (words + 3) & ~3; }

// Word offsets inside one schedule record (all sections padded to 16 bytes):
//   [0..3] n_rows, n_srcs, n_edges, 0 | row ids | neighbour ids (tail repeats the last) | per row: first 8-edge
//   chunk (low 16 bits) and degree (high 16 bits) | uint8 per edge: neighbour's position, every row's edges padded
//   to whole 8-byte chunks (pads repeat the row's last edge) | uint8 per edge: tag, same shape (K2 only)
struct RecLayout {
  int rows, srcs, eoff, loc, tag, words;
};
__host__ __device__ inline RecLayout rec_layout(int max_rows, int max_srcs, int loc_words, bool tag) {
  RecLayout r;
  r.rows = 4;
  r.srcs = r.rows + pad4(max_rows);
  r.eoff = r.srcs + pad4(max_srcs);
  r.loc = r.eoff + pad4(max_rows);
  r.tag = r.loc + loc_words;
  r.words = r.tag + (tag ? loc_words : 0);
  return r;
}


__device__ __forceinline__ void barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// wait until at most n of this wave's vector-memory operations (the youngest) are outstanding
#define GTS_VMCNT_CASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
__device__ __forceinline__ void wait_vm_all_but(int n) {
  switch (n) {
    GTS_VMCNT_CASE(1) GTS_VMCNT_CASE(2) GTS_VMCNT_CASE(3) GTS_VMCNT_CASE(4) GTS_VMCNT_CASE(5) GTS_VMCNT_CASE(6)
    GTS_VMCNT_CASE(7) GTS_VMCNT_CASE(8) GTS_VMCNT_CASE(9) GTS_VMCNT_CASE(10) GTS_VMCNT_CASE(11) GTS_VMCNT_CASE(12)
    GTS_VMCNT_CASE(13) GTS_VMCNT_CASE(14) GTS_VMCNT_CASE(15) GTS_VMCNT_CASE(16) GTS_VMCNT_CASE(17) GTS_VMCNT_CASE(18)
    GTS_VMCNT_CASE(19) GTS_VMCNT_CASE(20) GTS_VMCNT_CASE(21) GTS_VMCNT_CASE(22) GTS_VMCNT_CASE(23) GTS_VMCNT_CASE(24)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;   // waiting for more is always correct
  }
}
__device__ __forceinline__ void barrier_all() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }


// `cnt` (1..8, wave-uniform) as a compile-time constant: straight-line code for the exact edge count of a chunk
template <typename Body>
__device__ __forceinline__ void for_count(int cnt, Body&& body) {
  switch (cnt) {
    case 1: body(IC<1>{}); break;
    case 2: body(IC<2>{}); break;
    case 3: body(IC<3>{}); break;
    case 4: body(IC<4>{}); break;
    case 5: body(IC<5>{}); break;
    case 6: body(IC<6>{}); break;
    case 7: body(IC<7>{}); break;
    default: body(IC<8>{}); break;
  }
}
__device__ __forceinline__ unsigned chunk_byte(const uint2& w, int q) { return ((q < 4 ? w.x : w.y) >> (8 * (q & 3))) & 0xFF; }


// ---- gathers (LDS-DMA) ---------------------------------------------------------------------------------------
// Two ways to issue `buffer_load_dwordx4 ... lds` (64 lanes x 16 B from per-lane byte offsets into one contiguous
// KiB of LDS):
//   * BuiltinDma: the clang builtin.  hipcc's wait-count pass then treats the transfer as a pending LDS write and
//     puts `s_waitcnt vmcnt(0)` in front of every later LDS read it cannot tell apart from it — right for the forms
//     that gather, wait, and only then read;
//   * RawDma: the same instruction as inline assembly, for the streaming form, which reads one image while the
//     gathers into the OTHER image are in flight and orders the two itself (counted vmcnt + workgroup barrier).
typedef int v4i __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) unsigned char* LdsBytes;

struct BuiltinDma {
  __amdgpu_buffer_rsrc_t rsrc;
  __device__ __forceinline__ BuiltinDma(const void* base, unsigned bytes)
      : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, kRsrcFlags)) {}
  __device__ __forceinline__ void operator()(unsigned char* lds_dst, unsigned voff) const {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, reinterpret_cast<float*>(lds_dst), 16, voff, 0, 0, 0);
  }
};
struct RawDma {
  v4i rsrc;   // buffer resource words: base[31:0] | base[47:32] (stride 0) | bytes | flags
  __device__ __forceinline__ RawDma(const void* base, unsigned bytes) {
    const unsigned long long b = reinterpret_cast<unsigned long long>(base);
    rsrc = v4i{static_cast<int>(b), static_cast<int>((b >> 32) & 0xFFFF), static_cast<int>(bytes), static_cast<int>(kRsrcFlags)};
  }
  __device__ __forceinline__ void operator()(unsigned char* lds_dst, unsigned voff) const {
    const unsigned at = static_cast<unsigned>(reinterpret_cast<uintptr_t>((LdsBytes)lds_dst));   // wave-uniform
    unsigned keep;   // M0 holds the LDS destination; it is handed back as found
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(at), "v"(voff), "s"(rsrc) : "memory");
  }
};

// One column half of n_srcs neighbour rows -> image [n_srcs][512 B].  `src_of(i)` gives this lane's neighbour id
// for the pair of rows (i, i + 1): lanes 0-31 fetch row i, lanes 32-63 row i + 1 (the record repeats the last id
// after the end, and the host reserves an even number of image rows).  `first`, `step` in rows (even).
template <typename Dma, typename SrcOf>
__device__ __forceinline__ void gather_halves(const Dma& dma, int part, unsigned char* image, int n_srcs,
                                              int first, int step, SrcOf&& src_of) {
  const int hl = threadIdx.x & 31;
  for (int i = first; i < n_srcs; i += step) {
    const unsigned voff = static_cast<unsigned>(src_of(i)) * (kF * 4u) + static_cast<unsigned>(part) * kHalfBytes + hl * 16u;
    dma(image + i * kHalfBytes, voff);
  }
}

// ---- units dealt per XCD ---------------------------------------------------------------------------------------
// A persistent launch has gridDim.x = 8 * per_xcd workgroups; those with blockIdx % 8 == x (one XCD under round-robin placement:
// speed only) share the x-th eighth of the clusters, [clo, clo + span), and walk its units in an order the kernel chooses so that
// consecutive units are the same column slice of neighbouring clusters, whose halo rows meet in the XCD's L2.
//
// STATIC dealing: unit i of the walk goes to workgroup i % per_xcd.  A workgroup that falls ONE unit behind its neighbours is then
// per_xcd units behind them in the walk — a whole generation — and the halo rows it shares with them have left the L2 before it
// asks (1.57 x the table fetched where the walk in step fetches 1.20 x, profiles/r04/gat_l2_replay.log).
// DYNAMIC dealing: the XCD's workgroups draw the walk's next index off ONE counter, so the units in flight are always the latest
// per_xcd of the walk whatever each workgroup's pace.  Which workgroup computes a unit changes nothing in what it computes.
//   * The counters: kCounterStride words per XCD (a line of its own each): word 0 = units drawn, word kCounterDone = workgroups
//     finished.  Zero at launch; K1 / K2 leave them zero (their XCD's last workgroup resets them), the GAT passes zero them in the
//     pass in front.
//   * The dealer is the workgroup's LAST wave (it fetches no record piece).  It draws by an agent-scope atomic add (take) and hands
//     the drawn index to the other waves through kDealBytes of LDS, `l_deal` (publish): eight slots, whose contents the kernel's
//     `Fill` writes (K1 / K2: the raw index, which every wave decodes; GAT: the decoded (cluster, sub) pair).  An index past the walk's end
//     yields "no unit"; units come in walk order, so nothing follows an empty slot.
//   * A pipeline of PIPE units (fetching a record ... being reduced) is filled by ONE add of PIPE in the prologue: PIPE - 1 indices
//     into slots 0 .. PIPE - 2 for the prologue, the last into slot 6 for iteration 0.  One round trip, then a barrier.
//   * In the loop, iteration `it` reads slot 6 + (it & 1) behind its barrier.  The dealer issues the add for iteration it + 1 in
//     iteration `it` (take_next) and publishes it at the TOP of iteration it + 1 (publish_next), behind the wait every wave makes
//     there anyway and in front of that iteration's barrier: it never waits for the counter's round trip on its own, and the slot
//     it writes was last read two barriers ago.
constexpr int kCounterStride = 32;                           // words from one XCD's counters to the next
constexpr int kCounterDone = 16;                             // the XCD's count of finished workgroups, words behind its unit counter
constexpr int64_t kCounterBytes = 8 * kCounterStride * 4;
static_assert(kCounterBytes == 4 * GTS_CLUSTER_COUNTER_WORDS, "include/gts_hip.h promises callers this size");
static_assert(kCounterBytes == 4 * kBlock, "the GAT weight passes zero the counters with one workgroup, a word per thread");
constexpr int kDealBytes = 64;                               // l_deal, at the end of a workgroup's LDS
constexpr int kDealLoopSlot = 6;

struct XcdShare {
  int xcd, j, per_xcd;   // this workgroup is the XCD's j-th of per_xcd
};
__device__ __forceinline__ XcdShare xcd_share() { return XcdShare{static_cast<int>(blockIdx.x & 7), static_cast<int>(blockIdx.x >> 3), static_cast<int>(gridDim.x >> 3)}; }
struct XcdSpan {
  int clo, span;         // the XCD's clusters: [clo, clo + span)
};
__device__ __forceinline__ XcdSpan xcd_span(int n_clusters, int xcd) {
  XcdSpan s;
  s.clo = static_cast<int>(static_cast<long long>(n_clusters) * xcd / 8);
  s.span = static_cast<int>(static_cast<long long>(n_clusters) * (xcd + 1) / 8) - s.clo;
  return s;
}

__device__ __forceinline__ int deal_loop_slot(int it) { return kDealLoopSlot + (it & 1); }   // the slot iteration `it` reads

// PIPE: units in the kernel's pipeline.  fill(first, count, slot0): the kernel's way to write the walk's indices first .. first +
// count - 1 (held by lane 0) into l_deal's slots slot0 ..; called by every lane of the dealing wave.
template <int PIPE, typename Fill>
struct UnitDealer {
  unsigned* const& counters;   // the kernel argument itself, re-read where used (a copy held in registers cost the GAT kernels two)
  int xcd;
  int wave, n_waves;           // of this workgroup: its last wave deals
  Fill fill;
  unsigned taken;              // the add of the iteration before, not yet published (lane 0)

  __device__ __forceinline__ bool dealing() const { return wave == n_waves - 1; }
  __device__ __forceinline__ unsigned* counter() const { return counters + kCounterStride * xcd; }   // this XCD's unit counter
  __device__ __forceinline__ unsigned take(int count) const {
    unsigned base = 0;
    if ((threadIdx.x & (kWave - 1)) == 0)
      base = __hip_atomic_fetch_add(counter(), static_cast<unsigned>(count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return base;
  }
  __device__ __forceinline__ void prologue() {
    if (dealing()) {
      const unsigned first = take(PIPE);
      fill(first, PIPE - 1, 0);
      fill(first + (PIPE - 1), 1, kDealLoopSlot);
    }
    barrier_all();
  }
  __device__ __forceinline__ void publish_next(int it) const {   // top of iteration `it`, in front of its barrier
    if (it > 0 && dealing()) fill(taken, 1, deal_loop_slot(it));
  }
  __device__ __forceinline__ void take_next() {                  // inside iteration `it`: the unit iteration it + 1 enters
    if (dealing()) taken = take(1);
  }
};
template <int PIPE, typename Fill>
__device__ __forceinline__ UnitDealer<PIPE, Fill> unit_dealer(unsigned* const& counters, int xcd, int wave, int n_waves, Fill fill) {
  return UnitDealer<PIPE, Fill>{counters, xcd, wave, n_waves, fill, 0u};
}

constexpr int64_t kMaxLds = 160 * 1024;

inline int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return cus;
}

// workgroups of a persistent launch: per_cu on every CU, no more than there are units, a multiple of 8 (one share per XCD), at least 8
inline int64_t persistent_grid(int per_cu, int64_t units) {
  const int64_t grid = static_cast<int64_t>(device_cus()) * per_cu;
  return std::max<int64_t>(8, std::min(grid, (units + 7) / 8 * 8)) / 8 * 8;
}

template <typename Kernel>
inline void allow_big_lds(Kernel k) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kMaxLds));
}

// one persistent streaming kernel on `grid` workgroups of `waves` waves; its LDS attribute is set once per kernel, not per launch
template <auto Kernel, typename Args>
inline int launch_persistent(const Args& a, int64_t grid, int waves, int64_t wg_lds, hipStream_t st) {
  static const bool once = (allow_big_lds(Kernel), true);
  (void)once;
  Kernel<<<dim3(static_cast<unsigned>(grid)), waves * kWave, wg_lds, st>>>(a);
  return launch_status();
}

}  // namespace
}  // namespace gts
