// The persistent clustered K1 / K2 kernel WITH ITS TIMING ARMS, kept out of libgts_hip.so: cut as it stood at commit 9c71b5b ("Pin
// clustered K1/K2 and GAT kernels on hand-made cluster schedules") out of gnn-tumor-seg_amd/csrc/gts_spmm_cluster.hip, where every
// arm below sat inside the product kernel behind a WHATIF template parameter:
//   1 = no row gathers, 2 = no reduction and no stores, 3 = no stores (K1), 4 = stores without the reduction (K1),
//   9 = shader-clock stamps of wave 0 around the phases of an iteration, written over `arg`.
// A frozen experiment (logs: profiles/r04/cluster_whatif.log, profiles/r03_cluster_whatif.log): it carries its own copy of the unit
// dealing as it was then and need not follow the product kernel.  Include it BEHIND gts_spmm_cluster.hip (whose ClusterArgs, LdsPlan,
// cluster_geometry, reduce_winner_rows and gather helpers it uses), as tools/diag/cluster_whatif.hip does.
// Adapted in three places, otherwise the text of that commit: the names (whatif_reduce_max_rows, spmm_cluster_whatif_kernel,
// launch_cluster_whatif); an unused local of the launcher dropped; and, since cluster_geometry lost its `whatif` argument, the launcher
// holds the global g_cluster_ring at 1 around that call for the timing arms (single-threaded diagnostic use only).

namespace gts {
namespace {

// ---- reduce the rows of one unit out of its LDS slot ------------------------------------------------------
// `first` / `step`: this wave's share of the unit's row pairs (lanes 0-31 one row, lanes 32-63 the next).  Per
// 8-edge chunk: one 8-byte read gives the chunk's neighbour positions, then CNT 16-byte reads and 3 CNT vector
// operations per column — straight-line code for the exact count the longer of the wave's two rows needs (CNT is
// wave-uniform).  The pads of a row's last chunk repeat its last edge: a repeated value never beats the maximum
// it already is (strict '<'), so the shorter row needs no mask in K1; K2 masks by the degree.
template <int ARGB, int WHATIF = 0>   // WHATIF (tools/diag only): 3 = no stores, 4 = stores without the reduction
__device__ __forceinline__ int whatif_reduce_max_rows(const ClusterArgs& a, const int32_t* l_rec, const unsigned char* image,
                                               int part, int first, int step) {
  const int lane = threadIdx.x & (kWave - 1), half = lane >> 5, hl = lane & 31;
  const int n_rows = l_rec[0];
  const uint32_t* info = reinterpret_cast<const uint32_t*>(l_rec + a.layout.eoff);
  const uint2* loc = reinterpret_cast<const uint2*>(l_rec + a.layout.loc);
  const unsigned char* mine = image + hl * 16;
  int trips = 0;
  for (int j0 = 2 * first; j0 < n_rows; j0 += 2 * step, ++trips) {   // j0 is wave-uniform: the even row of the pair
    const int j = j0 + half;
    const bool have = j < n_rows;
    const uint32_t ri = have ? info[j] : 0u;
    const int c0 = ri & 0xFFFF, deg = ri >> 16;
    const int deg_w = max(__builtin_amdgcn_readlane(deg, 0), __builtin_amdgcn_readlane(deg, 32));
    float best[4];
    int slot[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) best[t] = -INFINITY, slot[t] = -1;
    for (int c = 0; 8 * c < deg_w && WHATIF != 4; ++c) {
      const bool mine_too = 8 * c < deg;                     // the shorter row of the pair may have run out of chunks
      const uint2 w = loc[mine_too ? c0 + c : c0];
      for_count(min(8, deg_w - 8 * c), [&](auto cnt_c) {
        constexpr int CNT = decltype(cnt_c)::value;
        // at most six of a chunk's rows in registers at a time (a seventh and eighth follow): 24 instead of 32 value registers at this
        // kernel's cap of 64, which the form that deals its units needs for its own state
        constexpr int FIRST = CNT > 6 ? 6 : CNT;
        float4 val[FIRST];
#pragma unroll
        for (int q = 0; q < FIRST; ++q) val[q] = *reinterpret_cast<const float4*>(mine + chunk_byte(w, q) * kHalfBytes);
#pragma unroll
        for (int q = 0; q < FIRST; ++q) {
          const float v4[4] = {val[q].x, val[q].y, val[q].z, val[q].w};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const bool up = mine_too && best[t] < v4[t];
            best[t] = up ? v4[t] : best[t];
            slot[t] = up ? 8 * c + q : slot[t];
          }
        }
        if constexpr (CNT > FIRST) {
          float4 rest[CNT - FIRST];
#pragma unroll
          for (int q = FIRST; q < CNT; ++q) rest[q - FIRST] = *reinterpret_cast<const float4*>(mine + chunk_byte(w, q) * kHalfBytes);
#pragma unroll
          for (int q = FIRST; q < CNT; ++q) {
            const float v4[4] = {rest[q - FIRST].x, rest[q - FIRST].y, rest[q - FIRST].z, rest[q - FIRST].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const bool up = mine_too && best[t] < v4[t];
              best[t] = up ? v4[t] : best[t];
              slot[t] = up ? 8 * c + q : slot[t];
            }
          }
        }
      });
    }
    Vec<4> o;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bool dead = isinf(best[t]);   // same rules as spmm_max_fwd_kernel (gts_spmm.hip)
      o.v[t] = dead ? 0.0f : best[t];
      slot[t] = (dead || (a.relu_input && !(best[t] > 0.0f))) ? -1 : slot[t];
    }
    if (WHATIF == 3) {
      if (o.v[0] == 123.456f) a.out[0] = static_cast<float>(slot[0] + slot[1] + slot[2] + slot[3]) + o.v[1] + o.v[2] + o.v[3];
    } else if (have) {
      const size_t off = static_cast<size_t>(l_rec[a.layout.rows + j]) * kF + part * (kF / 2) + hl * 4;
      if (a.nt & 1) o.store_nt(a.out + off); else o.store(a.out + off);
      if constexpr (ARGB == 1) {
        const uint32_t w = (slot[0] & 0xFF) | ((slot[1] & 0xFF) << 8) | ((slot[2] & 0xFF) << 16) |
                           (static_cast<uint32_t>(slot[3] & 0xFF) << 24);
        *reinterpret_cast<uint32_t*>(a.arg + off) = w;
      }
    }
  }
  return trips * (ARGB == 1 ? 2 : 1);   // vector-memory instructions this wave has just issued
}

// ---- the persistent streaming kernel --------------------------------------------------------------------------
// gridDim.x is a multiple of 8: the workgroups with blockIdx % 8 == x (one XCD under round-robin placement; speed
// only) share the x-th eighth of the units and take them round-robin.  LDS: three record slots, two images.
// WHATIF != 0 only in the timing experiments of tools/diag (wrong results): 1 = no row gathers, 2 = no reduction and
// no stores, 3 = no stores, 4 = stores without the reduction (K1).
template <bool BWD, int ARGB, int WHATIF = 0, int DEPTH = 1, bool DEAL = false>   // DEAL: units dealt off the XCD's counter (a.counters)
// Two workgroups per CU: 16 waves each for K1 (<= 64 registers), 12 for K2 (its 68 registers: 6 waves per SIMD).  With 8 waves
// the reduction of a unit is latency-bound (lattice, 8 graphs: 67.6 / 72.2 us against 63.9 / 67.8; k-NN graphs of mean
// degree 7 - 10: 78 - 144 us against 65 - 96, profiles/r03_cluster_other_graphs.log).
__global__ __launch_bounds__(1024, BWD ? 6 : 8) void spmm_cluster_whatif_kernel(const ClusterArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int n_waves = blockDim.x / kWave;
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
  const long long n_units = 2LL * a.n_clusters;
  const int lo = static_cast<int>(n_units * xcd / 8), hi = static_cast<int>(n_units * (xcd + 1) / 8);
  // Dealing (as in gat_cluster_stream_kernel, see there).  STATIC (a.counters == nullptr): unit lo + j + t * per_xcd is this workgroup's
  // t-th.  DYNAMIC (the default): the XCD's workgroups take their units off one counter, in the order "every cluster of the XCD's span for
  // the left half, then for the right half" — the units in flight stay neighbours in that walk whatever each workgroup's pace, and their
  // halo rows meet in the XCD's L2 (a workgroup one unit behind under static dealing is per_xcd units behind in the walk).
  constexpr bool dynamic = DEAL;           // a compile-time choice: as a run-time one it cost both forms spilled registers
  const int n_static = lo + j < hi ? (hi - lo - j + per_xcd - 1) / per_xcd : 0;   // units lo + j + t * per_xcd, t < n_static
  if (!dynamic && n_static == 0) return;
  const int clo = static_cast<int>(static_cast<long long>(a.n_clusters) * xcd / 8);
  const int span = static_cast<int>(static_cast<long long>(a.n_clusters) * (xcd + 1) / 8) - clo;
  const int words = a.layout.words;
  const int pieces = (words + 255) / 256;   // a record arrives as one or two whole 1 KiB LDS-DMA pieces (lanes past its end deliver zeros)
  const int rec_bytes = 1024 * pieces, image_bytes = a.slot_bytes - a.image_off;
  // gathers run `depth` units ahead of the reduction: depth + 1 images, depth + 2 record slots (the record of the unit whose
  // gathers are issued next is fetched one iteration before that)
  // (DEPTH is a template constant: with run-time slot counts the K1 form spills a register and both forms lose 8 - 10 %)
  constexpr int depth = DEPTH, n_images = DEPTH + 1, n_recs = DEPTH + 2;
  unsigned char* images = lds + n_recs * rec_bytes;
  const RawDma rr(a.rec, static_cast<unsigned>(a.n_clusters) * words * 4u);
  const RawDma rt(a.table, a.table_bytes);
  const RawDma rw(a.winners, BWD ? a.winners_bytes : 0);
  // units in the pipeline (2 * cluster + column half; < 0: none): [0] = the one fetch_record took last ... [PIPE - 1] = the one being reduced
  constexpr int PIPE = DEPTH + 2;
  // (kept only by the dealt form: under static dealing unit t is a closed form — its pipeline as registers cost spills)
  int u_unit[dynamic ? PIPE : 1];
#pragma unroll
  for (int q = 0; q < (dynamic ? PIPE : 1); ++q) u_unit[q] = -1;
  int32_t* l_deal = reinterpret_cast<int32_t*>(lds + a.deal_off);   // 0 .. PIPE - 2: the prologue's units, 6 / 7: the loop's
  // l_deal holds the counter's values as taken; every wave turns one into its unit (2 * cluster + half; < 0: the span is exhausted)
  auto next_unit = [&](int deal_slot) {
    if constexpr (dynamic) {
#pragma unroll
      for (int q = PIPE - 1; q > 0; --q) u_unit[q] = u_unit[q - 1];
      const unsigned idx = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(l_deal[deal_slot]));
      const unsigned part = idx >= static_cast<unsigned>(span) ? 1u : 0u;
      u_unit[0] = idx < 2u * static_cast<unsigned>(span) ? static_cast<int>(((clo + idx - part * span) << 1) | part) : -1;
    }
  };
  // stage k of the pipeline while unit `newest` is the one fetch_record takes: its unit, or < 0
  auto unit_at = [&](int k, int newest) {
    if constexpr (dynamic) {
      return u_unit[k];
    } else {
      const int t = newest - k;
      return t < n_static ? lo + j + t * per_xcd : -1;
    }
  };
  // the dealer (the workgroup's last wave): `count` units off the XCD's counter (take) into l_deal[slot0 ..] (publish).  In the loop
  // the add is issued in one iteration and published at the top of the next, behind the wait every wave makes there anyway: the dealer
  // never waits for the counter's round trip on its own.
  auto take = [&](int count) {
    unsigned base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(a.counters + 32 * xcd, static_cast<unsigned>(count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return base;
  };
  auto publish = [&](unsigned taken, int count, int slot0) {
    if (lane == 0) {
      for (int q = 0; q < count; ++q) l_deal[slot0 + q] = static_cast<int>(taken + q);
    }
  };
  auto fetch_record = [&](int t, int unit) {   // record of unit t -> its slot, by LDS-DMA (waves 0 / 1: one piece each)
    if (wave < pieces) {
      const unsigned cluster = static_cast<unsigned>(unit) >> 1;
      const int word = 256 * wave + 4 * lane;
      const unsigned voff = word < words ? (cluster * static_cast<unsigned>(words) + word) * 4u : 0xFFFFFFF0u;
      rr(lds + (t % n_recs) * rec_bytes + 1024 * wave, voff);
    }
  };
  auto issue_gathers = [&](int t, int unit) {   // this wave's share of unit t's gathers; its record is in LDS.  Returns their count
    const int32_t* l_rec = reinterpret_cast<const int32_t*>(lds + (t % n_recs) * rec_bytes);
    unsigned char* image = images + (t % n_images) * image_bytes;
    const int n_srcs = l_rec[1];
    const int part = unit & 1;
    const int half = lane >> 5;
    // lane l keeps the id of row 2 (wave + n_waves (l / 2)) + l % 2: every row pair this wave fetches, one LDS read
    const int last = pad4(a.max_srcs) - 1;
    const int32_t ids = l_rec[a.layout.srcs + min(2 * (wave + n_waves * (lane >> 1)) + (lane & 1), last)];
    int k = 0;
    gather_halves(rt, part, image, n_srcs, 2 * wave, 2 * n_waves, [&](int) {
      const int s0 = __builtin_amdgcn_readlane(ids, 2 * k), s1 = __builtin_amdgcn_readlane(ids, 2 * k + 1);
      ++k;
      return half ? s1 : s0;
    });
    if constexpr (BWD) {
      // lane l keeps the id of row 8 (wave + n_waves (l / 8)) + l % 8; piece k wants lanes 8 k .. 8 k + 7 spread by eights
      const int32_t ids8 = l_rec[a.layout.srcs + min(8 * (wave + n_waves * (lane >> 3)) + (lane & 7), last)];
      int k8 = 0;
      gather_winner_halves(rw, part, image + ((a.max_srcs + 1) & ~1) * kHalfBytes, n_srcs, 8 * wave, 8 * n_waves, [&](int) {
        const int32_t id = __builtin_amdgcn_ds_bpermute(4 * (8 * k8 + (lane >> 3)), ids8);
        ++k8;
        return id;
      });
      return k + k8;
    }
    return k;
  };

  // Per iteration a wave issues, in this order: [record fetch of unit it + depth + 1 (waves 0 / 1)] [gathers of unit it + depth]
  // [stores of unit it].  At the top of iteration `it` the gathers of unit `it` (issued `depth` iterations ago) and the record
  // fetched in iteration it - 1 must have landed; vector-memory operations retire in order, so everything YOUNGER than that
  // record fetch may stay in flight: the previous iteration's stores and, for depth >= 2, its gathers (for depth 1 those ARE
  // the gathers of unit `it`).
  if constexpr (dynamic) {
    if (wave == n_waves - 1) {
      const unsigned first = take(PIPE);      // ONE round trip for the prologue's units and the one iteration 0 enters
      publish(first, PIPE - 1, 0);
      publish(first + (PIPE - 1), 1, 6);
    }
    barrier_all();
  }
  unsigned taken = 0;                         // the dealer's add of the iteration before
#pragma unroll
  for (int t = 0; t <= depth; ++t) {        // afterwards stage depth - t holds unit t
    next_unit(t);
    if (unit_at(0, t) >= 0) fetch_record(t, unit_at(0, t));
  }
  barrier_all();
  int pending_gathers = 0, stores = 0;
#pragma unroll
  for (int t = 0; t < depth; ++t) pending_gathers = (WHATIF != 1 && unit_at(depth - t, depth) >= 0) ? issue_gathers(t, unit_at(depth - t, depth)) : 0;
  if (depth == 1) pending_gathers = 0;
  // WHATIF == 9 (tools/diag only): shader-clock stamps of wave 0 around the phases of an iteration, summed per workgroup into
  // `arg` (which then is a buffer of 8 x uint64 per workgroup, not the winners): wait for gathers | barrier | issue | reduce
  unsigned long long phase[4] = {0, 0, 0, 0}, stamp = 0;
  auto lap = [&](int which) {
    if constexpr (WHATIF == 9) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      phase[which] += now - stamp;
      stamp = now;
    }
  };
  if constexpr (WHATIF == 9) stamp = __builtin_amdgcn_s_memtime();
  int it = 0;
  for (; dynamic || it < n_static; ++it) {
    wait_vm_all_but(pending_gathers + stores);
    if constexpr (dynamic) {
      if (it > 0 && wave == n_waves - 1) publish(taken, 1, 6 + (it & 1));   // this slot was last read two barriers ago
    }
    lap(0);
    barrier_lds();                          // ... and everyone else's; the oldest image and the oldest record slot are free
    lap(1);
    next_unit(6 + (it & 1));                // stage 0 = unit it + depth + 1, stage 1 = unit it + depth, stage PIPE - 1 = unit it
    const int newest = it + depth + 1;
    const int unit_now = unit_at(PIPE - 1, newest);
    if constexpr (dynamic) {
      if (unit_now < 0) break;              // units come in walk order: nothing behind an empty slot
    }
    if constexpr (dynamic) {
      if (wave == n_waves - 1) taken = take(1);   // published at the top of the next iteration
    }
    if constexpr (DEPTH == 1) {             // the next unit's gathers first, then the record of the unit after it
      if (unit_at(1, newest) >= 0 && WHATIF != 1) issue_gathers(it + 1, unit_at(1, newest));
      if (unit_at(0, newest) >= 0) fetch_record(it + 2, unit_at(0, newest));
    } else {
      if (unit_at(0, newest) >= 0) fetch_record(it + depth + 1, unit_at(0, newest));
      pending_gathers = (unit_at(1, newest) >= 0 && WHATIF != 1) ? issue_gathers(it + depth, unit_at(1, newest)) : 0;
    }
    lap(2);
    const int32_t* l_rec = reinterpret_cast<const int32_t*>(lds + (it % n_recs) * rec_bytes);
    const unsigned char* image = images + (it % n_images) * image_bytes;
    const int part = unit_now & 1;
    if constexpr (WHATIF == 2)
      stores = 0;
    else if constexpr (WHATIF >= 3 && WHATIF <= 4 && !BWD)
      stores = WHATIF == 3 ? (whatif_reduce_max_rows<ARGB, WHATIF>(a, l_rec, image, part, wave, n_waves), 0)
                           : whatif_reduce_max_rows<ARGB, WHATIF>(a, l_rec, image, part, wave, n_waves);
    else if constexpr (BWD)
      stores = reduce_winner_rows(a, l_rec, image, image + ((a.max_srcs + 1) & ~1) * kHalfBytes, part, wave, n_waves);
    else
      stores = whatif_reduce_max_rows<ARGB>(a, l_rec, image, part, wave, n_waves);
    lap(3);
  }
  if constexpr (WHATIF == 9) {
    if (threadIdx.x == 0) {
      unsigned long long* dbg = reinterpret_cast<unsigned long long*>(a.arg) + 8 * static_cast<size_t>(blockIdx.x);
      for (int q = 0; q < 4; ++q) dbg[q] = phase[q];
      dbg[4] = static_cast<unsigned long long>(it);
    }
  }
  // the last workgroup of the XCD to finish leaves the counters zero for the next launch
  if (dynamic && threadIdx.x == 0) {   // (compile-time)
    unsigned* done = a.counters + 32 * xcd + 16;
    if (__hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == static_cast<unsigned>(per_xcd) - 1u) {
      __hip_atomic_store(a.counters + 32 * xcd, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <bool BWD, int ARGB, int WHATIF = 0>
inline int launch_cluster_whatif(ClusterArgs a, int max_rows, int loc_words, hipStream_t st) {
  const LdsPlan p = lds_plan(max_rows, a.max_srcs, loc_words, BWD);
  a.image_off = p.image_off, a.win_off = p.win_off, a.slot_bytes = p.slot_bytes;
  if (p.slot_bytes > kMaxLds) return GTS_ERR_SHAPE;
  {
    // the timing arms exist at gather depth 1 only: GTS_OPT_CLUSTER_RING is held at 1 while the product's geometry is computed for them
    const int ring_asked = g_cluster_ring;
    if (WHATIF != 0) g_cluster_ring = 1;
    const ClusterGeometry geo = cluster_geometry(a.n_clusters, a.layout.words, p.slot_bytes, p.image_off, BWD);
    g_cluster_ring = ring_asked;
    const int depth = geo.depth, waves = geo.waves;
    const int64_t wg_lds = geo.wg_lds, grid = geo.grid;
    a.deal_off = static_cast<int>(wg_lds) - 64;
    if (wg_lds > kMaxLds || a.layout.words > 512) return GTS_ERR_SHAPE;
    a.ring = depth;
    if (a.max_srcs > 64 * waves) return GTS_ERR_SHAPE;
    // fetch_record: wave p brings piece p of a record.  A workgroup of fewer waves than pieces (GTS_OPT_CLUSTER_CONSUMERS = 1,
    // records of more than 256 words) would reduce from a piece nobody fetched: refused, as the GAT launch refuses it
    if ((a.layout.words + 255) / 256 > waves) return GTS_ERR_SHAPE;
    if (!geo.deals) a.counters = nullptr;
    static const bool once = (allow_big_lds(spmm_cluster_whatif_kernel<BWD, ARGB, WHATIF, 1, false>),
                              allow_big_lds(spmm_cluster_whatif_kernel<BWD, ARGB, WHATIF, 1, true>),
                              allow_big_lds(spmm_cluster_whatif_kernel<BWD, ARGB, WHATIF == 0 ? 0 : WHATIF, WHATIF == 0 ? 2 : 1, false>),
                              allow_big_lds(spmm_cluster_whatif_kernel<BWD, ARGB, WHATIF == 0 ? 0 : WHATIF, WHATIF == 0 ? 2 : 1, true>), true);
    (void)once;
    const dim3 g3(static_cast<unsigned>(grid));
    if constexpr (WHATIF == 0) {
      if (depth == 2) {
        if (a.counters != nullptr) spmm_cluster_whatif_kernel<BWD, ARGB, 0, 2, true><<<g3, waves * kWave, wg_lds, st>>>(a);
        else spmm_cluster_whatif_kernel<BWD, ARGB, 0, 2, false><<<g3, waves * kWave, wg_lds, st>>>(a);
        return launch_status();
      }
    }
    if (a.counters != nullptr) spmm_cluster_whatif_kernel<BWD, ARGB, WHATIF, 1, true><<<g3, waves * kWave, wg_lds, st>>>(a);
    else spmm_cluster_whatif_kernel<BWD, ARGB, WHATIF, 1, false><<<g3, waves * kWave, wg_lds, st>>>(a);
    return launch_status();
  }
}

}  // namespace
}  // namespace gts
