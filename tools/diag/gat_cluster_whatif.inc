// The persistent clustered GAT kernel WITH ITS TIMING ARMS AND DEEPER PIPELINES, kept out of libgts_hip.so: cut as it stood at commit
// 9c71b5b ("Pin clustered K1/K2 and GAT kernels on hand-made cluster schedules") out of gnn-tumor-seg_amd/csrc/gts_gat_cluster.hip,
// where all of this sat inside the product kernel:
//   WHATIF 1 = no neighbour gathers, 2 = no reduction and no stores, 3 = reduction without stores, 9 = shader-clock stamps of wave 0
//          around the phases of an iteration, written over `out`;
//   DEPTH  2, 3 = gathers two / three units ahead of the reduction (MAXDEPTH, the `depth` of the plan): measured, no gain
//          (profiles/r04/gat_depth_ab.log) — the library runs depth 1 and its kernel knows no other;
//   grid_override = a launch of that many workgroups (8 = one per XCD: the span's units strictly in order).
// A frozen experiment (logs: profiles/r04/gat_whatif_*.log, gat_l2_replay.log): it carries its own copy of the unit dealing as it was
// then — the static walk's closed form divides by zero on an XCD whose span is empty (fewer than 8 clusters), fixed in the product
// only — and need not follow the product kernel.  Include it BEHIND gts_gat_cluster.hip (whose GatClusterArgs, GatPlan,
// reduce_edge_rows and helpers it uses), as tools/diag/gat_whatif.hip does.
// Adapted, otherwise the text of that commit: the names (whatif_reduce_wsum_rows, gat_cluster_whatif_kernel, launch_gat_cluster_whatif)
// and the plan, which extends the product's GatPlan by its depth (GatWhatifPlan, gat_whatif_plan).

#include <mutex>
#include <vector>

namespace gts {
namespace {

// the rows of one unit out of LDS: half a wave per row, 16 B per lane; acc = w_k * slice_k + acc in slot order (`mad`), one
// straight-line body per exact edge count of an 8-edge chunk.  The kernel is bound by the vector instructions it issues
// (profiles/r04: without its gathers it takes 3 / 4 of its time), so the common pair of rows — equal degrees, one chunk — runs
// a body without per-edge masks: the exact count is both rows' count.  Returns the number of store instructions issued.
template <bool BWD, bool NOSTORE = false>   // NOSTORE: tools/diag what-if runs only
__device__ __forceinline__ int whatif_reduce_wsum_rows(const GatClusterArgs& a, const int32_t* l_rec, const unsigned char* image,
                                                const float* l_side, const float* l_vec, int sub, int first, int step) {
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
    const int deg_a = __builtin_amdgcn_readlane(deg, 0), deg_b = __builtin_amdgcn_readlane(deg, 32);
    const int deg_w = max(deg_a, deg_b);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (deg_a == deg_b && deg_w <= 8) {
      if (deg_w > 0) {
        const uint2 w = loc[c0];
        const float4 wa = *reinterpret_cast<const float4*>(l_side + c0 * 8), wb = *reinterpret_cast<const float4*>(l_side + c0 * 8 + 4);
        const float wts[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
        for_count(deg_w, [&](auto cnt_c) {
          constexpr int CNT = decltype(cnt_c)::value;
          float4 val[CNT];
#pragma unroll
          for (int q = 0; q < CNT; ++q) val[q] = *reinterpret_cast<const float4*>(mine + chunk_byte(w, q) * kHalfBytes);
#pragma unroll
          for (int q = 0; q < CNT; ++q) {
            acc[0] = mad(wts[q], val[q].x, acc[0]);
            acc[1] = mad(wts[q], val[q].y, acc[1]);
            acc[2] = mad(wts[q], val[q].z, acc[2]);
            acc[3] = mad(wts[q], val[q].w, acc[3]);
          }
        });
      }
    } else {
      for (int c = 0; 8 * c < deg_w; ++c) {
        const int at = 8 * c < deg ? c0 + c : c0;                 // the shorter row of the pair re-reads its first chunk, masked below
        const uint2 w = loc[at];
        const float4 wa = *reinterpret_cast<const float4*>(l_side + at * 8), wb = *reinterpret_cast<const float4*>(l_side + at * 8 + 4);
        const float wts[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
        for_count(min(8, deg_w - 8 * c), [&](auto cnt_c) {
          constexpr int CNT = decltype(cnt_c)::value;
          float4 val[CNT];
#pragma unroll
          for (int q = 0; q < CNT; ++q) val[q] = *reinterpret_cast<const float4*>(mine + chunk_byte(w, q) * kHalfBytes);
#pragma unroll
          for (int q = 0; q < CNT; ++q) {
            const bool live = 8 * c + q < deg;
            const float v4[4] = {val[q].x, val[q].y, val[q].z, val[q].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = live ? mad(wts[q], v4[t], acc[t]) : acc[t];
          }
        });
      }
    }
    Vec<4> o{{acc[0], acc[1], acc[2], acc[3]}};
    if constexpr (BWD) {
      if (a.vec != nullptr) {   // el = <ft, attn_l>, er = <ft, attn_r>: their gradient w.r.t. ft
        const float2 sc = have ? *reinterpret_cast<const float2*>(l_side + a.chunk_slots * 8 + j * 2) : float2{0.f, 0.f};
        const float4 al = *reinterpret_cast<const float4*>(l_vec + hl * 4), ar = *reinterpret_cast<const float4*>(l_vec + 128 + hl * 4);
        const float al4[4] = {al.x, al.y, al.z, al.w}, ar4[4] = {ar.x, ar.y, ar.z, ar.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) o.v[t] = mad(sc.y, ar4[t], mad(sc.x, al4[t], o.v[t]));
      }
    } else {
      if (a.vec != nullptr) {
        const float4 bs = *reinterpret_cast<const float4*>(l_vec + hl * 4);
        o.v[0] += bs.x, o.v[1] += bs.y, o.v[2] += bs.z, o.v[3] += bs.w;
      }
      if (a.act == 1) {   // ELU: both pairs through elu_expm1_pair (gts_rows.h), then the selects — NaN included
        const v2f lo = elu_expm1_pair(v2f{o.v[0], o.v[1]}), hi = elu_expm1_pair(v2f{o.v[2], o.v[3]});
        o.v[0] = o.v[0] > 0.0f ? o.v[0] : lo.x;
        o.v[1] = o.v[1] > 0.0f ? o.v[1] : lo.y;
        o.v[2] = o.v[2] > 0.0f ? o.v[2] : hi.x;
        o.v[3] = o.v[3] > 0.0f ? o.v[3] : hi.y;
      }
    }
    if constexpr (NOSTORE) {
      if (o.v[0] == 123.456f) a.out[0] = o.v[1] + o.v[2] + o.v[3];
    } else if (have) {   // streamed out (GTS_OPT_CLUSTER_STREAMING, default on): the rows just written do not push the halo slices out of the XCD's L2
      float* dst = a.out + (static_cast<size_t>(l_rec[a.layout.rows + j]) * a.heads * kF + sub * (kF / 2) + hl * 4);
      if (a.nt) o.store_nt(dst); else o.store(dst);
    }
  }
  return NOSTORE ? 0 : trips;
}

// gridDim.x is a multiple of 8: the workgroups with blockIdx % 8 == x (one XCD under round-robin placement; speed only)
// share the x-th eighth of the CLUSTERS and walk its units sub-unit by sub-unit (all clusters of the span for head 0 /
// left half, then head 0 / right half, ...), round-robin: the units in flight on an XCD at one time are the same
// column half of neighbouring clusters, whose halo slices meet in its L2.
// MINW = 8: up to 16 waves per workgroup at <= 64 registers; 6: up to 12 waves at <= 80 (two workgroups per CU either way)
// MODE 0: forward aggregation;  1: source pass of the backward;  2: edge pass of the backward (half dot products)
// DEPTH: units the gathers run ahead of the reduction (DEPTH + 1 images).  A unit's reduction is short beside the round trip
// of its gathers, so with one unit ahead a workgroup spends most of an iteration waiting for the LAST of ~35 KB to land and the
// kernel's rate is (bytes in flight) / (loaded latency), whatever the L2 hits (profiles/r04: the time does not move with the
// bytes fetched); deeper images keep more of the LDS in flight.  Records run max(1, DEPTH - 1) units in front of the gathers.
// WHATIF (tools/diag only): 1 = no neighbour gathers, 2 = no reduction and no stores, 3 = reduction without stores
template <int MODE, int MINW, int DEPTH = 1, int WHATIF = 0>
__global__ __launch_bounds__(1024, MINW) void gat_cluster_whatif_kernel(const GatClusterArgs a) {
  constexpr bool BWD = MODE == 1;
  constexpr int AHEAD = DEPTH > 1 ? DEPTH - 1 : 1;   // records are fetched this many units in front of their gathers
  constexpr int R = DEPTH + AHEAD + 1;               // record / weight / vector slots
  constexpr int IMAGES = DEPTH + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int n_waves = blockDim.x / kWave;
  const int xcd = blockIdx.x & 7, jw = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
  const int subs = 2 * a.heads;
  const int clo = static_cast<int>(static_cast<long long>(a.n_clusters) * xcd / 8);
  const int span = static_cast<int>(static_cast<long long>(a.n_clusters) * (xcd + 1) / 8) - clo;
  const long long n_local = static_cast<long long>(span) * subs;
  // Dealing.  STATIC (a.counters == nullptr): unit i of the span to workgroup i % per_xcd.  A workgroup that falls ONE unit behind
  // its neighbours is then per_xcd units behind in the walk — a whole generation — and the halo slices it shares with them have
  // left the L2 before it asks: with the reduction in the loop the kernel fetched 1.57 x the table where the same walk without it
  // (all workgroups in step) fetched 1.20 x (profiles/r04/gat_l2_replay.log).  DYNAMIC (the default): the workgroups of an XCD
  // take their units from ONE counter (an agent-scope atomic add by the workgroup's last wave, one iteration before the unit's
  // record is fetched; the value goes round through LDS with the iteration's barrier), so the units in flight are always the
  // latest per_xcd ones of the walk, whatever the pace of each workgroup.  Which workgroup computes a unit changes nothing in what
  // it computes.
  const bool dynamic = a.counters != nullptr;
  const int n_static = jw < n_local ? static_cast<int>((n_local - jw + per_xcd - 1) / per_xcd) : 0;
  if (!dynamic && n_static == 0) return;
  const int words = a.layout.words;
  const int rec_pieces = a.rec_bytes / 1024;
  unsigned char* side_slots = lds + R * a.rec_bytes;
  unsigned char* vec_slots = side_slots + R * a.side_slot_bytes;
  unsigned char* images = MODE == 2 ? lds + R * a.rec_bytes : vec_slots + R * 1024;   // the edge pass keeps no weight / vector slots
  const RawDma rr(a.rec, static_cast<unsigned>(a.n_clusters) * words * 4u);
  const RawDma rt(a.table, a.table_bytes);
  const RawDma rs(a.side, a.side_bytes);
  const RawDma rv(a.vec, a.vec != nullptr ? a.vec_bytes : 0);
  const RawDma ro(MODE == 2 ? a.own : a.table, MODE == 2 ? a.own_bytes : a.table_bytes);
  // Unit order inside the span: groups of `a.group` consecutive clusters, a group walked through ALL its (head, half) slices
  // before the next one — consecutive units (= what the XCD's workgroups hold at one time) are the same slice of the group's
  // clusters, then the next slice of the same clusters.
  const unsigned group = static_cast<unsigned>(a.group > 0 && a.group < span ? a.group : span);
  // The walk is kept as scalar state and advanced by per_xcd units at a time (a few scalar operations: the two integer divisions
  // of the closed form, taken three times per iteration, were a fifth of the kernel's time — profiles/r04): `at` = the unit
  // fetch_record takes next, (first, size) its group, s its slice, c its cluster inside the group.
  unsigned w_first, w_size, w_s, w_c;
  {
    const unsigned i = static_cast<unsigned>(jw);                                  // this workgroup's first unit: the closed form, once
    const unsigned per_group = group * static_cast<unsigned>(subs);
    const unsigned gi = i / per_group, r = i - gi * per_group;
    w_first = gi * group;
    w_size = min(group, static_cast<unsigned>(span) - w_first);
    w_s = r / w_size;
    w_c = r - w_s * w_size;
  }
  auto advance = [&]() {                     // per_xcd units on; past the span's end the state is never used (size kept >= 1)
    w_c += static_cast<unsigned>(per_xcd);
    while (w_c >= w_size) {
      w_c -= w_size;
      if (++w_s == static_cast<unsigned>(subs)) {
        w_s = 0;
        w_first += group;
        w_size = w_first < static_cast<unsigned>(span) ? min(group, static_cast<unsigned>(span) - w_first) : 0x40000000u;
      }
    }
  };
  // (cluster, sub) of the units in the pipeline: [0] = the one fetch_record took last ... [PIPE - 1] = the one being reduced;
  // cluster < 0: no unit (the span is exhausted)
  constexpr int PIPE = DEPTH + AHEAD + 1;
  int u_cluster[PIPE], u_sub[PIPE];
#pragma unroll
  for (int q = 0; q < PIPE; ++q) u_cluster[q] = -1, u_sub[q] = 0;
  int32_t* l_deal = reinterpret_cast<int32_t*>(lds + a.deal_off);   // dynamic dealing: 8 x (cluster, sub); 0 .. PIPE - 2 the prologue's, 6 / 7 the loop's
  int entered = 0;
  auto next_unit = [&](int deal_slot) {      // shift the pipeline and enter the next unit at [0]
#pragma unroll
    for (int q = PIPE - 1; q > 0; --q) u_cluster[q] = u_cluster[q - 1], u_sub[q] = u_sub[q - 1];
    if (dynamic) {
      u_cluster[0] = __builtin_amdgcn_readfirstlane(l_deal[2 * deal_slot]);
      u_sub[0] = __builtin_amdgcn_readfirstlane(l_deal[2 * deal_slot + 1]);
    } else if (entered < n_static) {
      u_cluster[0] = clo + static_cast<int>(w_first + w_c), u_sub[0] = static_cast<int>(w_s);
      advance();
      ++entered;
    } else {
      u_cluster[0] = -1;
    }
  };
  // the dealer (the workgroup's last wave, which fetches no record piece): `count` units off the XCD's counter (take) into
  // l_deal[slot0 ..] (publish).  In the loop the add is issued in one iteration and published at the top of the next, behind the
  // wait every wave makes there anyway: the dealer never waits for the counter's round trip on its own.
  auto take = [&](int count) {
    unsigned base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(a.counters + 32 * xcd, static_cast<unsigned>(count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return base;
  };
  auto publish = [&](unsigned taken, int count, int slot0) {
    const unsigned base = __builtin_amdgcn_readfirstlane(taken);
    for (int q = 0; q < count; ++q) {
      const unsigned idx = base + q;
      const bool ok = idx < static_cast<unsigned long long>(n_local);
      const unsigned sl = idx / static_cast<unsigned>(max(span, 1));   // the whole span slice by slice (an empty span deals nothing)
      if (lane == 0) {
        l_deal[2 * (slot0 + q)] = ok ? clo + static_cast<int>(idx - sl * static_cast<unsigned>(span)) : -1;
        l_deal[2 * (slot0 + q) + 1] = ok ? static_cast<int>(sl) : 0;
      }
    }
  };
  // record, weights and epilogue vectors of unit t -> their slots, one LDS-DMA per piece and wave.  Returns this wave's count
  auto fetch_record = [&](int t, int cluster_id, int sub) {
    const unsigned cluster = static_cast<unsigned>(cluster_id);
    const int slot = t % R;
    if (wave < rec_pieces) {
      const int word = 256 * wave + 4 * lane;
      rr(lds + slot * a.rec_bytes + 1024 * wave, word < words ? (cluster * static_cast<unsigned>(words) + word) * 4u : 0xFFFFFFF0u);
      return 1;
    } else if (MODE == 2) {
      // the edge pass fetches nothing but the record
    } else if (wave < rec_pieces + a.side_pieces) {
      const int p = wave - rec_pieces, word = 256 * p + 4 * lane;
      const unsigned base = (cluster * static_cast<unsigned>(a.heads) + static_cast<unsigned>(sub >> 1)) * static_cast<unsigned>(a.side_floats);
      rs(side_slots + slot * a.side_slot_bytes + 1024 * p, word < a.side_floats ? (base + word) * 4u : 0xFFFFFFF0u);
      return 1;
    } else if (wave == rec_pieces + a.side_pieces && a.vec != nullptr) {
      // 128 floats of this (head, half) from each vector: lanes 0-31 the first (bias / attn_l), lanes 32-63 the second (attn_r)
      const unsigned first = static_cast<unsigned>(sub) * 128u + (lane & 31) * 4u;
      const unsigned off = (lane < 32 ? first : BWD ? static_cast<unsigned>(a.heads) * kF + first : 0x3FFFFFFCu) * 4u;
      rv(vec_slots + slot * 1024, off);
      return 1;
    }
    return 0;
  };
  auto issue_gathers = [&](int t, int sub) {   // this wave's share of unit t's gathers; its record is in LDS.  Returns their count
    const int32_t* l_rec = reinterpret_cast<const int32_t*>(lds + (t % R) * a.rec_bytes);
    unsigned char* image = images + (t % IMAGES) * a.image_bytes;
    const int n_srcs = l_rec[1];
    // lane l keeps the id of row 2 (wave + n_waves (l / 2)) + l % 2: every row pair this wave fetches, one LDS read
    const int last = pad4(a.max_srcs) - 1;
    const int32_t ids = l_rec[a.layout.srcs + min(2 * (wave + n_waves * (lane >> 1)) + (lane & 1), last)];
    const unsigned row_bytes = a.row_bytes;
    const unsigned col = static_cast<unsigned>(sub) * kHalfBytes + (lane & 31) * 16u;
    int k = 0;
    if constexpr (WHATIF != 1) {
      for (int i = 2 * wave; i < n_srcs; i += 2 * n_waves, ++k) {
        const int s0 = __builtin_amdgcn_readlane(ids, 2 * k), s1 = __builtin_amdgcn_readlane(ids, 2 * k + 1);
        rt(image + i * kHalfBytes, static_cast<unsigned>(lane < 32 ? s0 : s1) * row_bytes + col);
      }
    }
    int k2 = 0;
    if constexpr (MODE == 2 && WHATIF != 1) {   // ... and of its rows' own gradient slices, the same way out of the other table
      const int n_rows = l_rec[0];
      const int32_t own_ids = l_rec[a.layout.rows + min(2 * (wave + n_waves * (lane >> 1)) + (lane & 1), n_rows - 1)];
      for (int i = 2 * wave; i < n_rows; i += 2 * n_waves, ++k2) {
        const int s0 = __builtin_amdgcn_readlane(own_ids, 2 * k2), s1 = __builtin_amdgcn_readlane(own_ids, 2 * k2 + 1);
        ro(image + a.own_off + i * kHalfBytes, static_cast<unsigned>(lane < 32 ? s0 : s1) * a.own_row_bytes + col);
      }
    }
    return k + k2;
  };

  // Iteration `it` issues, in this order: [record / weights / vectors of unit it + DEPTH + AHEAD] [gathers of unit it + DEPTH]
  // [stores of unit it].  At its top the gathers of unit `it` and the record of unit it + DEPTH must have landed; vector-memory
  // operations retire in order, and the record of unit it + DEPTH was issued in front of the gathers of unit it + 1 (AHEAD =
  // DEPTH - 1; for DEPTH 1 in front of those of unit `it`), so everything YOUNGER than that record fetch may stay in flight:
  // the gathers of units it + 1 .. it + DEPTH - 1, the stores of the last DEPTH - 1 iterations (for DEPTH 1: of the last
  // one), and the record fetches of the last DEPTH - 2 iterations.
  constexpr int HIST = DEPTH > 1 ? DEPTH - 1 : 1;
  int g_hist[HIST], s_hist[HIST], r_hist[HIST];   // [0] = youngest; wave-uniform counts of this wave's operations
#pragma unroll
  for (int q = 0; q < HIST; ++q) g_hist[q] = s_hist[q] = r_hist[q] = 0;
  if (dynamic) {                               // the first PIPE units of this workgroup in one add: PIPE - 1 for the prologue, one for iteration 0
    if (wave == n_waves - 1) {
      const unsigned first = take(PIPE);      // ONE round trip for the prologue's units and the one iteration 0 enters
      publish(first, PIPE - 1, 0);
      publish(first + (PIPE - 1), 1, 6);
    }
    barrier_all();
  }
  unsigned taken = 0;                          // the dealer's add of the iteration before
#pragma unroll
  for (int t = 0; t < DEPTH + AHEAD; ++t) {   // afterwards u_*[DEPTH + AHEAD - 1 - t] is unit t
    next_unit(t);
    if (u_cluster[0] >= 0) fetch_record(t, u_cluster[0], u_sub[0]);
  }
  barrier_all();
#pragma unroll
  for (int t = 0; t < DEPTH; ++t) {
    const int cnt = u_cluster[DEPTH + AHEAD - 1 - t] >= 0 ? issue_gathers(t, u_sub[DEPTH + AHEAD - 1 - t]) : 0;
    if (t >= 1) {                              // the gathers of units 1 .. DEPTH - 1 stay in flight past the first wait
#pragma unroll
      for (int q = HIST - 1; q > 0; --q) g_hist[q] = g_hist[q - 1];
      g_hist[0] = cnt;
    }
  }
  // WHATIF == 9 (tools/diag only): shader-clock stamps of wave 0 around the phases of an iteration, summed per workgroup into
  // `out` (then a buffer of 8 x uint64 per workgroup, no rows are stored): wait for gathers | barrier | issue | reduce
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
  for (;; ++it) {
    int keep = 0;
    if constexpr (DEPTH == 1) {
      keep = s_hist[0];
    } else {
#pragma unroll
      for (int q = 0; q < DEPTH - 1; ++q) keep += g_hist[q] + s_hist[q];
#pragma unroll
      for (int q = 0; q < DEPTH - 2; ++q) keep += r_hist[q];
    }
    wait_vm_all_but(keep);
    if (dynamic && it > 0 && wave == n_waves - 1) publish(taken, 1, 6 + (it & 1));   // this slot was last read two barriers ago
    lap(0);
    barrier_lds();                          // ... and everyone else's; the oldest image and the oldest slots are free
    lap(1);
    next_unit(6 + (it & 1));                // u_*[0] = unit it + DEPTH + AHEAD, [AHEAD] = unit it + DEPTH, [PIPE - 1] = unit it
    if (u_cluster[PIPE - 1] < 0) break;     // units come in walk order: nothing behind an empty slot
    if (dynamic && wave == n_waves - 1) taken = take(1);   // published at the top of the next iteration
    const int recs = u_cluster[0] >= 0 ? fetch_record(it + DEPTH + AHEAD, u_cluster[0], u_sub[0]) : 0;
    const int gathers = u_cluster[AHEAD] >= 0 ? issue_gathers(it + DEPTH, u_sub[AHEAD]) : 0;
    lap(2);
    const int sub = u_sub[PIPE - 1], cluster = u_cluster[PIPE - 1];
    const int slot = it % R;
    int stores = 0;
    if constexpr (WHATIF == 2) {
      (void)cluster;
    } else if constexpr (MODE == 2) {
      // partial dot products of this (cluster, head) for column half `sub & 1`
      float* block = a.out + (static_cast<size_t>(sub & 1) * a.n_clusters * a.heads + static_cast<size_t>(cluster) * a.heads + (sub >> 1)) *
                                 (a.chunk_slots * 8);
      stores = reduce_edge_rows(a, reinterpret_cast<const int32_t*>(lds + slot * a.rec_bytes), images + (it % IMAGES) * a.image_bytes, block,
                                wave, n_waves);
    } else {
      stores = whatif_reduce_wsum_rows<BWD, WHATIF == 3 || WHATIF == 9>(a, reinterpret_cast<const int32_t*>(lds + slot * a.rec_bytes),
                                                   images + (it % IMAGES) * a.image_bytes,
                                                   reinterpret_cast<const float*>(side_slots + slot * a.side_slot_bytes),
                                                   reinterpret_cast<const float*>(vec_slots + slot * 1024), sub, wave, n_waves);
    }
#pragma unroll
    for (int q = HIST - 1; q > 0; --q) g_hist[q] = g_hist[q - 1], s_hist[q] = s_hist[q - 1], r_hist[q] = r_hist[q - 1];
    g_hist[0] = gathers, s_hist[0] = stores, r_hist[0] = recs;
    lap(3);
  }
  if constexpr (WHATIF == 9) {
    if (threadIdx.x == 0) {
      unsigned long long* dbg = reinterpret_cast<unsigned long long*>(a.out) + 8 * static_cast<size_t>(blockIdx.x);
      for (int q = 0; q < 4; ++q) dbg[q] = phase[q];
      dbg[4] = static_cast<unsigned long long>(it);
    }
  }
}

struct GatWhatifPlan : GatPlan {
  int depth;
};
// depth: units the gathers run ahead.  The library runs depth 1 (two images, two workgroups per CU); 2 and 3 are instantiated
// by tools/diag/gat_whatif.hip only (measured: no gain — the kernels are bound by the vector instructions they issue, and the
// deeper images leave room for one workgroup per CU; profiles/r04/gat_depth_ab.log)
inline GatWhatifPlan gat_whatif_plan(int max_rows, int max_srcs, int loc_words, bool tagged, bool bwd, bool edge = false, int depth = 1) {
  GatWhatifPlan p;
  p.chunk_slots = loc_words / 2;
  p.side_floats = p.chunk_slots * 8 + (bwd ? max_rows * 2 : 0);
  p.side_pieces = (p.side_floats + 255) / 256;
  p.rec_bytes = 1024 * ((rec_layout(max_rows, max_srcs, loc_words, tagged).words + 255) / 256);
  p.side_slot_bytes = 1024 * p.side_pieces;
  p.image_bytes = (((max_srcs + 1) & ~1) + (edge ? (max_rows + 1) & ~1 : 0)) * kHalfBytes;   // edge pass: the rows' own slices behind the neighbours'
  p.waves = g_gat_cluster_waves > 0 ? std::max(4, std::min(16, g_gat_cluster_waves)) : 12;
  for (p.depth = std::max(1, std::min(3, depth));; --p.depth) {
    const int64_t slots = p.depth + std::max(1, p.depth - 1) + 1;
    p.wg_lds = slots * p.rec_bytes + (edge ? 0 : slots * (p.side_slot_bytes + 1024)) + (p.depth + 1LL) * p.image_bytes + 64;
    if (p.wg_lds <= kMaxLds || p.depth == 1) break;
  }
  return p;
}

template <int MODE, int WHATIF = 0, int MAXDEPTH = 1>
int launch_gat_cluster_whatif(GatClusterArgs a, const GatWhatifPlan& p, hipStream_t st, int64_t grid_override = 0) {   // override: tools/diag only
  a.side_floats = p.side_floats, a.chunk_slots = p.chunk_slots, a.side_pieces = p.side_pieces;
  a.rec_bytes = p.rec_bytes, a.side_slot_bytes = p.side_slot_bytes, a.image_bytes = p.image_bytes;
  a.own_off = ((a.max_srcs + 1) & ~1) * kHalfBytes;
  a.deal_off = static_cast<int>(p.wg_lds) - 64;
  if (g_gat_cluster_dealing == 1) a.counters = nullptr;   // static round-robin dealing (A/B runs)
  a.group = g_gat_cluster_group > 0 ? g_gat_cluster_group : 16;   // profiles/r04: source pass 152 -> 146 us, the other two passes unchanged
  const int per_cu = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>({g_cluster_per_cu > 0 ? g_cluster_per_cu : 2, kMaxLds / p.wg_lds,
                                                                               static_cast<int64_t>(32 / p.waves)})));
  const int64_t units = 2LL * a.heads * a.n_clusters;
  int64_t grid = static_cast<int64_t>(device_cus()) * per_cu;
  grid = std::max<int64_t>(8, std::min(grid, (units + 7) / 8 * 8)) / 8 * 8;
  if (grid_override > 0) grid = (grid_override + 7) / 8 * 8;
  auto go = [&](auto kernel) {
    static std::mutex guard;               // the LDS attribute once per kernel, not per launch
    static std::vector<const void*> allowed;
    {
      std::lock_guard<std::mutex> lock(guard);
      const void* id = reinterpret_cast<const void*>(kernel);
      if (std::find(allowed.begin(), allowed.end(), id) == allowed.end()) allow_big_lds(kernel), allowed.push_back(id);
    }
    kernel<<<dim3(static_cast<unsigned>(grid)), p.waves * kWave, p.wg_lds, st>>>(a);
    return launch_status();
  };
  if constexpr (MAXDEPTH >= 3) {
    if (p.depth == 3) return p.waves > 12 ? go(gat_cluster_whatif_kernel<MODE, 8, 3, WHATIF>) : go(gat_cluster_whatif_kernel<MODE, 6, 3, WHATIF>);
  }
  if constexpr (MAXDEPTH >= 2) {
    if (p.depth == 2) return p.waves > 12 ? go(gat_cluster_whatif_kernel<MODE, 8, 2, WHATIF>) : go(gat_cluster_whatif_kernel<MODE, 6, 2, WHATIF>);
  }
  if (p.depth != 1) return GTS_ERR_ARGKIND;
  return p.waves > 12 ? go(gat_cluster_whatif_kernel<MODE, 8, 1, WHATIF>) : go(gat_cluster_whatif_kernel<MODE, 6, 1, WHATIF>);
}

}  // namespace
}  // namespace gts
