// H1-H4: the BraTS 95th-percentile Hausdorff distance on the device — the border extraction, the
// six distance transforms and the percentile's order statistics that model/evaluation.py runs with
// scipy (binary_erosion, distance_transform_edt, np.percentile) for GNN.evaluate and
// RefinementModel.evaluate.
//
// Channels: bit c of a voxel's border byte is B(region c % 3, side c / 3) with regions WT / CT / ET
// and sides pred / truth.  scipy's EDT value is sqrt(float64(d2)) with d2 the exact integer minimum
// squared distance, so the device only has to produce the integers d2(p, B(r, other side)) for every
// p in B(r, side) and select two order statistics of that multiset; the host takes the square roots
// and interpolates.  Everything here is integer arithmetic: results do not depend on scheduling.
//
//   H1  border bits (the region rule is gts_volume.h's region_bits), one byte per voxel, plus the 6
//       border counts (block_add_counters: wave sums, one atomic per workgroup and channel);
//   H2  1-D distance along Z (the contiguous axis) to the nearest border voxel of each channel: the
//       lines of a workgroup are one contiguous byte range, staged in LDS and swept forward and back
//       by one lane per line; uint16 out (extents <= 4097), 0xFFFF = no feature in the line;
//   H3  along Y: exact lower envelope of the parabolas g^2(q) + (y - q)^2 (Felzenszwalb-Huttenlocher,
//       intersections compared by int64 cross-multiplication), one lane per (x, z) line, lanes of a
//       wave on consecutive z so every step of the walk is one coalesced row; int32 out;
//   H4  the same envelope along X, evaluated only where the OPPOSITE side's border bit is set; each
//       value goes to its region's histogram of d2 (bins below kSmallBins in LDS first); the distance
//       volume itself is never written;
//   H5  (selection) prefix sums over each region's histogram find the ranks np.percentile(., 95)
//       interpolates between.
//
// Under a voxel spacing (gts_surface_stats_i16) the squared distance is D2 = sum_a u_a^2 (p_a - q_a)^2 with
// integer units u_a, an exact int64.  H1 and H2 serve unchanged (H2's index distance along Z is what the
// weighted passes scale), and three weighted kernels replace H3-H5:
//   H3w the envelope of u_z^2 g^2(q) + u_y^2 (y - q)^2 along Y; int64 out;
//   H4w the envelope of f(q) + u_x^2 (x - q)^2 along X at the opposite side's border voxels; D2 has no
//       histogram to go to (one bin per value of B + 1 <= 2^62), so each value is appended to its region's
//       list (one cursor atomic per wave step) and counted against up to four thresholds D2 <= T_k;
//   H5w an 8-bit radix select over each region's list of int64 keys for the same two ranks, from the top
//       digit of the volume's bound B down (the house form of gts_select.h, 64-bit keys, one list per region).
#include "gts_volume.h"

namespace gts {
namespace {

constexpr int kChannels = 6;
constexpr uint16_t kInf16 = 0xFFFF;
constexpr int32_t kInf32 = 0x7FFFFFFF;
constexpr int64_t kMaxBound = int64_t{1} << 24;  // largest (X-1)^2 + (Y-1)^2 + (Z-1)^2 accepted
constexpr int kLineLanes = 64;                     // H2-H4: one wave per workgroup, one lane per line
constexpr int kLdsBudget = 64 * 1024;              // dynamic LDS of one H2-H4 workgroup
constexpr int kSmallBins = 1024;                   // H4's per-workgroup LDS histogram
constexpr int kSelectThreads = 1024;

// H1.  A region voxel is border when a 6-neighbour inside the volume lies outside the region, or when
// it lies on a face of an axis longer than 1; with all_border every region voxel is border.
__global__ __launch_bounds__(kBlock) void hd95_border_kernel(const int16_t* __restrict__ pred,
                                                             const int16_t* __restrict__ truth,
                                                             uint8_t* __restrict__ bits, unsigned* __restrict__ counts,
                                                             int X, int Y, int Z, int all_border) {
  const unsigned n = static_cast<unsigned>(X) * Y * Z, yz = static_cast<unsigned>(Y) * Z;
  unsigned mine[kChannels] = {0, 0, 0, 0, 0, 0};
  for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const auto [x, y, z] = split_xyz(i, Y, Z);
    unsigned out = 0;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int16_t* v = side ? truth : pred;
      unsigned m = region_bits(v[i]);
      if (m && !all_border) {
        unsigned inner = m;
        if (Z > 1) inner &= (z > 0 ? region_bits(v[i - 1]) : 0u) & (z + 1 < unsigned(Z) ? region_bits(v[i + 1]) : 0u);
        if (Y > 1) inner &= (y > 0 ? region_bits(v[i - Z]) : 0u) & (y + 1 < unsigned(Y) ? region_bits(v[i + Z]) : 0u);
        if (X > 1) inner &= (x > 0 ? region_bits(v[i - yz]) : 0u) & (x + 1 < unsigned(X) ? region_bits(v[i + yz]) : 0u);
        m &= ~inner;
      }
      out |= m << (3 * side);
    }
    bits[i] = static_cast<uint8_t>(out);
#pragma unroll
    for (int c = 0; c < kChannels; ++c) mine[c] += (out >> c) & 1u;
  }
  block_add_counters(mine, counts);
}

// H2.  Lines line0 .. line0 + lines - 1 (flattened (x, y)) are the contiguous bytes [line0 * Z, ...).
__global__ __launch_bounds__(kLineLanes) void hd95_pass_z_kernel(const uint8_t* __restrict__ bits,
                                                                 uint16_t* __restrict__ g1, int n_lines, int Z,
                                                                 int lines_per_block, size_t n) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int line0 = blockIdx.x * lines_per_block;
  const int lines = min(lines_per_block, n_lines - line0);
  const int len = lines * Z;
  uint8_t* b = lds;
  uint16_t* d = reinterpret_cast<uint16_t*>(lds + ((lines_per_block * Z + 15) & ~15));
  const size_t base = static_cast<size_t>(line0) * Z;
  for (int k = threadIdx.x; k < len; k += kLineLanes) b[k] = bits[base + k];
  __syncthreads();
  const int t = threadIdx.x;
  for (int c = 0; c < kChannels; ++c) {
    if (t < lines) {
      const uint8_t* bl = b + t * Z;
      uint16_t* dl = d + t * Z;
      int last = -1;
      for (int z = 0; z < Z; ++z) {
        if ((bl[z] >> c) & 1) last = z;
        dl[z] = last < 0 ? kInf16 : static_cast<uint16_t>(z - last);
      }
      last = -1;
      for (int z = Z - 1; z >= 0; --z) {
        if ((bl[z] >> c) & 1) last = z;
        if (last >= 0 && last - z < dl[z]) dl[z] = static_cast<uint16_t>(last - z);
      }
    }
    __syncthreads();
    uint16_t* out = g1 + c * n + base;
    for (int k = threadIdx.x; k < len; k += kLineLanes) out[k] = d[k];
    __syncthreads();
  }
}

// Pop test of the integer lower envelope: with stack top p over pp and a new parabola q (pp < p < q,
// h(i) = f(i) + i^2), p is hidden when its intersection with q is not right of its intersection with pp:
// (h(q) - h(p)) / 2(q - p) <= (h(p) - h(pp)) / 2(p - pp), cross-multiplied (|h| < 2^26, |dq| < 2^13).
__device__ __forceinline__ bool hidden(int64_t hpp, int pp, int64_t hp, int p, int64_t hq, int q) {
  return (hq - hp) * (p - pp) <= (hp - hpp) * (q - p);
}

// H3.  Block (zc, x, c): lanes are the lines (x, z = zc * lanes + lane) of channel c along Y.  LDS per
// lane: the line's 1-D distances (uint16) and the envelope stack (uint16 positions), lane-interleaved.
__global__ __launch_bounds__(kLineLanes) void hd95_pass_y_kernel(const uint16_t* __restrict__ g1,
                                                                 int32_t* __restrict__ g2, int Y, int Z,
                                                                 int lanes, size_t n) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint16_t* f = reinterpret_cast<uint16_t*>(lds);
  uint16_t* v = f + static_cast<size_t>(Y) * lanes;
  const int lane = threadIdx.x, z = blockIdx.x * lanes + lane, x = blockIdx.y, c = blockIdx.z;
  if (lane >= lanes || z >= Z) return;
  const size_t step = Z, base = c * n + static_cast<size_t>(x) * Y * Z + z;
  int k = -1;
  int64_t h_top = 0, h_below = 0;  // h of v[k] and v[k - 1]
  for (int q = 0; q < Y; ++q) {
    const uint16_t g = g1[base + q * step];
    f[q * lanes + lane] = g;
    if (g == kInf16) continue;
    const int64_t hq = int64_t{g} * g + int64_t{q} * q;
    while (k >= 1 && hidden(h_below, v[(k - 1) * lanes + lane], h_top, v[k * lanes + lane], hq, q)) {
      --k;
      h_top = h_below;
      if (k >= 1) {
        const int pp = v[(k - 1) * lanes + lane];
        const int64_t gp = f[pp * lanes + lane];
        h_below = gp * gp + int64_t{pp} * pp;
      }
    }
    ++k;
    v[k * lanes + lane] = static_cast<uint16_t>(q);
    h_below = h_top;
    h_top = hq;
  }
  if (k < 0) {
    for (int y = 0; y < Y; ++y) g2[base + y * step] = kInf32;
    return;
  }
  int j = 0, p = v[lane];
  int32_t fp = int32_t{f[p * lanes + lane]} * f[p * lanes + lane];
  for (int y = 0; y < Y; ++y) {
    while (j < k) {
      const int p1 = v[(j + 1) * lanes + lane];
      const int32_t f1 = int32_t{f[p1 * lanes + lane]} * f[p1 * lanes + lane];
      if (f1 + (y - p1) * (y - p1) > fp + (y - p) * (y - p)) break;
      ++j;
      p = p1;
      fp = f1;
    }
    g2[base + y * step] = fp + (y - p) * (y - p);
  }
}

// H4.  Block (zc, y, c): lanes are the lines (y, z) of channel c along X.  Evaluated only at voxels of
// the opposite side's border; d2 goes to region c % 3's histogram.
__global__ __launch_bounds__(kLineLanes) void hd95_pass_x_kernel(const int32_t* __restrict__ g2,
                                                                 const uint8_t* __restrict__ bits,
                                                                 unsigned* __restrict__ hist, int64_t bins, int X,
                                                                 int Y, int Z, int lanes, size_t n) {
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned* small = reinterpret_cast<unsigned*>(lds);
  int32_t* f = reinterpret_cast<int32_t*>(small + kSmallBins);
  uint16_t* v = reinterpret_cast<uint16_t*>(f + static_cast<size_t>(X) * lanes);
  const int lane = threadIdx.x, z = blockIdx.x * lanes + lane, y = blockIdx.y, c = blockIdx.z;
  const int opposite = c < 3 ? c + 3 : c - 3;
  unsigned* region_hist = hist + (c % 3) * bins;
  for (int b = lane; b < kSmallBins; b += kLineLanes) small[b] = 0;
  __syncthreads();
  if (lane < lanes && z < Z) {
    const size_t step = static_cast<size_t>(Y) * Z, line = static_cast<size_t>(y) * Z + z, base = c * n + line;
    int k = -1;
    int64_t h_top = 0, h_below = 0;
    for (int q = 0; q < X; ++q) {
      const int32_t fq = g2[base + q * step];
      f[q * lanes + lane] = fq;
      if (fq == kInf32) continue;
      const int64_t hq = int64_t{fq} + int64_t{q} * q;
      while (k >= 1 && hidden(h_below, v[(k - 1) * lanes + lane], h_top, v[k * lanes + lane], hq, q)) {
        --k;
        h_top = h_below;
        if (k >= 1) {
          const int pp = v[(k - 1) * lanes + lane];
          h_below = int64_t{f[pp * lanes + lane]} + int64_t{pp} * pp;
        }
      }
      ++k;
      v[k * lanes + lane] = static_cast<uint16_t>(q);
      h_below = h_top;
      h_top = hq;
    }
    if (k >= 0) {  // no feature in the line: the region is absent from that side and the value is unused
      int j = 0, p = v[lane];
      int32_t fp = f[p * lanes + lane];
      for (int x = 0; x < X; ++x) {
        if (!((bits[line + x * step] >> opposite) & 1)) continue;
        while (j < k) {
          const int p1 = v[(j + 1) * lanes + lane];
          const int32_t f1 = f[p1 * lanes + lane];
          if (f1 + (x - p1) * (x - p1) > fp + (x - p) * (x - p)) break;
          ++j;
          p = p1;
          fp = f1;
        }
        const int32_t d2 = fp + (x - p) * (x - p);
        if (d2 < kSmallBins)
          atomicAdd(&small[d2], 1u);
        else
          atomicAdd(&region_hist[d2], 1u);
      }
    }
  }
  __syncthreads();
  for (int b = lane; b < kSmallBins && b < bins; b += kLineLanes)
    if (small[b]) atomicAdd(&region_hist[b], small[b]);
}

// H5.  Block r: out[r] = {n, d2 at rank lo, d2 at rank hi, presence bits (1 pred, 2 truth)} with the
// ranks of np.percentile's linear method at 95: v = (n - 1) * 0.95, lo = floor(v), hi = lo + 1, or
// both n - 1 when v >= n - 1.  Thread t sums bins [t * chunk, (t + 1) * chunk), a block scan places
// the chunks, and the thread whose chunk holds a rank walks it.
__global__ __launch_bounds__(kSelectThreads) void hd95_select_kernel(const unsigned* __restrict__ hist,
                                                                     const unsigned* __restrict__ counts,
                                                                     int64_t bins, long long* __restrict__ out) {
  __shared__ unsigned long long scan[kSelectThreads];
  const int r = blockIdx.x, t = threadIdx.x;
  const long long n_pred = counts[r], n_truth = counts[3 + r], n = n_pred + n_truth;
  const long long flags = (n_pred > 0 ? 1 : 0) | (n_truth > 0 ? 2 : 0);
  if (t == 0) {
    out[4 * r] = n;
    out[4 * r + 3] = flags;
    out[4 * r + 1] = 0;
    out[4 * r + 2] = 0;
  }
  if (flags != 3) return;  // uniform over the block
  const double vi = static_cast<double>(n - 1) * 0.95;
  long long rank[2];
  if (vi >= static_cast<double>(n - 1)) {
    rank[0] = rank[1] = n - 1;
  } else {
    rank[0] = static_cast<long long>(floor(vi));
    rank[1] = rank[0] + 1;
  }
  const unsigned* h = hist + r * bins;
  const int64_t chunk = (bins + kSelectThreads - 1) / kSelectThreads;
  const int64_t b0 = min(bins, t * chunk), b1 = min(bins, b0 + chunk);
  unsigned long long s = 0;
  for (int64_t b = b0; b < b1; ++b) s += h[b];
  scan[t] = s;
  __syncthreads();
  for (int off = 1; off < kSelectThreads; off <<= 1) {
    const unsigned long long add = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const unsigned long long incl = scan[t], excl = incl - s;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const unsigned long long k = static_cast<unsigned long long>(rank[w]);
    if (k < excl || k >= incl) continue;
    unsigned long long acc = excl;
    for (int64_t b = b0; b < b1; ++b) {
      acc += h[b];
      if (k < acc) {
        out[4 * r + 1 + w] = b;
        break;
      }
    }
  }
}

// ------------------------------------------------------------------ the weighted passes (H3w-H5w)
constexpr int64_t kInf64 = INT64_MAX;
constexpr int kMaxThresholds = 4;
constexpr int kOutInts = 4 + 2 * kMaxThresholds;   // one region's row of gts_surface_stats_i16's table
constexpr int kRadixBins = 256;
constexpr int kSelectBlocks = 256;                   // H5w: workgroups per region and pass

struct Thresholds {
  long long t[kMaxThresholds];
  int n;
};

// H5w's state: per region and rank the digits found so far and the rank still to skip among the keys that
// carry them; `active` says the region is present on both sides (only then are ranks selected).
struct SurfaceSelect {
  unsigned long long prefix[3][2];
  unsigned long long rank[3][2];
  unsigned active[3];
};

// H3w.  H3's launch shape and LDS (the line's uint16 index distances and the stack): the int64 values are
// recomputed from g, never staged.  g2 = min over q of uz2 * g(q)^2 + uy2 * (y - q)^2.  The pop test on
// weighted parabolas, h(i) = f(i) + u^2 i^2, is `hidden` itself: the common curvature u^2 cancels from both
// sides.  0 <= h <= B and the index differences are below max(N_a); the host admits a volume only when
// B * max(N_a) < 2^62, so no product leaves int64.
__global__ __launch_bounds__(kLineLanes) void surface_pass_y_kernel(const uint16_t* __restrict__ g1,
                                                                    int64_t* __restrict__ g2, int64_t uz2,
                                                                    int64_t uy2, int Y, int Z, int lanes, size_t n) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint16_t* f = reinterpret_cast<uint16_t*>(lds);
  uint16_t* v = f + static_cast<size_t>(Y) * lanes;
  const int lane = threadIdx.x, z = blockIdx.x * lanes + lane, x = blockIdx.y, c = blockIdx.z;
  if (lane >= lanes || z >= Z) return;
  const size_t step = Z, base = c * n + static_cast<size_t>(x) * Y * Z + z;
  int k = -1;
  int64_t h_top = 0, h_below = 0;  // h of v[k] and v[k - 1]
  for (int q = 0; q < Y; ++q) {
    const uint16_t g = g1[base + q * step];
    f[q * lanes + lane] = g;
    if (g == kInf16) continue;
    const int64_t hq = uz2 * (int64_t{g} * g) + uy2 * (int64_t{q} * q);
    while (k >= 1 && hidden(h_below, v[(k - 1) * lanes + lane], h_top, v[k * lanes + lane], hq, q)) {
      --k;
      h_top = h_below;
      if (k >= 1) {
        const int pp = v[(k - 1) * lanes + lane];
        const int64_t gp = f[pp * lanes + lane];
        h_below = uz2 * (gp * gp) + uy2 * (int64_t{pp} * pp);
      }
    }
    ++k;
    v[k * lanes + lane] = static_cast<uint16_t>(q);
    h_below = h_top;
    h_top = hq;
  }
  if (k < 0) {
    for (int y = 0; y < Y; ++y) g2[base + y * step] = kInf64;
    return;
  }
  int j = 0, p = v[lane];
  int64_t fp = uz2 * (int64_t{f[p * lanes + lane]} * f[p * lanes + lane]);
  for (int y = 0; y < Y; ++y) {
    while (j < k) {
      const int p1 = v[(j + 1) * lanes + lane];
      const int64_t f1 = uz2 * (int64_t{f[p1 * lanes + lane]} * f[p1 * lanes + lane]);
      if (f1 + uy2 * (int64_t{y - p1} * (y - p1)) > fp + uy2 * (int64_t{y - p} * (y - p))) break;
      ++j;
      p = p1;
      fp = f1;
    }
    g2[base + y * step] = fp + uy2 * (int64_t{y - p} * (y - p));
  }
}

// H4w.  Block (zc, y, c) as in H4; LDS per lane: the line's int64 values and the stack.  Every lane of the
// wave walks x together, so that the lanes with a value at this x take their list slots from one atomic on
// the region's cursor.  The values belong to the border voxels of the side opposite to channel c's.
__global__ __launch_bounds__(kLineLanes) void surface_pass_x_kernel(
    const int64_t* __restrict__ g2, const uint8_t* __restrict__ bits, unsigned long long* __restrict__ lists,
    unsigned* __restrict__ cursor, unsigned* __restrict__ within, int64_t ux2, Thresholds th, int X, int Y, int Z,
    int lanes, size_t n) {
  extern __shared__ __align__(16) unsigned char lds[];
  int64_t* f = reinterpret_cast<int64_t*>(lds);
  uint16_t* v = reinterpret_cast<uint16_t*>(f + static_cast<size_t>(X) * lanes);
  const int lane = threadIdx.x, z = blockIdx.x * lanes + lane, y = blockIdx.y, c = blockIdx.z;
  const int opposite = c < 3 ? c + 3 : c - 3, region = c % 3;
  const size_t capacity = 2 * n;  // |B(r, pred)| + |B(r, truth)| <= 2 n
  unsigned long long* list = lists + region * capacity;
  const size_t step = static_cast<size_t>(Y) * Z, line = static_cast<size_t>(y) * Z + z, base = c * n + line;
  int k = -1;
  if (lane < lanes && z < Z) {
    int64_t h_top = 0, h_below = 0;
    for (int q = 0; q < X; ++q) {
      const int64_t fq = g2[base + q * step];
      f[q * lanes + lane] = fq;
      if (fq == kInf64) continue;
      const int64_t hq = fq + ux2 * (int64_t{q} * q);
      while (k >= 1 && hidden(h_below, v[(k - 1) * lanes + lane], h_top, v[k * lanes + lane], hq, q)) {
        --k;
        h_top = h_below;
        if (k >= 1) {
          const int pp = v[(k - 1) * lanes + lane];
          h_below = f[pp * lanes + lane] + ux2 * (int64_t{pp} * pp);
        }
      }
      ++k;
      v[k * lanes + lane] = static_cast<uint16_t>(q);
      h_below = h_top;
      h_top = hq;
    }
  }
  // k < 0: a lane outside the volume, or no feature in the line (the region is absent from that side)
  const bool has = k >= 0;
  int j = 0, p = has ? v[lane] : 0;
  int64_t fp = has ? f[p * lanes + lane] : 0;
  unsigned mine[kMaxThresholds] = {0, 0, 0, 0};
  for (int x = 0; x < X; ++x) {
    const bool on = has && ((bits[line + x * step] >> opposite) & 1);
    int64_t d2 = 0;
    if (on) {
      while (j < k) {
        const int p1 = v[(j + 1) * lanes + lane];
        const int64_t f1 = f[p1 * lanes + lane];
        if (f1 + ux2 * (int64_t{x - p1} * (x - p1)) > fp + ux2 * (int64_t{x - p} * (x - p))) break;
        ++j;
        p = p1;
        fp = f1;
      }
      d2 = fp + ux2 * (int64_t{x - p} * (x - p));
#pragma unroll
      for (int t = 0; t < kMaxThresholds; ++t) mine[t] += (t < th.n && d2 <= th.t[t]) ? 1u : 0u;
    }
    const unsigned long long takers = __ballot(on);
    if (takers) {  // uniform over the wave
      const int leader = __ffsll(static_cast<long long>(takers)) - 1;
      unsigned first = 0;
      if (lane == leader) first = atomicAdd(&cursor[region], static_cast<unsigned>(__popcll(takers)));
      first = __shfl(first, leader, kWave);
      const size_t slot = first + __popcll(takers & ((1ull << lane) - 1));
      if (on && slot < capacity) list[slot] = static_cast<unsigned long long>(d2);
    }
  }
  unsigned* mine_out = within + (region * 2 + opposite / 3) * kMaxThresholds;
#pragma unroll
  for (int t = 0; t < kMaxThresholds; ++t) {
    const unsigned s = wave_sum(mine[t]);
    if (lane == 0 && s) atomicAdd(&mine_out[t], s);
  }
}

// H5w, start: the fixed entries of the table (n, presence bits, the threshold counts) and the two ranks of
// np.percentile's linear method at 95, as H5 takes them.
__global__ void surface_select_init_kernel(const unsigned* __restrict__ counts, const unsigned* __restrict__ within,
                                           SurfaceSelect* __restrict__ st, long long* __restrict__ out) {
  const int r = threadIdx.x;
  if (r >= 3) return;
  const long long n_pred = counts[r], n_truth = counts[3 + r], n = n_pred + n_truth;
  const long long flags = (n_pred > 0 ? 1 : 0) | (n_truth > 0 ? 2 : 0);
  long long* row = out + kOutInts * r;
  row[0] = n;
  row[1] = 0;
  row[2] = 0;
  row[3] = flags;
  for (int i = 0; i < 2 * kMaxThresholds; ++i) row[4 + i] = flags == 3 ? within[r * 2 * kMaxThresholds + i] : 0;
  long long lo = 0, hi = 0;
  if (flags == 3) {
    const double vi = static_cast<double>(n - 1) * 0.95;
    if (vi >= static_cast<double>(n - 1)) {
      lo = hi = n - 1;
    } else {
      lo = static_cast<long long>(floor(vi));
      hi = lo + 1;
    }
  }
  st->prefix[r][0] = st->prefix[r][1] = 0;
  st->rank[r][0] = static_cast<unsigned long long>(lo);
  st->rank[r][1] = static_cast<unsigned long long>(hi);
  st->active[r] = flags == 3;
}

// H5w, one pass: blocks (b, r) count digit (key >> shift) & 255 over the keys of region r's list whose higher
// digits equal a rank's prefix; the second rank has a histogram of its own once the prefixes differ.
__global__ __launch_bounds__(kBlock) void surface_hist_kernel(const unsigned long long* __restrict__ lists,
                                                              size_t capacity, const unsigned* __restrict__ cursor,
                                                              const SurfaceSelect* __restrict__ st,
                                                              unsigned* __restrict__ hist, int shift) {
  __shared__ unsigned h[2 * kRadixBins];
  const int r = blockIdx.y;
  if (!st->active[r]) return;  // uniform over the block
  for (int i = threadIdx.x; i < 2 * kRadixBins; i += kBlock) h[i] = 0;
  const unsigned long long hi_mask = shift + 8 >= 64 ? 0ull : (~0ull << (shift + 8));
  const unsigned long long p0 = st->prefix[r][0], p1 = st->prefix[r][1];
  const bool both = p0 != p1;
  const size_t held = cursor[r], len = held < capacity ? held : capacity;
  const unsigned long long* list = lists + r * capacity;
  __syncthreads();
  for (size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; e < len;
       e += static_cast<size_t>(gridDim.x) * kBlock) {
    const unsigned long long key = list[e];
    const unsigned d = static_cast<unsigned>(key >> shift) & (kRadixBins - 1);
    if (((key ^ p0) & hi_mask) == 0) atomicAdd(&h[d], 1u);
    if (both && ((key ^ p1) & hi_mask) == 0) atomicAdd(&h[kRadixBins + d], 1u);
  }
  __syncthreads();
  unsigned* region_hist = hist + r * 2 * kRadixBins;
  for (int i = threadIdx.x; i < 2 * kRadixBins; i += kBlock)
    if (h[i]) atomicAdd(&region_hist[i], h[i]);
}

// H5w, one step: each (region, rank) walks its histogram to the bin that holds its rank and appends the digit
// to its prefix; the histograms are cleared for the next pass.  After the last pass the prefix is D2.
__global__ __launch_bounds__(kBlock) void surface_select_step_kernel(unsigned* __restrict__ hist,
                                                                     SurfaceSelect* __restrict__ st, int shift,
                                                                     long long* __restrict__ out) {
  const int t = threadIdx.x, r = t >> 1, w = t & 1;
  unsigned long long prefix = 0, k = 0;
  const bool mine = t < 6 && st->active[r];
  if (mine) {
    const bool shared_hist = st->prefix[r][0] == st->prefix[r][1];
    const unsigned* h = hist + (2 * r + (shared_hist ? 0 : w)) * kRadixBins;
    prefix = st->prefix[r][w];
    k = st->rank[r][w];
    unsigned long long acc = 0, digit = kRadixBins - 1;
    for (int b = 0; b < kRadixBins; ++b) {
      if (k < acc + h[b]) {
        digit = b;
        break;
      }
      acc += h[b];
    }
    k -= acc;
    prefix |= digit << shift;
  }
  __syncthreads();  // every walk has read the prefixes and the histograms
  if (mine) {
    st->prefix[r][w] = prefix;
    st->rank[r][w] = k;
    if (shift == 0) out[kOutInts * r + 1 + w] = static_cast<long long>(prefix);
  }
  for (int i = t; i < 3 * 2 * kRadixBins; i += kBlock) hist[i] = 0;
}

struct Hd95Layout {
  int64_t bins, n, hist, bits, g1, g2, total;
};

// false for extents < 1, X * Y * Z >= 2^31 or (X-1)^2 + (Y-1)^2 + (Z-1)^2 > 2^24
inline bool hd95_layout(int64_t X, int64_t Y, int64_t Z, Hd95Layout* l) {
  if (!volume_voxels(X, Y, Z, false, &l->n)) return false;
  // X + Y + Z - 3 <= X * Y * Z < 2^31 for extents >= 1, so the sum of squares stays below 2^62
  const int64_t bound = (X - 1) * (X - 1) + (Y - 1) * (Y - 1) + (Z - 1) * (Z - 1);
  if (bound > kMaxBound) return false;  // every extent is then <= 4097
  l->bins = bound + 1;
  l->hist = kHeaderBytes;  // counts: 6 uint32 in the header
  l->bits = l->hist + round256(3 * l->bins * 4);
  l->g1 = l->bits + round256(l->n);
  l->g2 = l->g1 + round256(kChannels * l->n * 2);
  l->total = l->g2 + kChannels * l->n * 4;
  return true;
}

inline int lanes_for(int64_t bytes_per_lane, int64_t budget) {
  const int64_t l = budget / bytes_per_lane;
  return static_cast<int>(l < kLineLanes ? l : kLineLanes);
}

struct SurfaceLayout {
  int64_t n, sel_hist, sel_state, bits, g1, g2, lists, total;
  int top_shift;  // shift of the highest 8-bit digit a D2 of this volume can have
};

// false for extents outside [1, 4097], X * Y * Z >= 2^31 or B * max(N_a) >= 2^62 with B = sum u_a^2 (N_a - 1)^2:
// every D2 and every h is then at most B and every product of `hidden` stays inside int64.  units must have
// passed units_ok (u^2 (N - 1)^2 <= 10^12 * 2^24 then fits the 128-bit sums used here).
inline bool surface_layout(int64_t X, int64_t Y, int64_t Z, const int64_t* units, SurfaceLayout* l) {
  if (!volume_voxels(X, Y, Z, false, &l->n)) return false;
  if (X > kMmMaxExtent || Y > kMmMaxExtent || Z > kMmMaxExtent) return false;
  const int64_t extent[3] = {X, Y, Z};
  unsigned __int128 bound = 0;
  int64_t longest = 1;
  for (int a = 0; a < 3; ++a) {
    const unsigned __int128 u = static_cast<unsigned __int128>(units[a]), d = extent[a] - 1;
    bound += u * u * d * d;
    if (extent[a] > longest) longest = extent[a];
  }
  if (bound * static_cast<unsigned __int128>(longest) >= (static_cast<unsigned __int128>(1) << 62)) return false;
  l->top_shift = 0;
  while (l->top_shift < 56 && (static_cast<uint64_t>(bound) >> (l->top_shift + 8)) != 0) l->top_shift += 8;
  // header: counts 6 uint32 at 0, list cursors 3 uint32 at 32, threshold counts [3][2][4] uint32 at 64
  l->sel_hist = kHeaderBytes;
  l->sel_state = l->sel_hist + 3 * 2 * kRadixBins * 4;
  l->bits = l->sel_state + round256(sizeof(SurfaceSelect));
  l->g1 = l->bits + round256(l->n);
  l->g2 = l->g1 + round256(kChannels * l->n * 2);
  l->lists = l->g2 + round256(kChannels * l->n * 8);
  l->total = l->lists + 3 * 2 * l->n * 8;
  return true;
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_surface_workspace(int64_t X, int64_t Y, int64_t Z, const int64_t* units) {
  gts::SurfaceLayout l;
  return units && gts::units_ok(units) && gts::surface_layout(X, Y, Z, units, &l) ? l.total : 0;
}

extern "C" int32_t gts_surface_stats_i16(const int16_t* pred, const int16_t* truth, int64_t X, int64_t Y, int64_t Z,
                                         int32_t all_border, const int64_t* units, const int64_t* thresholds,
                                         int32_t n_thresholds, int64_t* out, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!pred || !truth || !units || !out || !workspace) return GTS_ERR_NULL;
  if (n_thresholds < 0 || n_thresholds > kMaxThresholds) return GTS_ERR_ARGKIND;
  if (n_thresholds > 0 && !thresholds) return GTS_ERR_NULL;
  if (!units_ok(units) || (all_border != 0 && all_border != 1)) return GTS_ERR_ARGKIND;
  Thresholds th = {{0, 0, 0, 0}, n_thresholds};
  for (int t = 0; t < n_thresholds; ++t) {
    if (thresholds[t] < 0) return GTS_ERR_ARGKIND;
    th.t[t] = thresholds[t];
  }
  SurfaceLayout l;
  if (!surface_layout(X, Y, Z, units, &l) || workspace_bytes < l.total) return GTS_ERR_SHAPE;
  if (X == 1 && Y == 1 && Z == 1) all_border = 1;  // a lone voxel has no neighbour inside: its own border
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  unsigned* counts = reinterpret_cast<unsigned*>(ws);
  unsigned* cursor = reinterpret_cast<unsigned*>(ws + 32);
  unsigned* within = reinterpret_cast<unsigned*>(ws + 64);
  unsigned* sel_hist = reinterpret_cast<unsigned*>(ws + l.sel_hist);
  SurfaceSelect* sel = reinterpret_cast<SurfaceSelect*>(ws + l.sel_state);
  uint8_t* bits = reinterpret_cast<uint8_t*>(ws + l.bits);
  uint16_t* g1 = reinterpret_cast<uint16_t*>(ws + l.g1);
  int64_t* g2 = reinterpret_cast<int64_t*>(ws + l.g2);
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(ws + l.lists);
  long long* table = reinterpret_cast<long long*>(out);
  const int x = static_cast<int>(X), y = static_cast<int>(Y), z = static_cast<int>(Z);
  const size_t n = static_cast<size_t>(l.n);
  const int64_t ux2 = units[0] * units[0], uy2 = units[1] * units[1], uz2 = units[2] * units[2];

  if (hipMemsetAsync(ws, 0, l.bits, st) != hipSuccess) return launch_status();
  hd95_border_kernel<<<blocks_for(l.n, kBlock, 2048), kBlock, 0, st>>>(pred, truth, bits, counts, x, y, z, all_border);

  const int lz = lanes_for(3 * Z + 16, kLdsBudget);  // H2, as in gts_hd95_order_stats_i16
  const int n_lines = x * y;
  hd95_pass_z_kernel<<<(n_lines + lz - 1) / lz, kLineLanes, static_cast<size_t>(((lz * z + 15) & ~15) + 2 * lz * z),
                       st>>>(bits, g1, n_lines, z, lz, n);

  // H3w stages what H3 stages, uint16 distances (2) and stack positions (2) per element of a line: 64 lanes
  // while 4 Y * 64 <= 64 KiB, i.e. up to Y = 256
  const int ly = lanes_for(4 * Y, kLdsBudget);
  surface_pass_y_kernel<<<dim3((z + ly - 1) / ly, x, kChannels), kLineLanes, static_cast<size_t>(4 * ly * y), st>>>(
      g1, g2, uz2, uy2, y, z, ly, n);

  // H4w: int64 values (8) and stack positions (2) per element, no LDS histogram: 64 lanes while
  // 10 X * 64 <= 64 KiB, i.e. up to X = 102; the longest line (4097) leaves one lane
  const int lx = lanes_for(10 * X, kLdsBudget);
  surface_pass_x_kernel<<<dim3((z + lx - 1) / lx, y, kChannels), kLineLanes, static_cast<size_t>(10 * lx * x), st>>>(
      g2, bits, lists, cursor, within, ux2, th, x, y, z, lx, n);

  surface_select_init_kernel<<<1, kWave, 0, st>>>(counts, within, sel, table);
  const dim3 select_grid(blocks_for(2 * l.n, kBlock, kSelectBlocks), 3);
  for (int shift = l.top_shift; shift >= 0; shift -= 8) {
    surface_hist_kernel<<<select_grid, kBlock, 0, st>>>(lists, 2 * n, cursor, sel, sel_hist, shift);
    surface_select_step_kernel<<<1, kBlock, 0, st>>>(sel_hist, sel, shift, table);
  }
  return launch_status();
}

extern "C" int64_t gts_hd95_workspace(int64_t X, int64_t Y, int64_t Z) {
  gts::Hd95Layout l;
  return gts::hd95_layout(X, Y, Z, &l) ? l.total : 0;
}

extern "C" int32_t gts_hd95_order_stats_i16(const int16_t* pred, const int16_t* truth, int64_t X, int64_t Y,
                                            int64_t Z, int32_t all_border, int64_t* out, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
  using namespace gts;
  if (!pred || !truth || !out || !workspace) return GTS_ERR_NULL;
  Hd95Layout l;
  if (!hd95_layout(X, Y, Z, &l) || workspace_bytes < l.total) return GTS_ERR_SHAPE;
  if (all_border != 0 && all_border != 1) return GTS_ERR_ARGKIND;
  if (X == 1 && Y == 1 && Z == 1) all_border = 1;  // a lone voxel has no neighbour inside: its own border
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  unsigned* counts = reinterpret_cast<unsigned*>(ws);
  unsigned* hist = reinterpret_cast<unsigned*>(ws + l.hist);
  uint8_t* bits = reinterpret_cast<uint8_t*>(ws + l.bits);
  uint16_t* g1 = reinterpret_cast<uint16_t*>(ws + l.g1);
  int32_t* g2 = reinterpret_cast<int32_t*>(ws + l.g2);
  const int x = static_cast<int>(X), y = static_cast<int>(Y), z = static_cast<int>(Z);
  const size_t n = static_cast<size_t>(l.n);

  if (hipMemsetAsync(ws, 0, l.bits, st) != hipSuccess) return launch_status();
  hd95_border_kernel<<<blocks_for(l.n, kBlock, 2048), kBlock, 0, st>>>(pred, truth, bits, counts, x, y, z, all_border);

  // H2: bytes (1) + distances (2) per element of a line; the distances start 16-byte aligned
  const int lz = lanes_for(3 * Z + 16, kLdsBudget);
  const int n_lines = x * y;
  hd95_pass_z_kernel<<<(n_lines + lz - 1) / lz, kLineLanes, static_cast<size_t>(((lz * z + 15) & ~15) + 2 * lz * z),
                       st>>>(bits, g1, n_lines, z, lz, n);

  const int ly = lanes_for(4 * Y, kLdsBudget);
  hd95_pass_y_kernel<<<dim3((z + ly - 1) / ly, x, kChannels), kLineLanes, static_cast<size_t>(4 * ly * y), st>>>(
      g1, g2, y, z, ly, n);

  const int lx = lanes_for(6 * X, kLdsBudget - 4 * kSmallBins);
  hd95_pass_x_kernel<<<dim3((z + lx - 1) / lx, y, kChannels), kLineLanes,
                       static_cast<size_t>(4 * kSmallBins + 6 * lx * x), st>>>(g2, bits, hist, l.bins, x, y, z, lx,
                                                                               n);

  hd95_select_kernel<<<3, kSelectThreads, 0, st>>>(hist, counts, l.bins, reinterpret_cast<long long*>(out));
  return launch_status();
}
