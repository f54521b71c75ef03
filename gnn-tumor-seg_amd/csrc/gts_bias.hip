// Z1-Z5: remove the bias field (slow multiplicative intensity inhomogeneity) of one MRI volume, N4's scheme
// under this project's own definition (no counterpart in the reference, whose data had it removed).
//
// One modality volume v[Z][Y][X] (x fastest, int16 or float32).  u = float32(log(float64(v))) where v is finite
// and above a threshold, NaN elsewhere; the NaNs of u are the mask of every later pass.  The log field is a sum
// of uniform cubic B-spline lattices, level l with spans = spans0 << l cells and n = spans + 3 control points per
// axis, float64 L_l[c][b][a] (z slowest), the levels one after another in one array.  The HOST tabulates the
// splines per axis (gts/bias.py basis): for index i of an axis of extent N at level l a cell (int32, 0 ..
// spans - 1) and four weights on the control points cell .. cell + 3,
//   weights  float64  x: [levels][4][X], then y: [levels][4][Y], then z: [levels][4][Z]
//   cells    int32    x: [levels][X],    then y: [levels][Y],    then z: [levels][Z]
// so that the kernels only multiply and add, in float64 and without contraction, in one fixed order:
//   field(x, y, z) = sum_l sum_a Bx_a * ( sum_b By_b * ( sum_c Bz_c * L_l[cz + c][cy + b][cx + a] ) )
// every sum ascending from its first term, the levels last.  The two inner sums do not depend on x: a wave
// takes one row (y, z), forms them once as n row coefficients per level in LDS (a lane per coefficient) and then
// spends four multiply-adds per voxel and level, lanes along x.  Same bits as the 64-tap form in that order.
// A cell outside 0 .. spans - 1 is clamped: the tables index nothing outside the lattice.
//
//   Z1 gts_bias_log        u, and the number of mask voxels (integer atomics)
//   Z2 gts_bias_range      min and max of d = float64(u) - field over the mask: one pair per workgroup, then one
//                          workgroup over the pairs.  Exact: min and max do not depend on order.
//   Z3 gts_bias_histogram  counts of bin = clamp(floor((d - lo) / w + 0.5), 0, 199), w = (hi - lo) / 199: uint32
//                          LDS table per workgroup, 64-bit integer global atomics.  Independent of the grid.
//   Z4 gts_bias_fit        r = d - E(d) with E linear between the 200 entries of the sharpened table; Lee's
//                          scattered-data B-spline fit, which factorises: per axis p_a = B_a^3 / sum B^2 and
//                          q_a = B_a^2 (tabulated by the host for the level being fitted, [8][N] per axis),
//                            num[c][b][a] = sum pz_c py_b px_a r,   den[c][b][a] = sum qz_c qy_b qx_a.
//                          Pass A, a wave per row: for each 64-voxel piece of the row and each cell k in it
//                          (ascending) the xor-tree wave sum of px_a r and qx_a over the piece's mask voxels of
//                          that cell, added by lane k + a to its own pair -> [Z][Y][n] pairs.  Pass B, a thread per
//                          (z, b', a'): the rows y ascending.  Pass C, a thread per (c', b', a'): z ascending, then
//                          delta = num / den, 0 where den == 0.  No atomics: which workgroup takes which row is all
//                          the grid decides, so the sums have the same bits on every run and for every grid.
//   Z5 gts_bias_mean       the mask sum of the field per row (wave xor tree), one workgroup over the rows in a
//                          fixed pattern, sum / n.   gts_bias_apply: out = float32(float64(v) / exp(field - m)) at
//                          every voxel, and optionally float32(field - m).
#include <math.h>
#include <stddef.h>

#include <algorithm>

#include "gts_scan.h"

namespace gts {
namespace {

constexpr int kMaxSpans = GTS_BIAS_MAX_SPANS;
constexpr int kMaxLevels = 6;                  // spans0 << (levels - 1) <= 32
constexpr int kMaxCoefs = 96;                  // sum over the levels of spans + 3 <= 63 + 18
constexpr int kBins = GTS_BIAS_BINS;
constexpr int kMaxGrid = 4096;

// The first member of every row kernel's argument struct.
struct Basis {
  const double* wx;
  const double* wy;
  const double* wz;
  const int* cx;
  const int* cy;
  const int* cz;
  const double* lattice;
  int X, Y, Z;
  int spans0, levels;
};

__device__ __forceinline__ int clamp_cell(int c, int spans) { return c < 0 ? 0 : (c < spans ? c : spans - 1); }

// Lanes of one wave: coef[first coefficient of level l + a'] = sum_b By_b (sum_c Bz_c L_l[cz + c][cy + b][a']).
__device__ __forceinline__ void row_coefficients(const Basis& b, int y, int z, int lane, double* coef) {
  int spans = b.spans0, c0 = 0;
  int64_t l0 = 0;
  for (int l = 0; l < b.levels; ++l, spans <<= 1) {
    const int n = spans + 3;
    const int cy = clamp_cell(b.cy[int64_t{l} * b.Y + y], spans), cz = clamp_cell(b.cz[int64_t{l} * b.Z + z], spans);
    double wy[4], wz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wy[k] = b.wy[(int64_t{l} * 4 + k) * b.Y + y];
      wz[k] = b.wz[(int64_t{l} * 4 + k) * b.Z + z];
    }
    for (int a = lane; a < n; a += kWave) {
      const double* L = b.lattice + l0 + (int64_t{cz} * n + cy) * n + a;
      double s = 0.0;
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        double t = wz[0] * L[(int64_t{0} * n + bb) * n];
#pragma unroll
        for (int c = 1; c < 4; ++c) t = t + wz[c] * L[(int64_t{c} * n + bb) * n];
        s = bb == 0 ? wy[0] * t : s + wy[bb] * t;
      }
      coef[c0 + a] = s;
    }
    c0 += n;
    l0 += int64_t{n} * n * n;
  }
}

__device__ __forceinline__ double field_at(const Basis& b, const double* coef, int x) {
  int spans = b.spans0, c0 = 0;
  double f = 0.0;
  for (int l = 0; l < b.levels; ++l, spans <<= 1) {
    const double* c = coef + c0 + clamp_cell(b.cx[int64_t{l} * b.X + x], spans);
    const double* w = b.wx + int64_t{l} * 4 * b.X + x;
    double t = w[0] * c[0];
    t = t + w[b.X] * c[1];
    t = t + w[2 * int64_t{b.X}] * c[2];
    t = t + w[3 * int64_t{b.X}] * c[3];
    f = l == 0 ? t : f + t;
    c0 += spans + 3;
  }
  return f;
}

// row(r, y, z, coef) for every row r = z * Y + y, one wave per row, the wave's row coefficients in LDS.  Every
// thread of the workgroup must call it; inside row() the whole wave is active.
template <typename Row>
__device__ __forceinline__ void for_each_row(const Basis& b, Row&& row) {
  __shared__ double coef[kWavesPerBlock][kMaxCoefs];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t rows = int64_t{b.Y} * b.Z;
  for (int64_t r0 = int64_t{blockIdx.x} * kWavesPerBlock; r0 < rows; r0 += int64_t{gridDim.x} * kWavesPerBlock) {
    const int64_t r = r0 + wave;
    const bool on = r < rows;
    const int y = on ? static_cast<int>(r % b.Y) : 0, z = on ? static_cast<int>(r / b.Y) : 0;
    if (on) row_coefficients(b, y, z, lane, coef[wave]);
    __syncthreads();
    if (on) row(r, y, z, coef[wave]);
    __syncthreads();
  }
}

__device__ __forceinline__ double wave_min(double v) { return wave_reduce(v, [](double a, double b) { return fmin(a, b); }); }
__device__ __forceinline__ double wave_max(double v) { return wave_reduce(v, [](double a, double b) { return fmax(a, b); }); }

// ------------------------------------------------------------------ Z1
template <typename T>
__global__ __launch_bounds__(kBlock) void bias_log_kernel(const T* __restrict__ src, int64_t vol, double threshold,
                                                          float* __restrict__ u,
                                                          unsigned long long* __restrict__ count) {
  unsigned mine[1] = {0};
  for (int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x; i < vol; i += int64_t{gridDim.x} * kBlock) {
    const double v = static_cast<double>(src[i]);
    const bool member = is_finite(v) && v > threshold;
    u[i] = member ? static_cast<float>(log(v)) : __builtin_nanf("");
    mine[0] += member ? 1u : 0u;
  }
  block_add_counters(mine, count);
}

// ------------------------------------------------------------------ Z2
struct RangeArgs {
  Basis b;
  const float* u;
  double* partial;  // [gridDim.x][2]
};

__global__ __launch_bounds__(kBlock) void bias_range_kernel(const RangeArgs p) {
  __shared__ double red[kWavesPerBlock][2];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  double lo = INFINITY, hi = -INFINITY;
  for_each_row(p.b, [&](int64_t r, int, int, const double* coef) {
    const float* __restrict__ u = p.u + r * p.b.X;
    for (int x = lane; x < p.b.X; x += kWave) {
      const float uv = u[x];
      if (uv == uv) {
        const double d = static_cast<double>(uv) - field_at(p.b, coef, x);
        if (d < lo) lo = d;
        if (d > hi) hi = d;
      }
    }
  });
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane == 0) red[wave][0] = lo, red[wave][1] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWavesPerBlock; ++w) lo = fmin(lo, red[w][0]), hi = fmax(hi, red[w][1]);
    p.partial[2 * blockIdx.x] = lo;
    p.partial[2 * blockIdx.x + 1] = hi;
  }
}

__global__ __launch_bounds__(kBlock) void bias_range_final_kernel(const double* __restrict__ partial, int blocks,
                                                                  double* __restrict__ out) {
  __shared__ double red[kWavesPerBlock][2];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  double lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < blocks; i += kBlock) lo = fmin(lo, partial[2 * i]), hi = fmax(hi, partial[2 * i + 1]);
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane == 0) red[wave][0] = lo, red[wave][1] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWavesPerBlock; ++w) lo = fmin(lo, red[w][0]), hi = fmax(hi, red[w][1]);
    out[0] = lo;
    out[1] = hi;
  }
}

// ------------------------------------------------------------------ Z3
struct HistArgs {
  Basis b;
  const float* u;
  unsigned long long* counts;  // [kBins]
  double lo, w;
};

__global__ __launch_bounds__(kBlock) void bias_histogram_kernel(const HistArgs p) {
  __shared__ unsigned hist[kBins];
  block_hist_clear(hist, kBins);
  const int lane = threadIdx.x & (kWave - 1);
  for_each_row(p.b, [&](int64_t r, int, int, const double* coef) {
    const float* __restrict__ u = p.u + r * p.b.X;
    for (int x = lane; x < p.b.X; x += kWave) {
      const float uv = u[x];
      if (uv == uv) {
        const double d = static_cast<double>(uv) - field_at(p.b, coef, x);
        const double q = floor((d - p.lo) / p.w + 0.5);
        atomicAdd(&hist[q >= 1.0 ? (q < static_cast<double>(kBins - 1) ? static_cast<int>(q) : kBins - 1) : 0], 1u);
      }
    }
  });
  block_hist_flush(hist, kBins, p.counts);
}

// ------------------------------------------------------------------ Z4
struct FitArgs {
  Basis b;
  const float* u;
  const double* fx;   // the fitted level's [8][X]: px_0..3, qx_0..3
  double* rowsums;    // [Z][Y][n][2]
  int level;
  double lo, w;
  double table[kBins];  // read with kernarg_entry: the struct is the kernel's only argument
};

__global__ __launch_bounds__(kBlock) void bias_fit_rows_kernel(const FitArgs p) {
  __shared__ double table[kBins];
  for (int i = threadIdx.x; i < kBins; i += kBlock) table[i] = kernarg_entry<double>(offsetof(FitArgs, table), i);
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const int X = p.b.X, spans = p.b.spans0 << p.level, n = spans + 3;
  const int* __restrict__ cells = p.b.cx + int64_t{p.level} * X;
  for_each_row(p.b, [&](int64_t r, int, int, const double* coef) {
    const float* __restrict__ u = p.u + r * X;
    double acc_n = 0.0, acc_d = 0.0;  // control point `lane` of the row
    for (int x0 = 0; x0 < X; x0 += kWave) {
      const int x = x0 + lane;
      bool member = false;
      int cell = 0;
      double pr[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
      if (x < X) {
        const float uv = u[x];
        if (uv == uv) {
          member = true;
          cell = clamp_cell(cells[x], spans);
          const double d = static_cast<double>(uv) - field_at(p.b, coef, x);
          const double pos = (d - p.lo) / p.w, fl = floor(pos);
          const int i0 = fl >= 1.0 ? (fl < static_cast<double>(kBins - 2) ? static_cast<int>(fl) : kBins - 2) : 0;
          const double fr = pos - static_cast<double>(i0);
          const double res = d - (table[i0] + (table[i0 + 1] - table[i0]) * fr);
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            pr[a] = p.fx[int64_t{a} * X + x] * res;
            q[a] = p.fx[int64_t{4 + a} * X + x];
          }
        }
      }
      const int last = x0 + kWave - 1 < X ? x0 + kWave - 1 : X - 1;
      const int k_lo = clamp_cell(cells[x0], spans), k_hi = clamp_cell(cells[last], spans);  // the same in every lane
      for (int k = k_lo; k <= k_hi; ++k) {
        const bool mine = member && cell == k;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const double sn = wave_sum(mine ? pr[a] : 0.0), sd = wave_sum(mine ? q[a] : 0.0);
          if (lane == k + a) acc_n += sn, acc_d += sd;
        }
      }
    }
    if (lane < n) {
      p.rowsums[(r * n + lane) * 2] = acc_n;
      p.rowsums[(r * n + lane) * 2 + 1] = acc_d;
    }
  });
}

// Pass B: ysums[z][b'][a'] = sum over y ascending, b = b' - cell(y) in 0..3, of (py_b N, qy_b D)[z][y][a'].
__global__ __launch_bounds__(kBlock) void bias_fit_y_kernel(const double* __restrict__ rowsums,
                                                            const double* __restrict__ fy,
                                                            const int* __restrict__ cells, int Y, int Z, int spans,
                                                            double* __restrict__ ysums) {
  const int n = spans + 3;
  const int64_t i = int64_t{blockIdx.x} * kBlock + threadIdx.x;
  if (i >= int64_t{Z} * n * n) return;
  const int a = static_cast<int>(i % n), bp = static_cast<int>((i / n) % n);
  const int64_t z = i / (int64_t{n} * n);
  double sn = 0.0, sd = 0.0;
  for (int y = 0; y < Y; ++y) {
    const int b = bp - clamp_cell(cells[y], spans);
    if (b < 0 || b > 3) continue;
    const double* pair = rowsums + ((z * Y + y) * n + a) * 2;
    sn += fy[int64_t{b} * Y + y] * pair[0];
    sd += fy[int64_t{4 + b} * Y + y] * pair[1];
  }
  ysums[2 * i] = sn;
  ysums[2 * i + 1] = sd;
}

// Pass C: out[0] = num, out[1] = den, out[2] = delta, each [n][n][n].
__global__ __launch_bounds__(kBlock) void bias_fit_z_kernel(const double* __restrict__ ysums,
                                                            const double* __restrict__ fz,
                                                            const int* __restrict__ cells, int Z, int spans,
                                                            double* __restrict__ out) {
  const int n = spans + 3;
  const int total = n * n * n;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const int cp = i / (n * n), rest = i - cp * n * n;
  double sn = 0.0, sd = 0.0;
  for (int z = 0; z < Z; ++z) {
    const int c = cp - clamp_cell(cells[z], spans);
    if (c < 0 || c > 3) continue;
    const double* pair = ysums + (int64_t{z} * n * n + rest) * 2;
    sn += fz[int64_t{c} * Z + z] * pair[0];
    sd += fz[int64_t{4 + c} * Z + z] * pair[1];
  }
  out[i] = sn;
  out[total + i] = sd;
  out[2 * total + i] = sd == 0.0 ? 0.0 : sn / sd;
}

// ------------------------------------------------------------------ Z5
struct MeanArgs {
  Basis b;
  const float* u;
  double* partial;  // [rows][2]: the row's sum of the field over its mask voxels, their number
};

__global__ __launch_bounds__(kBlock) void bias_mean_rows_kernel(const MeanArgs p) {
  const int lane = threadIdx.x & (kWave - 1);
  for_each_row(p.b, [&](int64_t r, int, int, const double* coef) {
    const float* __restrict__ u = p.u + r * p.b.X;
    double s = 0.0, c = 0.0;
    for (int x = lane; x < p.b.X; x += kWave) {
      const float uv = u[x];
      if (uv == uv) s += field_at(p.b, coef, x), c += 1.0;
    }
    s = wave_sum(s);
    c = wave_sum(c);
    if (lane == 0) p.partial[2 * r] = s, p.partial[2 * r + 1] = c;
  });
}

// out[0] = sum, out[1] = n, out[2] = sum / n (0 for an empty mask): thread t adds rows t, t + 256, ... ascending,
// then the xor tree per wave, then the four waves in order.
__global__ __launch_bounds__(kBlock) void bias_mean_final_kernel(const double* __restrict__ partial, int64_t rows,
                                                                 double* __restrict__ out) {
  __shared__ double red[kWavesPerBlock][2];
  double s = 0.0, c = 0.0;
  for (int64_t r = threadIdx.x; r < rows; r += kBlock) s += partial[2 * r], c += partial[2 * r + 1];
  s = wave_sum(s);
  c = wave_sum(c);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave][0] = s, red[threadIdx.x / kWave][1] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWavesPerBlock; ++w) s += red[w][0], c += red[w][1];
    out[0] = s;
    out[1] = c;
    out[2] = c > 0.0 ? s / c : 0.0;
  }
}

struct ApplyArgs {
  Basis b;
  const void* src;
  float* out;
  float* field;  // may be null
  double mean;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void bias_apply_kernel(const ApplyArgs p) {
  const int lane = threadIdx.x & (kWave - 1);
  for_each_row(p.b, [&](int64_t r, int, int, const double* coef) {
    const T* __restrict__ src = static_cast<const T*>(p.src) + r * p.b.X;
    for (int x = lane; x < p.b.X; x += kWave) {
      const double f = field_at(p.b, coef, x) - p.mean;
      p.out[r * p.b.X + x] = static_cast<float>(static_cast<double>(src[x]) / exp(f));
      if (p.field) p.field[r * p.b.X + x] = static_cast<float>(f);
    }
  });
}

// ------------------------------------------------------------------ host
struct Layout {
  int64_t partial, rowsums, ysums, total;
};

inline Layout layout(int64_t Y, int64_t Z, int64_t spans) {
  const int64_t n = spans + 3, rows = Y * Z;
  Layout l;
  l.partial = 0;                                        // Z2: [<= rows][2], Z5: [rows][2]
  l.rowsums = round256(std::max<int64_t>(rows, kMaxGrid) * 16);
  l.ysums = l.rowsums + round256(rows * n * 16);
  l.total = l.ysums + round256(Z * n * n * 16);
  return l;
}

inline bool levels_ok(int64_t spans0, int64_t levels) {
  return spans0 >= 1 && levels >= 1 && levels <= kMaxLevels && (spans0 << (levels - 1)) <= kMaxSpans;
}

Basis make_basis(const double* weights, const int32_t* cells, const double* lattice, int64_t X, int64_t Y, int64_t Z,
                 int64_t spans0, int64_t levels) {
  Basis b;
  b.wx = weights;
  b.wy = b.wx + levels * 4 * X;
  b.wz = b.wy + levels * 4 * Y;
  b.cx = cells;
  b.cy = b.cx + levels * X;
  b.cz = b.cy + levels * Y;
  b.lattice = lattice;
  b.X = static_cast<int>(X), b.Y = static_cast<int>(Y), b.Z = static_cast<int>(Z);
  b.spans0 = static_cast<int>(spans0), b.levels = static_cast<int>(levels);
  return b;
}

// workgroups of four rows each: the caller's count, else enough for every row up to kMaxGrid
inline int row_grid(int64_t rows, int64_t grid_blocks) {
  const int64_t groups = (rows + kWavesPerBlock - 1) / kWavesPerBlock;
  return static_cast<int>(std::min<int64_t>(grid_blocks > 0 ? grid_blocks : kMaxGrid, groups));
}

// the checks the row kernels share; GTS_OK when the call may launch
int check_rows(const void* u, const double* weights, const int32_t* cells, const double* lattice, int64_t X, int64_t Y,
               int64_t Z, int64_t spans0, int64_t levels, int64_t grid_blocks) {
  if (!u || !weights || !cells || !lattice) return GTS_ERR_NULL;
  if (!scan_extents_ok(X, Y, Z) || !levels_ok(spans0, levels) || !grid_blocks_ok(grid_blocks))
    return GTS_ERR_SHAPE;
  return GTS_OK;
}

}  // namespace
}  // namespace gts

extern "C" int64_t gts_bias_workspace(int64_t X, int64_t Y, int64_t Z, int64_t spans) {
  using namespace gts;
  if (!scan_extents_ok(X, Y, Z) || spans < 1 || spans > kMaxSpans) return GTS_ERR_SHAPE;
  return layout(Y, Z, spans).total;
}

extern "C" int32_t gts_bias_log(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z, double threshold,
                                float* u, uint64_t* count, void* stream) {
  using namespace gts;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  if (!src || !u || !count) return GTS_ERR_NULL;
  if (!scan_extents_ok(X, Y, Z)) return GTS_ERR_SHAPE;
  if (!is_finite(threshold) || threshold < 0.0) return GTS_ERR_ARGKIND;
  const int64_t vol = X * Y * Z;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(count, 0, 8, st) != hipSuccess) return launch_status();
  auto* cnt = reinterpret_cast<unsigned long long*>(count);
  const int grid = blocks_for(vol, kBlock, kMaxGrid);
  return with_scan_type(dtype, src, [&](auto* s) {
    bias_log_kernel<<<grid, kBlock, 0, st>>>(s, vol, threshold, u, cnt);
    return launch_status();
  });
}

extern "C" int32_t gts_bias_range(const float* u, int64_t X, int64_t Y, int64_t Z, const double* weights,
                                  const int32_t* cells, const double* lattice, int64_t spans0, int64_t levels,
                                  double* range, void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                                  void* stream) {
  using namespace gts;
  const int status = check_rows(u, weights, cells, lattice, X, Y, Z, spans0, levels, grid_blocks);
  if (status != GTS_OK) return status;
  if (!range || !workspace) return GTS_ERR_NULL;
  if (workspace_bytes < layout(Y, Z, spans0 << (levels - 1)).total) return GTS_ERR_SHAPE;
  RangeArgs p;
  p.b = make_basis(weights, cells, lattice, X, Y, Z, spans0, levels);
  p.u = u;
  p.partial = static_cast<double*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = row_grid(Y * Z, grid_blocks);  // <= rows: the pairs fit the workspace's first part
  bias_range_kernel<<<grid, kBlock, 0, st>>>(p);
  bias_range_final_kernel<<<1, kBlock, 0, st>>>(p.partial, grid, range);
  return launch_status();
}

extern "C" int32_t gts_bias_histogram(const float* u, int64_t X, int64_t Y, int64_t Z, const double* weights,
                                      const int32_t* cells, const double* lattice, int64_t spans0, int64_t levels,
                                      double lo, double hi, int64_t* counts, int64_t grid_blocks, void* stream) {
  using namespace gts;
  const int status = check_rows(u, weights, cells, lattice, X, Y, Z, spans0, levels, grid_blocks);
  if (status != GTS_OK) return status;
  if (!counts) return GTS_ERR_NULL;
  const double w = (hi - lo) / static_cast<double>(kBins - 1);
  if (!is_finite(lo) || !is_finite(hi) || !(hi > lo) || !is_finite(w) || !(w > 0.0)) return GTS_ERR_ARGKIND;
  HistArgs p;
  p.b = make_basis(weights, cells, lattice, X, Y, Z, spans0, levels);
  p.u = u;
  p.counts = reinterpret_cast<unsigned long long*>(counts);
  p.lo = lo, p.w = w;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, kBins * sizeof(int64_t), st) != hipSuccess) return launch_status();
  bias_histogram_kernel<<<row_grid(Y * Z, grid_blocks), kBlock, 0, st>>>(p);
  return launch_status();
}

extern "C" int32_t gts_bias_fit(const float* u, int64_t X, int64_t Y, int64_t Z, const double* weights,
                                const int32_t* cells, const double* lattice, int64_t spans0, int64_t levels,
                                int64_t level, const double* fit_weights, double lo, double hi, const double* table,
                                double* out, void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                                void* stream) {
  using namespace gts;
  const int status = check_rows(u, weights, cells, lattice, X, Y, Z, spans0, levels, grid_blocks);
  if (status != GTS_OK) return status;
  if (!fit_weights || !table || !out || !workspace) return GTS_ERR_NULL;
  if (level < 0 || level >= levels) return GTS_ERR_SHAPE;
  const int spans = static_cast<int>(spans0 << level), n = spans + 3;
  const Layout l = layout(Y, Z, spans0 << (levels - 1));
  if (workspace_bytes < l.total) return GTS_ERR_SHAPE;
  FitArgs p;
  p.w = (hi - lo) / static_cast<double>(kBins - 1);
  if (!is_finite(lo) || !is_finite(hi) || !(hi > lo) || !is_finite(p.w) || !(p.w > 0.0)) return GTS_ERR_ARGKIND;
  for (int i = 0; i < kBins; ++i) {
    if (!is_finite(table[i])) return GTS_ERR_ARGKIND;
    p.table[i] = table[i];
  }
  p.b = make_basis(weights, cells, lattice, X, Y, Z, spans0, levels);
  p.u = u;
  p.fx = fit_weights;
  p.level = static_cast<int>(level);
  p.lo = lo;
  char* ws = static_cast<char*>(workspace);
  p.rowsums = reinterpret_cast<double*>(ws + l.rowsums);
  double* ysums = reinterpret_cast<double*>(ws + l.ysums);
  hipStream_t st = static_cast<hipStream_t>(stream);
  bias_fit_rows_kernel<<<row_grid(Y * Z, grid_blocks), kBlock, 0, st>>>(p);
  bias_fit_y_kernel<<<blocks_for(Z * n * n, kBlock), kBlock, 0, st>>>(p.rowsums, fit_weights + 8 * X, p.b.cy + level * Y,
                                                                      p.b.Y, p.b.Z, spans, ysums);
  bias_fit_z_kernel<<<blocks_for(int64_t{n} * n * n, kBlock), kBlock, 0, st>>>(ysums, fit_weights + 8 * X + 8 * Y,
                                                                               p.b.cz + level * Z, p.b.Z, spans, out);
  return launch_status();
}

extern "C" int32_t gts_bias_mean(const float* u, int64_t X, int64_t Y, int64_t Z, const double* weights,
                                 const int32_t* cells, const double* lattice, int64_t spans0, int64_t levels,
                                 double* out, void* workspace, int64_t workspace_bytes, int64_t grid_blocks,
                                 void* stream) {
  using namespace gts;
  const int status = check_rows(u, weights, cells, lattice, X, Y, Z, spans0, levels, grid_blocks);
  if (status != GTS_OK) return status;
  if (!out || !workspace) return GTS_ERR_NULL;
  if (workspace_bytes < layout(Y, Z, spans0 << (levels - 1)).total) return GTS_ERR_SHAPE;
  MeanArgs p;
  p.b = make_basis(weights, cells, lattice, X, Y, Z, spans0, levels);
  p.u = u;
  p.partial = static_cast<double*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  bias_mean_rows_kernel<<<row_grid(Y * Z, grid_blocks), kBlock, 0, st>>>(p);
  bias_mean_final_kernel<<<1, kBlock, 0, st>>>(p.partial, Y * Z, out);
  return launch_status();
}

extern "C" int32_t gts_bias_apply(const void* src, int32_t dtype, int64_t X, int64_t Y, int64_t Z,
                                  const double* weights, const int32_t* cells, const double* lattice, int64_t spans0,
                                  int64_t levels, double mean, float* out, float* field, int64_t grid_blocks,
                                  void* stream) {
  using namespace gts;
  if (!scan_type_ok(dtype)) return GTS_ERR_ARGKIND;
  const int status = check_rows(src, weights, cells, lattice, X, Y, Z, spans0, levels, grid_blocks);
  if (status != GTS_OK) return status;
  if (!out) return GTS_ERR_NULL;
  if (!is_finite(mean)) return GTS_ERR_ARGKIND;
  ApplyArgs p;
  p.b = make_basis(weights, cells, lattice, X, Y, Z, spans0, levels);
  p.src = src;
  p.out = out;
  p.field = field;
  p.mean = mean;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = row_grid(Y * Z, grid_blocks);
  if (dtype == kI16)
    bias_apply_kernel<int16_t><<<grid, kBlock, 0, st>>>(p);
  else
    bias_apply_kernel<float><<<grid, kBlock, 0, st>>>(p);
  return launch_status();
}
