// View evaluation on the device, for gfx950: what `Mapper.gs_eval_offline` (utils/mapper.py:1950-2056)
// and eval/eval_mesh_utils.py (`eval_pair`, `nn_correspondance`) do per evaluated view on the host.
//   view metrics   one streaming pass over the image: per-channel squared-error sums and, under the reference's depth
//                  mask, count, sum |dd| and sum dd^2; fp32 per-block partials, fp64 final sums, one record.
//   back-projection  depth image -> world points (+ colours) in row-major pixel order: flag, scan, scatter.
//   voxel centroids  Open3D `voxel_down_sample`: grid anchored at min - voxel/2, mean of each occupied cell's points in
//                  ascending cell key (x fastest).  Bounds, keys, radix sort (rocPRIM), run heads, one thread per run
//                  summing in fp64 in the sorted (stable = input) order: no atomics, bitwise repeatable.
//   nearest neighbour  dst filed by cell (21 bits per axis, x fastest), radix-sorted, stored as float4 (xyz + index);
//                  one thread per query walks rings of cells, one binary search per (y, z) row.
//   pair reduce    both distance lists -> the sums eval_pair's eleven figures are formed from.
// Every count that a later stage needs stays on the device (`*_dev` arguments: the live length of a buffer whose
// capacity the host knows), so a whole eval_pair call reads one record.  No entry point here allocates, copies or waits.
// Everything is integer / gather / stream work; nothing is shaped for the matrix cores.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "devprim.hpp"

namespace {

namespace devprim = pings::devprim;
using i64 = long long;
using u64 = unsigned long long;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / pings::kWave;
constexpr int kPartBlocks = 512;               // blocks of the bounds / image reductions (grid-stride above that)
constexpr int kAxisBits = 21;                  // cell index bits per axis of a key
constexpr int kAxisCells = 1 << kAxisBits;
constexpr i64 kMaxCount = ((i64)1 << 31) - 1;  // rocPRIM takes int sizes; float4.w carries an index as int bits
constexpr int kMaxRings = 64;
constexpr int kReduceBlock = 1024;
constexpr u64 kPadKey = ~0ull;                 // key of a buffer row past the live count: sorts behind every cell

inline unsigned blocks_for(i64 n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// live rows of a buffer of `cap` rows: the device count when there is one, clamped into [0, cap]
__device__ __forceinline__ i64 live_count(i64 cap, const int64_t* dev) {
  if (!dev) return cap;
  const i64 c = (i64)*dev;
  return c < 0 ? 0 : (c > cap ? cap : c);
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// Exclusive scan of one int per thread over a kBlock workgroup; *total = the workgroup's sum.
__device__ __forceinline__ int block_exclusive_scan(int x, int* total) {
  return pings::block_exclusive_scan<kBlock>(x, total);
}

// ------------------------------------------------------------------ view metrics
constexpr int kViewPart = 8;   // floats per block: 4 channel sums, count, sum |dd|, sum dd^2, pad

struct ViewArgs {
  const float *rgb, *gt, *depth, *gt_depth, *alpha;
  i64 hw;
  int channels, use_alpha;
  float dmin, dmax, amin;
};

__global__ __launch_bounds__(kBlock) void view_partial_kernel(ViewArgs a, float* __restrict__ part) {
  __shared__ float red[kViewPart][kWaves];
  float acc[kViewPart] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (i64 i = (i64)blockIdx.x * kBlock + threadIdx.x; i < a.hw; i += (i64)gridDim.x * kBlock) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < a.channels) {
        const float d = a.rgb[c * a.hw + i] - a.gt[c * a.hw + i];
        acc[c] += d * d;
      }
    }
    if (a.depth) {
      const float r = a.depth[i], g = a.gt_depth[i];
      bool ok = g > a.dmin && r > a.dmin && g < a.dmax && r < a.dmax;      // mapper.py:1969, all strict
      if (a.use_alpha) ok = ok && a.alpha[i] > a.amin;                    // :1972
      if (ok) {
        const float e = fabsf(g - r);
        acc[4] += 1.f;
        acc[5] += e;
        acc[6] += e * e;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kViewPart; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < kViewPart) {
    float s = red[threadIdx.x][0];
    for (int w = 1; w < kWaves; ++w) s += red[threadIdx.x][w];
    part[(i64)blockIdx.x * kViewPart + threadIdx.x] = s;
  }
}

// one workgroup: the partials summed in fp64 in a fixed order, then the record
__global__ __launch_bounds__(kBlock) void view_finish_kernel(const float* __restrict__ part, int nblocks, ViewArgs a,
                                                             const float* __restrict__ ssim,
                                                             double* __restrict__ rec) {
  __shared__ double red[kViewPart][kWaves];
  double acc[kViewPart];
#pragma unroll
  for (int k = 0; k < kViewPart; ++k) acc[k] = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += kBlock) {
#pragma unroll
    for (int k = 0; k < kViewPart; ++k) acc[k] += (double)part[(i64)b * kViewPart + k];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kViewPart; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot[kViewPart];
  for (int k = 0; k < kViewPart; ++k) {
    tot[k] = red[k][0];
    for (int w = 1; w < kWaves; ++w) tot[k] += red[k][w];
  }
  double psnr = 0.0;
  for (int c = 0; c < 4; ++c) {
    const double mse = c < a.channels ? tot[c] / (double)a.hw : NAN;
    rec[5 + c] = mse;
    if (c < a.channels) psnr += 20.0 * log10(1.0 / sqrt(mse));           // utils/loss.py psnr; mse 0 -> inf
  }
  rec[0] = psnr / (double)a.channels;
  rec[1] = ssim ? (double)*ssim : NAN;
  const double n = tot[4];
  rec[2] = a.depth ? tot[5] / n : NAN;                                    // np.mean of an empty array: 0 / 0 = NaN
  rec[3] = a.depth ? sqrt(tot[6] / n) : NAN;
  rec[4] = n;
}

// ------------------------------------------------------------------ back-projection
struct BpArgs {
  const float *depth, *rgb, *alpha;
  i64 hw;
  int width, use_alpha;
  double fx, fy, cx, cy, trunc;
  double T[12];     // camera -> world, rows of [R | t]
  float amin;
};

__device__ __forceinline__ bool bp_keep(const BpArgs& a, i64 i) {
  if (i >= a.hw) return false;
  const double d = (double)a.depth[i];
  bool ok = d > 0.0 && d < a.trunc;                   // Open3D: >= depth_trunc becomes 0, 0 gives no point
  if (a.use_alpha) ok = ok && a.alpha[i] > a.amin;    // the reference's rendered_depth[~accu_alpha_mask] = 0
  return ok;
}

__global__ __launch_bounds__(kBlock) void bp_count_kernel(BpArgs a, int* __restrict__ cnt) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  int tot;
  block_exclusive_scan(bp_keep(a, i) ? 1 : 0, &tot);
  if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void bp_emit_kernel(BpArgs a, const int* __restrict__ off, int nb,
                                                         float* __restrict__ points, float* __restrict__ colors,
                                                         int64_t* __restrict__ count) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  const bool keep = bp_keep(a, i);
  int tot;
  const int r0 = block_exclusive_scan(keep ? 1 : 0, &tot);
  if (i == 0) *count = (int64_t)off[nb - 1];
  if (!keep) return;
  const i64 o = (i64)(blockIdx.x ? off[blockIdx.x - 1] : 0) + r0;        // o < kept total <= hw
  const double z = (double)a.depth[i];
  const double u = (double)(i % a.width), v = (double)(i / a.width);
  const double x = (u - a.cx) * z / a.fx, y = (v - a.cy) * z / a.fy;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    points[3 * o + r] = (float)(a.T[4 * r] * x + a.T[4 * r + 1] * y + a.T[4 * r + 2] * z + a.T[4 * r + 3]);
  if (colors) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // (rgb * 255).byte() / 255: truncation of the fp32 product, then Open3D's uint8 / 255.0
      const float b = fminf(fmaxf(floorf(a.rgb[c * a.hw + i] * 255.f), 0.f), 255.f);
      colors[3 * o + c] = (float)((double)b / 255.0);
    }
  }
}

// ------------------------------------------------------------------ cell grid shared by the centroids and the search
struct Part {
  float mn[3], mx[3];
};

struct GridInfo {
  double lo[3], hi[3];   // lo: origin of cell 0 per axis; hi: largest coordinate
  int dim[3];            // cells per axis (>= 1 when cnt > 0)
  int overflow;          // the extent does not fit kAxisBits per axis
  i64 cnt;               // live points
};

// C: floats per row of the cloud (3: positions; 6: positions and colours).  Cells come from the first three.
template <int C>
__global__ __launch_bounds__(kBlock) void bounds_kernel(const float* __restrict__ pts, i64 cap,
                                                        const int64_t* __restrict__ n_dev, Part* __restrict__ partial) {
  __shared__ float red[6][kWaves];
  const i64 n = live_count(cap, n_dev);
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (i64 i = (i64)blockIdx.x * kBlock + threadIdx.x; i < n; i += (i64)gridDim.x * kBlock) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = pts[C * i + a];
      v[a] = fminf(v[a], x);
      v[3 + a] = fmaxf(v[3 + a], x);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    float x = v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float y = __shfl_xor(x, off, 64);
      x = k < 3 ? fminf(x, y) : fmaxf(x, y);
    }
    if (lane == 0) red[k][wave] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Part p;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      float x = red[k][0];
      for (int w = 1; w < kWaves; ++w) x = k < 3 ? fminf(x, red[k][w]) : fmaxf(x, red[k][w]);
      if (k < 3) p.mn[k] = x; else p.mx[k - 3] = x;
    }
    partial[blockIdx.x] = p;
  }
}

// cell index of coordinate x on one axis, as a double (floor of the fp64 quotient, as Open3D forms it)
__device__ __forceinline__ double cell_of(float x, double lo, double cell) { return floor(((double)x - lo) / cell); }

// one thread: the grid of the live points.  shift = 0.5 anchors it half a cell below the minimum (voxel_down_sample).
__global__ void grid_info_kernel(const Part* __restrict__ partial, int nblocks, i64 cap,
                                 const int64_t* __restrict__ n_dev, double cell, double shift,
                                 GridInfo* __restrict__ info, int32_t* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Part b = partial[0];
  for (int i = 1; i < nblocks; ++i) {
    const Part c = partial[i];
    for (int a = 0; a < 3; ++a) {
      b.mn[a] = fminf(b.mn[a], c.mn[a]);
      b.mx[a] = fmaxf(b.mx[a], c.mx[a]);
    }
  }
  GridInfo gi;
  gi.cnt = live_count(cap, n_dev);
  gi.overflow = 0;
  for (int a = 0; a < 3; ++a) {
    gi.lo[a] = (double)b.mn[a] - shift * cell;
    gi.hi[a] = (double)b.mx[a];
    const double top = cell_of(b.mx[a], gi.lo[a], cell);        // NaN / inf when there is no finite point
    int d = 1;
    if (top >= 0.0 && top < (double)kAxisCells) d = (int)top + 1;
    else if (top >= (double)kAxisCells) { d = kAxisCells; gi.overflow = 1; }
    gi.dim[a] = d;
  }
  *info = gi;
  if (gi.overflow) *status = *status | PINGS_EVAL_EXTENT;       // this thread is the only writer in this launch
}

__device__ __forceinline__ u64 make_key(int x, int y, int z) {
  return (u64)x | (u64)y << kAxisBits | (u64)z << (2 * kAxisBits);
}

// cell of a filed point: clamped into the grid (a NaN coordinate files into cell 0; it never wins a comparison)
__device__ __forceinline__ int filed_cell(float x, double lo, double cell, int dim) {
  const double t = cell_of(x, lo, cell);
  return (int)fmin(fmax(t, 0.0), (double)(dim - 1));
}

template <int C>
__global__ __launch_bounds__(kBlock) void key_kernel(const float* __restrict__ pts, i64 cap,
                                                     const GridInfo* __restrict__ info, double cell,
                                                     u64* __restrict__ key, uint32_t* __restrict__ val) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cap) return;
  u64 k = kPadKey;
  if (i < info->cnt) {
    const int x = filed_cell(pts[C * i], info->lo[0], cell, info->dim[0]);
    const int y = filed_cell(pts[C * i + 1], info->lo[1], cell, info->dim[1]);
    const int z = filed_cell(pts[C * i + 2], info->lo[2], cell, info->dim[2]);
    k = make_key(x, y, z);
  }
  key[i] = k;
  val[i] = (uint32_t)i;
}

struct GridScratch {
  Part* partial;
  GridInfo* info;
  u64 *key, *key_sorted;
  uint32_t *val, *val_sorted;
  float4* pts4;                 // search only
  int *flag, *rank, *start;     // centroids only
  i64* cells;                   // centroids only: occupied cells
  void* temp;
  size_t temp_bytes, total;
};

GridScratch carve_grid(void* base, i64 cap, bool search) {
  pings::Carver c(base);
  GridScratch s{};
  const size_t n = (size_t)cap;
  s.partial = c.take<Part>(kPartBlocks);
  s.info = c.take<GridInfo>(1);
  s.key = c.take<u64>(n);
  s.key_sorted = c.take<u64>(n);
  s.val = c.take<uint32_t>(n);
  s.val_sorted = c.take<uint32_t>(n);
  s.temp_bytes = devprim::sort_pairs_u64_u32_temp_bytes(cap);
  if (search) {
    s.pts4 = c.take<float4>(n);
  } else {
    s.flag = c.take<int>(n);
    s.rank = c.take<int>(n);
    s.start = c.take<int>(n);
    s.cells = c.take<i64>(1);
    s.temp_bytes = std::max(s.temp_bytes, devprim::inclusive_sum_i32_temp_bytes(cap));   // the scan follows the sort
  }
  s.temp_bytes = pings::align_up(s.temp_bytes);
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

// bounds, grid, keys and the sort by key: the front of both pipelines
template <int C = 3>
int file_points(const float* pts, i64 cap, const int64_t* n_dev, double cell, double shift, const GridScratch& s,
                int32_t* status, hipStream_t st) {
  const int nb = (int)std::min<i64>(kPartBlocks, (cap + kBlock - 1) / kBlock);
  bounds_kernel<C><<<nb, kBlock, 0, st>>>(pts, cap, n_dev, s.partial);
  PINGS_LAUNCH_CHECK();
  grid_info_kernel<<<1, 64, 0, st>>>(s.partial, nb, cap, n_dev, cell, shift, s.info, status);
  PINGS_LAUNCH_CHECK();
  key_kernel<C><<<blocks_for(cap), kBlock, 0, st>>>(pts, cap, s.info, cell, s.key, s.val);
  PINGS_LAUNCH_CHECK();
  return devprim::sort_pairs_u64_u32(s.temp, s.temp_bytes, s.key, s.key_sorted, s.val, s.val_sorted, cap, 0, 64, st);
}

// ------------------------------------------------------------------ voxel centroids
__global__ __launch_bounds__(kBlock) void vc_heads_kernel(const u64* __restrict__ ks, i64 cap,
                                                          const GridInfo* __restrict__ info, int* __restrict__ flag) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cap) return;
  flag[i] = (i < info->cnt && (i == 0 || ks[i] != ks[i - 1])) ? 1 : 0;
}

// rows already in `out` (0 without a device offset), clamped into [0, out_cap]
__device__ __forceinline__ i64 rows_before(const int64_t* offset, i64 out_cap) {
  return offset ? live_count(out_cap, offset) : 0;
}

// *count = rows in `out` after this call: the rows before it plus the occupied cells, at most out_cap (then `full`, when
// it is not 0, is or-ed into *status: this thread is the only writer in this launch)
__global__ __launch_bounds__(kBlock) void vc_starts_kernel(const int* __restrict__ flag, const int* __restrict__ rank,
                                                           i64 cap, const GridInfo* __restrict__ info,
                                                           int* __restrict__ start, const int64_t* __restrict__ offset,
                                                           i64 out_cap, i64* __restrict__ cells,
                                                           int64_t* __restrict__ count, int32_t* __restrict__ status,
                                                           int full) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cap) return;
  if (flag[i]) start[rank[i] - 1] = (int)i;          // rank = inclusive sum of the flags: 1 <= rank <= cap
  if (i == cap - 1) {                                // rank[i]: occupied cells (0 when there is no live point)
    *cells = (i64)rank[i];
    const i64 total = rows_before(offset, out_cap) + (i64)rank[i];
    if (total > out_cap && full) *status = *status | full;
    *count = (int64_t)(total > out_cap ? out_cap : total);
  }
}

// one thread per occupied cell: the mean of its points over all C columns, summed in fp64 in sorted order (a stable
// sort: input order); cell r becomes row (rows before this call) + r of `out`
template <int C>
__global__ __launch_bounds__(kBlock) void vc_mean_kernel(const float* __restrict__ pts, const uint32_t* __restrict__ vs,
                                                         const int* __restrict__ start, i64 cap,
                                                         const GridInfo* __restrict__ info,
                                                         const i64* __restrict__ cells,
                                                         const int64_t* __restrict__ offset, i64 out_cap,
                                                         float* __restrict__ out) {
  const i64 r = (i64)blockIdx.x * kBlock + threadIdx.x;
  const i64 base = rows_before(offset, out_cap);
  const i64 runs = *cells;                                                  // <= cap
  if (r >= runs || base + r >= out_cap) return;                             // a cell that finds no room is dropped
  const i64 cnt = info->cnt > cap ? cap : info->cnt;
  const i64 b = start[r], e = r + 1 < runs ? (i64)start[r + 1] : cnt;
  double s[C];
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = 0.0;
  for (i64 j = b; j < e; ++j) {                      // e <= cnt <= cap
    const i64 p = (i64)vs[j];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] += (double)pts[C * p + c];
  }
  const double inv = 1.0 / (double)(e - b);
#pragma unroll
  for (int c = 0; c < C; ++c) out[C * (base + r) + c] = (float)(s[c] * inv);
}

// ------------------------------------------------------------------ nearest neighbour
__global__ __launch_bounds__(kBlock) void nn_pack_kernel(const float* __restrict__ pts, const uint32_t* __restrict__ vs,
                                                         i64 cap, const GridInfo* __restrict__ info,
                                                         float4* __restrict__ out) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cap || i >= info->cnt) return;
  const i64 p = (i64)vs[i];
  out[i] = make_float4(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], __int_as_float((int)p));
}

struct Best {
  float d2;
  int idx;
};

// the cells xa..xb of row (y, z): one contiguous key range of the sorted array
__device__ __forceinline__ void scan_row(const u64* __restrict__ keys, const float4* __restrict__ pts, i64 m, int dimx,
                                         int xa, int xb, int y, int z, float qx, float qy, float qz, Best& best) {
  xa = xa < 0 ? 0 : xa;
  xb = xb > dimx - 1 ? dimx - 1 : xb;
  if (xa > xb) return;
  const u64 klo = make_key(xa, y, z), khi = make_key(xb, y, z);
  i64 lo = 0, hi = m;
  for (int s = 0; s < 32 && lo < hi; ++s) {          // m < 2^31: at most 31 halvings
    const i64 mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < klo) lo = mid + 1;
    else hi = mid;
  }
  for (i64 j = lo; j < m; ++j) {
    if (keys[j] > khi) break;
    const float4 p = pts[j];
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const int id = __float_as_int(p.w);
    if (d2 < best.d2 || (d2 == best.d2 && id < best.idx)) {
      best.d2 = d2;
      best.idx = id;
    }
  }
}

constexpr float kSlack = 1.f - 2e-5f;   // on the ring bound: covers the rounding of cell indices and of fp32 distances

__global__ __launch_bounds__(kBlock) void nn_query_kernel(const float* __restrict__ src, i64 ncap,
                                                          const int64_t* __restrict__ n_dev,
                                                          const GridInfo* __restrict__ info,
                                                          const u64* __restrict__ keys, const float4* __restrict__ pts,
                                                          i64 mcap, double cell, float max_dist, int rings,
                                                          float* __restrict__ dist, int64_t* __restrict__ idx) {
  const i64 i = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ncap) return;
  float out_d = INFINITY;
  i64 out_i = -1;
  const i64 n = live_count(ncap, n_dev);
  const i64 m = info->cnt > mcap ? mcap : info->cnt;
  if (info->overflow) {
    out_d = NAN;                                      // the grid could not be built: no distance is valid
    out_i = -2;
  } else if (i < n && m > 0) {
    const float q[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
    double box2 = 0.0;
    int qc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double x = (double)q[a], lo = info->lo[a], hi = info->hi[a];
      const double e = x < lo ? lo - x : (x > hi ? x - hi : 0.0);
      box2 += e * e;
      // a query within max_dist of the box lies within `rings` cells of it; the clamp only guards the conversion
      const double t = cell_of(q[a], lo, cell);
      qc[a] = (int)fmin(fmax(t, -(double)(rings + 1)), (double)(info->dim[a] + rings));
    }
    if (box2 < (double)max_dist * (double)max_dist) {                    // false for a NaN query too
      const int dimx = info->dim[0], dimy = info->dim[1], dimz = info->dim[2];
      const float c = (float)cell;
      const float md2 = max_dist * max_dist;
      Best best{INFINITY, 0x7FFFFFFF};
      for (int r = 0; r <= rings; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
          const int z = qc[2] + dz;
          if (z < 0 || z >= dimz) continue;
          for (int dy = -r; dy <= r; ++dy) {
            const int y = qc[1] + dy;
            if (y < 0 || y >= dimy) continue;
            const int ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
            // every point of this row is at least this far away in y and z
            const float gy = (float)(ay > 0 ? ay - 1 : 0) * c, gz = (float)(az > 0 ? az - 1 : 0) * c;
            const float row2 = (gy * gy + gz * gz) * kSlack;
            if (row2 > best.d2 || row2 >= md2) continue;
            if (ay == r || az == r) {
              scan_row(keys, pts, m, dimx, qc[0] - r, qc[0] + r, y, z, q[0], q[1], q[2], best);
            } else {                                                     // an inner row: only its two end cells are new
              scan_row(keys, pts, m, dimx, qc[0] - r, qc[0] - r, y, z, q[0], q[1], q[2], best);
              scan_row(keys, pts, m, dimx, qc[0] + r, qc[0] + r, y, z, q[0], q[1], q[2], best);
            }
          }
        }
        // every point not yet seen is at least r cells away on some axis
        const float lim = (float)r * c * kSlack;
        if (best.d2 <= lim * lim) break;
      }
      const float d = sqrtf(best.d2);
      if (best.idx != 0x7FFFFFFF && d < max_dist) {
        out_d = d;
        out_i = (i64)best.idx;
      }
    }
  }
  dist[i] = out_d;
  idx[i] = (int64_t)out_i;
}

// ------------------------------------------------------------------ pair reduce
// one workgroup, fixed order: {kept, sum d, sum d^2, inliers} of the precision side, then of the recall side
__global__ __launch_bounds__(kReduceBlock) void pair_reduce_kernel(const float* __restrict__ dp, i64 pcap,
                                                                   const int64_t* __restrict__ p_dev,
                                                                   const float* __restrict__ dr, i64 rcap,
                                                                   const int64_t* __restrict__ r_dev, double thr,
                                                                   double tcom, const int32_t* __restrict__ status,
                                                                   double* __restrict__ rec) {
  __shared__ double red[8][kReduceBlock / pings::kWave];
  const i64 np = live_count(pcap, p_dev), nr = live_count(rcap, r_dev);
  double acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.0;
  for (i64 i = threadIdx.x; i < np; i += kReduceBlock) {
    const double d = (double)dp[i];
    if (d < INFINITY) {                               // an outlier (no neighbour below truncation_acc) is dropped
      acc[0] += 1.0;
      acc[1] += d;
      acc[2] += d * d;
      acc[3] += d < thr ? 1.0 : 0.0;
    }
  }
  for (i64 i = threadIdx.x; i < nr; i += kReduceBlock) {
    double d = (double)dr[i];
    if (!(d < INFINITY)) d = tcom;                    // an outlier counts with the truncation distance
    acc[4] += 1.0;
    acc[5] += d;
    acc[6] += d * d;
    acc[7] += d < thr ? 1.0 : 0.0;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < 8; ++k) {
      double s = red[k][0];
      for (int w = 1; w < kReduceBlock / pings::kWave; ++w) s += red[k][w];
      rec[k] = s;
    }
    rec[8] = (double)np;
    rec[9] = (double)nr;
    rec[10] = status ? (double)*status : 0.0;
    rec[11] = 0.0;
  }
}

bool count_ok(int64_t n) { return n > 0 && n <= kMaxCount; }

// the centroids of a cloud of C floats per row, appended to `out` behind *offset rows (0 without one)
template <int C>
int voxel_means(const float* points, int64_t n, const int64_t* n_dev, double voxel, void* scratch, float* out,
                const int64_t* offset, int64_t out_cap, int64_t* count, int32_t* status, int full, hipStream_t st) {
  const GridScratch s = carve_grid(scratch, n, false);
  if (int e = file_points<C>(points, n, n_dev, voxel, 0.5, s, status, st)) return e;
  vc_heads_kernel<<<blocks_for(n), kBlock, 0, st>>>(s.key_sorted, n, s.info, s.flag);
  PINGS_LAUNCH_CHECK();
  if (int e = devprim::inclusive_sum_i32(s.temp, s.temp_bytes, s.flag, s.rank, n, st)) return e;
  vc_starts_kernel<<<blocks_for(n), kBlock, 0, st>>>(s.flag, s.rank, n, s.info, s.start, offset, out_cap, s.cells, count,
                                                     status, full);
  PINGS_LAUNCH_CHECK();
  vc_mean_kernel<C><<<blocks_for(n), kBlock, 0, st>>>(points, s.val_sorted, s.start, n, s.info, s.cells, offset, out_cap,
                                                      out);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

struct BpScratch {
  int *cnt, *off;   // per block: points kept, their inclusive scan
  void* temp;
  size_t temp_bytes, total;
};
BpScratch carve_backproject(void* base, i64 hw) {
  pings::Carver c(base);
  BpScratch s;
  const size_t nb = (size_t)blocks_for(hw);
  s.cnt = c.take<int>(nb);
  s.off = c.take<int>(nb);
  s.temp_bytes = devprim::inclusive_sum_i32_temp_bytes((i64)nb);
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}

}  // namespace

PINGS_API size_t pings_eval_view_metrics_scratch_bytes(int64_t hw) {
  if (hw <= 0) return 0;
  return pings::align_up(sizeof(float) * kViewPart * kPartBlocks);
}

PINGS_API int pings_eval_view_metrics(const float* rgb, const float* gt, int channels, int64_t hw, const float* depth,
                                      const float* gt_depth, const float* alpha, float depth_min, float depth_max,
                                      float min_alpha, int use_alpha, const float* ssim, void* scratch, double* record,
                                      void* stream) {
  PINGS_ARG_CHECK(rgb && gt && scratch && record, "null pointer");
  PINGS_ARG_CHECK((depth == nullptr) == (gt_depth == nullptr), "null pointer: depth and gt_depth come together");
  PINGS_ARG_CHECK(!use_alpha || (alpha && depth), "null pointer: use_alpha needs alpha and depth");
  PINGS_ARG_CHECK(channels >= 1 && channels <= 4, "1 to 4 channels");
  PINGS_ARG_CHECK(hw > 0 && hw <= ((int64_t)1 << 40), "empty or oversized image");
  hipStream_t st = pings::as_stream(stream);
  const ViewArgs a{rgb, gt, depth, gt_depth, alpha, hw, channels, use_alpha ? 1 : 0, depth_min, depth_max, min_alpha};
  float* part = static_cast<float*>(scratch);
  const int nb = (int)std::min<i64>(kPartBlocks, (hw + kBlock - 1) / kBlock);
  pings::prof::Scope sc("eval_view_metrics", st);
  view_partial_kernel<<<nb, kBlock, 0, st>>>(a, part);
  PINGS_LAUNCH_CHECK();
  view_finish_kernel<<<1, kBlock, 0, st>>>(part, nb, a, ssim, record);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API size_t pings_eval_backproject_scratch_bytes(int64_t hw) {
  return count_ok(hw) ? carve_backproject(nullptr, hw).total : 0;
}

PINGS_API int pings_eval_backproject(const float* depth, const float* rgb, const float* alpha, int height, int width,
                                     const double* intrinsic, const double* cam_to_world, double depth_trunc,
                                     float min_alpha, int use_alpha, void* scratch, float* points, float* colors,
                                     int64_t* count, void* stream) {
  PINGS_ARG_CHECK(depth && intrinsic && cam_to_world && scratch && points && count, "null pointer");
  PINGS_ARG_CHECK((rgb == nullptr) == (colors == nullptr), "null pointer: rgb and colors come together");
  PINGS_ARG_CHECK(!use_alpha || alpha, "null pointer: use_alpha needs alpha");
  PINGS_ARG_CHECK(height > 0 && width > 0 && count_ok((int64_t)height * width), "empty or oversized image");
  PINGS_ARG_CHECK(intrinsic[0] != 0.0 && intrinsic[1] != 0.0, "zero focal length");
  hipStream_t st = pings::as_stream(stream);
  BpArgs a{};
  a.depth = depth; a.rgb = rgb; a.alpha = alpha;
  a.hw = (i64)height * width;
  a.width = width;
  a.use_alpha = use_alpha ? 1 : 0;
  a.fx = intrinsic[0]; a.fy = intrinsic[1]; a.cx = intrinsic[2]; a.cy = intrinsic[3];
  a.trunc = depth_trunc;
  for (int k = 0; k < 12; ++k) a.T[k] = cam_to_world[k];
  a.amin = min_alpha;
  const int nb = (int)blocks_for(a.hw);
  const BpScratch s = carve_backproject(scratch, a.hw);
  pings::prof::Scope sc("eval_backproject", st);
  bp_count_kernel<<<nb, kBlock, 0, st>>>(a, s.cnt);
  PINGS_LAUNCH_CHECK();
  if (int e = devprim::inclusive_sum_i32(s.temp, s.temp_bytes, s.cnt, s.off, nb, st)) return e;
  bp_emit_kernel<<<nb, kBlock, 0, st>>>(a, s.off, nb, points, colors, count);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API size_t pings_eval_voxel_scratch_bytes(int64_t n) {
  return count_ok(n) ? carve_grid(nullptr, n, false).total : 0;
}

PINGS_API int pings_eval_voxel_centroids(const float* points, int64_t n, const int64_t* n_dev, double voxel,
                                         void* scratch, float* out, int64_t* count, int32_t* status, void* stream) {
  PINGS_ARG_CHECK(points && scratch && out && count && status, "null pointer");
  PINGS_ARG_CHECK(count_ok(n), "empty or oversized cloud");
  PINGS_ARG_CHECK(voxel > 0.0 && std::isfinite(voxel), "voxel size must be positive");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("eval_voxel_centroids", st);
  return voxel_means<3>(points, n, n_dev, voxel, scratch, out, nullptr, n, count, status, 0, st);
}

// The coloured voxel average of the camera front-end lives here, with the kernels it instantiates.
PINGS_API size_t pings_camfront_voxel_scratch_bytes(int64_t n) { return pings_eval_voxel_scratch_bytes(n); }

PINGS_API int pings_camfront_voxel_average(const float* rows, int64_t n, const int64_t* n_dev, double voxel,
                                           void* scratch, float* out, int64_t out_cap, const int64_t* offset,
                                           int64_t* count, int32_t* status, void* stream) {
  PINGS_ARG_CHECK(rows && scratch && out && count && status, "null pointer");
  PINGS_ARG_CHECK(offset != count, "offset and count must be different words");
  PINGS_ARG_CHECK(count_ok(n) && out_cap > 0 && out_cap <= kMaxCount, "empty or oversized cloud");
  PINGS_ARG_CHECK(voxel > 0.0 && std::isfinite(voxel), "voxel size must be positive");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("camfront_voxel_average", st);
  return voxel_means<6>(rows, n, n_dev, voxel, scratch, out, offset, out_cap, count, status, PINGS_CAMFRONT_FULL, st);
}

PINGS_API size_t pings_eval_nn_scratch_bytes(int64_t m) {
  return count_ok(m) ? carve_grid(nullptr, m, true).total : 0;
}

PINGS_API int pings_eval_nn_build(const float* dst, int64_t m, const int64_t* m_dev, double cell, void* scratch,
                                  int32_t* status, void* stream) {
  PINGS_ARG_CHECK(dst && scratch && status, "null pointer");
  PINGS_ARG_CHECK(count_ok(m), "empty or oversized cloud");
  PINGS_ARG_CHECK(cell > 0.0 && std::isfinite(cell), "cell size must be positive");
  hipStream_t st = pings::as_stream(stream);
  const GridScratch s = carve_grid(scratch, m, true);
  pings::prof::Scope sc("eval_nn_build", st);
  if (int e = file_points(dst, m, m_dev, cell, 0.0, s, status, st)) return e;
  nn_pack_kernel<<<blocks_for(m), kBlock, 0, st>>>(dst, s.val_sorted, m, s.info, s.pts4);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_eval_nn_query(const float* src, int64_t n, const int64_t* n_dev, const void* scratch, int64_t m,
                                  double cell, double max_dist, float* dist, int64_t* idx, void* stream) {
  PINGS_ARG_CHECK(src && scratch && dist && idx, "null pointer");
  PINGS_ARG_CHECK(count_ok(n) && count_ok(m), "empty or oversized cloud");
  PINGS_ARG_CHECK(cell > 0.0 && std::isfinite(cell), "cell size must be positive");
  PINGS_ARG_CHECK(max_dist > 0.0 && std::isfinite(max_dist), "max_dist must be positive and finite");
  const double rings = std::ceil(max_dist / cell);
  PINGS_ARG_CHECK(rings <= (double)kMaxRings, "max_dist spans too many cells: use a larger cell");
  hipStream_t st = pings::as_stream(stream);
  const GridScratch s = carve_grid(const_cast<void*>(scratch), m, true);
  pings::prof::Scope sc("eval_nn_query", st);
  nn_query_kernel<<<blocks_for(n), kBlock, 0, st>>>(src, n, n_dev, s.info, s.key_sorted, s.pts4, m, cell,
                                                    (float)max_dist, (int)rings, dist, idx);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_eval_pair_reduce(const float* dist_p, int64_t np, const int64_t* np_dev, const float* dist_r,
                                     int64_t nr, const int64_t* nr_dev, double threshold, double truncation_com,
                                     const int32_t* status, double* record, void* stream) {
  PINGS_ARG_CHECK(dist_p && dist_r && record, "null pointer");
  PINGS_ARG_CHECK(count_ok(np) && count_ok(nr), "empty or oversized list");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("eval_pair_reduce", st);
  pair_reduce_kernel<<<1, kReduceBlock, 0, st>>>(dist_p, np, np_dev, dist_r, nr, nr_dev, threshold, truncation_com,
                                                 status, record);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}
