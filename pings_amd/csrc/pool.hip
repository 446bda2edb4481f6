// SDF training-sample pool on the device, for gfx950.
//
// Restates what the reference does in plain torch around the mapper's sample pool:
//   pool_sample     DataSampler.sample (utils/data_sampler.py:18-264): the measured point, the close-to-surface
//                   samples, the free-space samples in front of and behind the surface, written ray-wise
//                   (row = p * S + s) in ONE launch, one thread per output row, fp32 op for op.
//   pool_draw       the index chain and the row gathers of Mapper.get_batch (utils/mapper.py:704-771) in one launch.
//   pool_transform  Mapper.transform_data_pool (utils/mapper.py:774-778, utils/tools.py:903-921): p <- R[ts] p + t[ts]
//                   in place, without the [N,4,4] gather; pool_ts_range gives the caller min / max of ts beforehand.
//   pool_window     the sample window of process_frame (utils/mapper.py:429-438): ascending rows with
//                   |p - origin| < radius.  Per-wave counts, a one-wave scan of the counts, one read-back, per-wave
//                   ballot compaction: no [N] temporary, every write bounded by the caller's capacity.
// All kernels are HBM-stream / gather bound.  No float atomics and no LDS: waves never hand values to each other,
// so every result is bitwise reproducible.
#include <climits>

#include "common.hpp"

namespace {

using i64 = long long;
using u64 = unsigned long long;

inline unsigned blocks_for(i64 n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

// ------------------------------------------------------------------ sampler
struct SampleK {
  pings_pool_sample_args a;
  // python-side scalar products, formed in double and rounded once (as torch does with python scalars)
  float range, two_sigma, front_min, end_dist, dw_base, dw_scale, max_range, drop_max, drop_diff;
};

__global__ __launch_bounds__(256) void pool_sample_kernel(SampleK k) {
  const pings_pool_sample_args& a = k.a;
  const int ns = a.surface_sample_n, nf = a.free_front_n, nb = a.free_behind_n;
  const i64 S = (i64)ns + nf + nb + 1;
  const i64 row = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.P * S) return;
  const i64 p = row / S;
  const int s = (int)(row - p * S);
  const float x = a.points[3 * p], y = a.points[3 * p + 1], z = a.points[3 * p + 2];
  const float dist = sqrtf((x * x + y * y) + z * z);          // torch.linalg.norm(points, dim=1)
  float disp, ratio;
  if (s == 0) {                                                // Part 0: the measured point
    disp = 0.f;
    ratio = 1.f;
  } else if (s <= ns) {                                        // Part 1: close to the surface (:50-58)
    disp = a.noise_surface[(i64)(s - 1) * a.P + p] * k.range;
    ratio = disp / dist + 1.0f;
  } else if (s <= ns + nf) {                                   // Part 2: free space in front (:74-85)
    const float free_max = 1.0f - k.two_sigma / dist;
    const float diff = free_max - k.front_min;
    ratio = a.noise_front[(i64)(s - ns - 1) * a.P + p] * diff + k.front_min;
    disp = (ratio - 1.0f) * dist;
  } else {                                                     // Part 3: free space behind (:94-107)
    const float free_max = k.end_dist / dist + 1.0f;
    const float behind_min = 1.0f + k.two_sigma / dist;
    const float diff = free_max - behind_min;
    ratio = a.noise_behind[(i64)(s - ns - nf - 1) * a.P + p] * diff + behind_min;
    disp = (ratio - 1.0f) * dist;
  }
  a.coord[3 * row] = x * ratio;
  a.coord[3 * row + 1] = y * ratio;
  a.coord[3 * row + 2] = z * ratio;
  a.sdf_label[row] = disp * -1.0f;                             // :223
  const bool surface = s <= ns;
  float w = 1.0f;
  if (a.dist_weight_on && surface) w = k.dw_base - (dist / k.max_range) * k.dw_scale;   // :151-156
  if (a.behind_dropoff_on) {                                   // :160-168; the comparisons keep a NaN, as torch.clamp
    float d = (k.drop_max - disp) / k.drop_diff;
    d = d < 0.0f ? 0.0f : (d > 1.0f ? 1.0f : d);
    d = d * 0.8f + 0.2f;
    w = w * d;
  }
  if (!surface) w = w * -1.0f;                                 // :171
  a.weight[row] = w;
  if (a.out_normal) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out_normal[3 * row + c] = a.normal[3 * p + c];
  }
  if (a.out_sem) {                                             // cat with the fp32 zeros promotes, then .int() (:190-198)
    float lab = 0.f;
    if (surface) lab = a.sem_is_i64 ? (float)((const i64*)a.sem)[p] : (float)((const int32_t*)a.sem)[p];
    a.out_sem[row] = (int32_t)lab;
  }
  if (a.out_color) {
    const int C = a.color_channels;
    for (int c = 0; c < C; ++c) a.out_color[row * C + c] = surface ? a.color[p * C + c] : -1.0f;
  }
}

// ------------------------------------------------------------------ batch draw
constexpr int MAX_DRAW_JOBS = 16;
struct DrawK {
  const uint8_t* src[MAX_DRAW_JOBS];
  uint8_t* dst[MAX_DRAW_JOBS];
  i64 row_bytes[MAX_DRAW_JOBS];
  const i64 *r_hist, *r_new, *local_idx, *new_idx;
  i64 bs_history, bs, n_local, n_new, pool_rows;
  int32_t* oob;
};

// the pool row of output row b, or -1 when any link of the chain is out of range
__device__ inline i64 draw_row(const DrawK& k, i64 b) {
  i64 i;
  if (b < k.bs_history) {
    i = k.r_hist[b];
    if (k.local_idx) {
      if (i < 0 || i >= k.n_local) return -1;
      i = k.local_idx[i];
    }
  } else {
    i = k.r_new[b - k.bs_history];
    if (i < 0 || i >= k.n_new) return -1;
    i = k.new_idx[i];
  }
  return (i < 0 || i >= k.pool_rows) ? -1 : i;
}

// blockIdx.y = tensor; rows of 4-byte multiples move as words, the others as bytes
__global__ __launch_bounds__(256) void pool_draw_kernel(DrawK k) {
  const int g = blockIdx.y;
  const i64 rb = k.row_bytes[g];
  const bool words = (rb & 3) == 0 && ((uintptr_t)k.src[g] & 3) == 0 && ((uintptr_t)k.dst[g] & 3) == 0;
  const i64 rw = words ? rb >> 2 : rb;
  const i64 stride = (i64)gridDim.x * 256;
  bool bad = false;
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < k.bs * rw; e += stride) {
    const i64 r = e / rw, c = e - r * rw;
    const i64 i = draw_row(k, r);
    bad |= i < 0;
    if (words) {
      reinterpret_cast<uint32_t*>(k.dst[g])[e] = i < 0 ? 0u : reinterpret_cast<const uint32_t*>(k.src[g])[i * rw + c];
    } else {
      k.dst[g][e] = i < 0 ? (uint8_t)0 : k.src[g][i * rw + c];
    }
  }
  if (bad && k.oob) atomicOr(k.oob, 1);
}

// ------------------------------------------------------------------ transform
__global__ void ts_range_init_kernel(i64* __restrict__ mm) {
  mm[0] = LLONG_MAX;
  mm[1] = LLONG_MIN;
}

template <typename TS>
__global__ __launch_bounds__(256) void ts_range_kernel(const TS* __restrict__ ts, i64 N, i64* __restrict__ mm) {
  i64 lo = LLONG_MAX, hi = LLONG_MIN;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < N; i += (i64)gridDim.x * 256) {
    const i64 v = (i64)ts[i];
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const i64 l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) {                               // integer min / max: order does not matter
    atomicMin(&mm[0], lo);
    atomicMax(&mm[1], hi);
  }
}

template <typename PT, typename TS>
__global__ __launch_bounds__(256) void pool_transform_kernel(i64 N, float* __restrict__ pts, const TS* __restrict__ tsv,
                                                             const PT* __restrict__ pose, i64 T,
                                                             int32_t* __restrict__ oob) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  i64 ts = (i64)tsv[i];
  if (ts < 0) ts += T;                                         // python indexing
  if (ts < 0 || ts >= T) {                                     // the reference's IndexError: flagged, row not moved
    if (oob) atomicOr(oob, 1);
    return;
  }
  const PT* M = pose + 16 * ts;
  const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float r0 = (float)M[4 * r], r1 = (float)M[4 * r + 1], r2 = (float)M[4 * r + 2], t = (float)M[4 * r + 3];
    pts[3 * i + r] = ((r0 * x + r1 * y) + r2 * z) + t;         // bmm row, then + translation
  }
}

// ------------------------------------------------------------------ window
constexpr int kChunk = 2048;                                   // rows per wave: 32 steps of 64 lanes

__device__ inline bool in_window(const float* __restrict__ pts, i64 i, float ox, float oy, float oz, float radius,
                                 int range_2d) {
  const float dx = pts[3 * i] - ox, dy = pts[3 * i + 1] - oy;
  float s = dx * dx + dy * dy;
  if (!range_2d) {
    const float dz = pts[3 * i + 2] - oz;
    s = s + dz * dz;
  }
  return sqrtf(s) < radius;
}

__global__ __launch_bounds__(256) void window_count_kernel(const float* __restrict__ pts, i64 N,
                                                           const float* __restrict__ origin, float radius, int range_2d,
                                                           uint32_t* __restrict__ counts, i64 nchunks) {
  const i64 chunk = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;                                // wave-uniform
  const int lane = threadIdx.x & 63;
  const float ox = origin[0], oy = origin[1], oz = origin[2];
  uint32_t c = 0;
  for (int step = 0; step < kChunk / 64; ++step) {
    const i64 i = chunk * kChunk + step * 64 + lane;
    const bool in = i < N && in_window(pts, i, ox, oy, oz, radius, range_2d);
    c += (uint32_t)__popcll(__ballot(in));
  }
  if (lane == 0) counts[chunk] = c;
}

// one wave: exclusive scan of the chunk counts, the total as two 32-bit words for the read-back
__global__ __launch_bounds__(64) void window_scan_kernel(const uint32_t* __restrict__ counts, i64 nchunks,
                                                         i64* __restrict__ offsets, uint32_t* __restrict__ total2) {
  const int lane = threadIdx.x;
  i64 carry = 0;
  for (i64 base = 0; base < nchunks; base += 64) {
    const i64 j = base + lane;
    const i64 own = j < nchunks ? (i64)counts[j] : 0;
    i64 v = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const i64 u = __shfl_up(v, off, 64);
      if (lane >= off) v += u;
    }
    if (j < nchunks) offsets[j] = carry + v - own;
    carry += __shfl(v, 63, 64);
  }
  if (lane == 0) {
    total2[0] = (uint32_t)((u64)carry & 0xFFFFFFFFull);
    total2[1] = (uint32_t)((u64)carry >> 32);
  }
}

__global__ __launch_bounds__(256) void window_emit_kernel(const float* __restrict__ pts, i64 N,
                                                          const float* __restrict__ origin, float radius, int range_2d,
                                                          const i64* __restrict__ offsets, i64 nchunks,
                                                          i64* __restrict__ rows, i64 cap) {
  const i64 chunk = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;                                // wave-uniform
  const int lane = threadIdx.x & 63;
  const float ox = origin[0], oy = origin[1], oz = origin[2];
  i64 pos = offsets[chunk];
  for (int step = 0; step < kChunk / 64; ++step) {
    const i64 i = chunk * kChunk + step * 64 + lane;
    const bool in = i < N && in_window(pts, i, ox, oy, oz, radius, range_2d);
    const u64 m = __ballot(in);
    const i64 at = pos + __popcll(m & (((u64)1 << lane) - 1));
    if (in && at < cap) rows[at] = i;                          // never past the caller's buffer
    pos += __popcll(m);
  }
}

struct WindowScratch {
  uint32_t* counts;
  i64* offsets;
  uint32_t* total2;
  i64 nchunks;
  size_t total;
};
WindowScratch carve_window(void* blob, i64 n) {
  pings::Carver c(blob);
  WindowScratch w;
  w.nchunks = n > 0 ? (n + kChunk - 1) / kChunk : 0;
  const size_t nc = (size_t)(w.nchunks > 0 ? w.nchunks : 1);
  w.counts = c.take<uint32_t>(nc);
  w.offsets = c.take<i64>(nc);
  w.total2 = c.take<uint32_t>(2);
  w.total = c.total();
  return w;
}

}  // namespace

PINGS_API int pings_pool_sample(const pings_pool_sample_args* args, void* stream) {
  PINGS_ARG_CHECK(args != nullptr, "null pointer");
  const pings_pool_sample_args& a = *args;
  PINGS_ARG_CHECK(a.P >= 0 && a.surface_sample_n >= 0 && a.free_front_n >= 0 && a.free_behind_n >= 0, "bad sizes");
  const i64 S = (i64)a.surface_sample_n + a.free_front_n + a.free_behind_n + 1;
  PINGS_ARG_CHECK(a.P <= (int64_t)0x7FFFFFF0 / S, "too many rows");
  if (a.P == 0) return PINGS_OK;
  PINGS_ARG_CHECK(a.points && a.coord && a.sdf_label && a.weight, "null pointer");
  PINGS_ARG_CHECK((a.surface_sample_n == 0 || a.noise_surface) && (a.free_front_n == 0 || a.noise_front) &&
                      (a.free_behind_n == 0 || a.noise_behind), "null pointer (noise)");
  PINGS_ARG_CHECK(!a.out_normal || a.normal, "null pointer (normal)");
  PINGS_ARG_CHECK(!a.out_sem || a.sem, "null pointer (sem)");
  PINGS_ARG_CHECK(!a.out_color || (a.color && a.color_channels >= 1 && a.color_channels <= 4), "colour: 1..4 channels");
  SampleK k;
  k.a = a;
  const double end = a.free_sample_end_dist;
  k.range = (float)a.surface_sample_range;
  k.two_sigma = (float)(2.0 * a.surface_sample_range);        // sigma_ratio * surface_sample_range
  k.front_min = (float)a.free_sample_begin_ratio;
  k.end_dist = (float)end;
  k.dw_base = (float)(1 + a.dist_weight_scale * 0.5);
  k.dw_scale = (float)a.dist_weight_scale;
  k.max_range = (float)a.max_range;
  k.drop_max = (float)end;
  k.drop_diff = (float)(end - 0.2 * end);                      // dropoff_max - dropoff_min
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_sample", st);
  pool_sample_kernel<<<blocks_for(a.P * S), 256, 0, st>>>(k);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_pool_draw(const pings_gather_job* jobs, int njobs, const int64_t* r_hist, int64_t bs_history,
                              const int64_t* r_new, int64_t bs_new, const int64_t* local_idx, int64_t n_local,
                              const int64_t* new_idx, int64_t n_new, int64_t pool_rows, int32_t* out_of_range,
                              void* stream) {
  PINGS_ARG_CHECK(jobs && njobs > 0 && njobs <= MAX_DRAW_JOBS, "null pointer or not 1..16 jobs");
  PINGS_ARG_CHECK(bs_history >= 0 && bs_new >= 0 && n_local >= 0 && n_new >= 0 && pool_rows >= 0, "bad sizes");
  const i64 bs = bs_history + bs_new;
  if (bs == 0) return PINGS_OK;
  PINGS_ARG_CHECK(bs_history == 0 || r_hist, "null pointer (r_hist)");
  PINGS_ARG_CHECK(bs_new == 0 || (r_new && (new_idx || n_new == 0)), "null pointer (r_new / new_idx)");
  PINGS_ARG_CHECK(local_idx || n_local == 0, "null pointer (local_idx)");
  DrawK k{};
  i64 most = 0;
  for (int g = 0; g < njobs; ++g) {
    PINGS_ARG_CHECK(jobs[g].row_bytes > 0 && jobs[g].rows == bs, "job: row_bytes > 0 and rows == bs_history + bs_new");
    PINGS_ARG_CHECK(jobs[g].dst && (jobs[g].src || pool_rows == 0), "null pointer in job");
    k.src[g] = reinterpret_cast<const uint8_t*>(jobs[g].src);
    k.dst[g] = reinterpret_cast<uint8_t*>(jobs[g].dst);
    k.row_bytes[g] = jobs[g].row_bytes;
    const i64 work = bs * ((jobs[g].row_bytes & 3) == 0 ? jobs[g].row_bytes >> 2 : jobs[g].row_bytes);
    if (work > most) most = work;
  }
  k.r_hist = (const i64*)r_hist; k.r_new = (const i64*)r_new;
  k.local_idx = (const i64*)local_idx; k.new_idx = (const i64*)new_idx;
  k.bs_history = bs_history; k.bs = bs; k.n_local = n_local; k.n_new = n_new; k.pool_rows = pool_rows;
  k.oob = out_of_range;
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_draw", st);
  const i64 nb = (most + 255) / 256;
  pool_draw_kernel<<<dim3((unsigned)(nb < 4096 ? nb : 4096), (unsigned)njobs), 256, 0, st>>>(k);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_pool_ts_range(const void* ts, int32_t ts_is_i64, int64_t N, int64_t* min_max, void* stream) {
  PINGS_ARG_CHECK(N >= 0 && min_max, "null pointer or negative N");
  PINGS_ARG_CHECK(N == 0 || ts, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_ts_range", st);
  ts_range_init_kernel<<<1, 1, 0, st>>>(reinterpret_cast<i64*>(min_max));
  PINGS_LAUNCH_CHECK();
  if (N == 0) return PINGS_OK;
  const unsigned nb = blocks_for(N) < 2048u ? blocks_for(N) : 2048u;
  if (ts_is_i64)
    ts_range_kernel<i64><<<nb, 256, 0, st>>>((const i64*)ts, N, reinterpret_cast<i64*>(min_max));
  else
    ts_range_kernel<int32_t><<<nb, 256, 0, st>>>((const int32_t*)ts, N, reinterpret_cast<i64*>(min_max));
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_pool_transform(int64_t N, float* points, const void* ts, int32_t ts_is_i64, const void* pose_diff,
                                   int32_t pose_is_f64, int64_t num_poses, int32_t* out_of_range, void* stream) {
  PINGS_ARG_CHECK(N >= 0 && num_poses > 0, "bad sizes");
  if (N == 0) return PINGS_OK;
  PINGS_ARG_CHECK(points && ts && pose_diff, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_transform", st);
  const unsigned nb = blocks_for(N);
  if (pose_is_f64) {
    if (ts_is_i64)
      pool_transform_kernel<double, i64><<<nb, 256, 0, st>>>(N, points, (const i64*)ts, (const double*)pose_diff,
                                                             num_poses, out_of_range);
    else
      pool_transform_kernel<double, int32_t><<<nb, 256, 0, st>>>(N, points, (const int32_t*)ts,
                                                                 (const double*)pose_diff, num_poses, out_of_range);
  } else {
    if (ts_is_i64)
      pool_transform_kernel<float, i64><<<nb, 256, 0, st>>>(N, points, (const i64*)ts, (const float*)pose_diff,
                                                            num_poses, out_of_range);
    else
      pool_transform_kernel<float, int32_t><<<nb, 256, 0, st>>>(N, points, (const int32_t*)ts, (const float*)pose_diff,
                                                                num_poses, out_of_range);
  }
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API size_t pings_pool_window_scratch_bytes(int64_t n) { return carve_window(nullptr, n).total; }

PINGS_API int pings_pool_window_count(const float* points, int64_t n, const float* origin, float radius,
                                      int32_t range_filter_2d, void* scratch, int64_t* count, void* stream) {
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFF0 && count, "null pointer or bad size");
  *count = 0;
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(points && origin && scratch, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_window_count", st);
  WindowScratch w = carve_window(scratch, n);
  window_count_kernel<<<(unsigned)((w.nchunks + 3) / 4), 256, 0, st>>>(points, n, origin, radius, range_filter_2d,
                                                                       w.counts, w.nchunks);
  PINGS_LAUNCH_CHECK();
  window_scan_kernel<<<1, 64, 0, st>>>(w.counts, w.nchunks, w.offsets, w.total2);
  PINGS_LAUNCH_CHECK();
  const uint32_t* src[2] = {w.total2, w.total2 + 1};
  uint32_t got[2] = {0u, 0u};
  if (int e = pings::host_read_words(src, 2, got, st)) return e;
  *count = (int64_t)(((u64)got[1] << 32) | got[0]);
  return PINGS_OK;
}

PINGS_API int pings_pool_window(const float* points, int64_t n, const float* origin, float radius,
                                int32_t range_filter_2d, const void* scratch, int64_t* rows, int64_t capacity,
                                void* stream) {
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFF0 && capacity >= 0, "bad size");
  if (n == 0 || capacity == 0) return PINGS_OK;
  PINGS_ARG_CHECK(points && origin && scratch && rows, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_window", st);
  WindowScratch w = carve_window(const_cast<void*>(scratch), n);
  window_emit_kernel<<<(unsigned)((w.nchunks + 3) / 4), 256, 0, st>>>(points, n, origin, radius, range_filter_2d,
                                                                      w.offsets, w.nchunks, reinterpret_cast<i64*>(rows),
                                                                      capacity);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}
