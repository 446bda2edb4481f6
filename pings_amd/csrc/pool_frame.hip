// The pool part of Mapper.process_frame on the device, for gfx950.
//
// Restates what the reference does in plain torch, once per mapped frame, around its kernels:
//   pool_append          the seven torch.cat calls and transform_torch of utils/mapper.py:340-366: rows [n, n + m) of
//                        every pool tensor in ONE launch, one thread per appended row.
//   pool_discard_mark    `filter_mask[true_indices[discarded_index]] = False` (:395-399) on a byte mask.
//   pool_compact         the boolean-mask indexing of every pool tensor (:404-423), stable and out of place.  Built as
//                        the sample window of pool.hip is: a wave owns 2048 consecutive rows, rank from ballot and
//                        popcount, one wave scans the per-wave counts, one read-back (kept rows, kept rows of the tail).
//   pool_select_update   the update points of :262-284: rows with |sdf_label| < thr, transformed by the frame's pose,
//                        their colours, their normals rotated; count / scan / emit as above.
// All kernels are HBM-stream bound.  Plain stores, no float atomics, no LDS: a hand-off between waves is always a new
// launch, so every result is bitwise reproducible.
#include "common.hpp"

namespace {

using i64 = long long;
using u64 = unsigned long long;

constexpr int kChunk = 2048;                                   // rows per wave: 32 steps of 64 lanes
constexpr int MAX_JOBS = 16;

inline unsigned blocks_for(i64 n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

// the frame's pose as the kernels use it: fp64 entries are rounded to fp32 first (`transformation.to(points)`)
struct Pose {
  float r[3][3], t[3];
};
template <typename PT>
__device__ inline Pose load_pose(const void* pose) {
  const PT* M = reinterpret_cast<const PT*>(pose);
  Pose p;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) p.r[i][j] = (float)M[4 * i + j];
    p.t[i] = (float)M[4 * i + 3];
  }
  return p;
}
// ((R_i0 x + R_i1 y) + R_i2 z) [+ t_i]: the order of pool_transform_kernel
__device__ inline void rigid(const Pose& p, const float* __restrict__ src, float* __restrict__ dst, bool translate) {
  const float x = src[0], y = src[1], z = src[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float v = (p.r[i][0] * x + p.r[i][1] * y) + p.r[i][2] * z;
    dst[i] = translate ? v + p.t[i] : v;
  }
}

// ------------------------------------------------------------------ append
template <typename PT>
__global__ __launch_bounds__(256) void pool_append_kernel(pings_pool_append_args a) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.m) return;
  const i64 o = a.n + i;                                       // < capacity (checked by the host)
  const Pose p = load_pose<PT>(a.pose);
  rigid(p, a.coord + 3 * i, a.global_coord_pool + 3 * o, true);
  a.sdf_label_pool[o] = a.sdf_label[i];
  a.weight_pool[o] = a.weight[i];
  a.time_pool[o] = a.frame_id;
  if (a.sem_label_pool) a.sem_label_pool[o] = a.sem[i];
  if (a.color_pool) {
    const int C = a.color_channels;
    for (int c = 0; c < C; ++c) a.color_pool[o * C + c] = a.color[i * C + c];
  }
  if (a.normal_label_pool) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.normal_label_pool[3 * o + c] = a.normal[3 * i + c];
  }
}

// ------------------------------------------------------------------ discard mark
__global__ __launch_bounds__(256) void pool_discard_kernel(const i64* __restrict__ r, i64 count, i64 n,
                                                           uint8_t* __restrict__ keep, int32_t* __restrict__ status) {
  bool bad = false;
  for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < count; j += (i64)gridDim.x * 256) {
    const i64 row = r[j];
    if (row < 0 || row >= n) bad = true;                       // never dereferenced
    else keep[row] = 0;                                        // duplicates store the same byte
  }
  if (bad && status) atomicOr(status, 1);
}

// ------------------------------------------------------------------ count / scan, shared by compact and select
struct Scratch {
  uint32_t* counts;      // [nchunks] selected rows of the chunk
  uint32_t* tails;       // [nchunks] those among the last `tail` rows
  i64* offsets;          // [nchunks] exclusive scan of counts
  uint32_t* totals;      // [4]: total (lo, hi), tail total (lo, hi)
  i64 nchunks;
  size_t total;
};
Scratch carve(void* blob, i64 n) {
  pings::Carver c(blob);
  Scratch w;
  w.nchunks = n > 0 ? (n + kChunk - 1) / kChunk : 0;
  const size_t nc = (size_t)(w.nchunks > 0 ? w.nchunks : 1);
  w.counts = c.take<uint32_t>(nc);
  w.tails = c.take<uint32_t>(nc);
  w.offsets = c.take<i64>(nc);
  w.totals = c.take<uint32_t>(4);
  w.total = c.total();
  return w;
}

struct KeepPred {
  const uint8_t* keep;
  __device__ bool operator()(i64 i) const { return keep[i] != 0; }
};
struct LabelPred {
  const float* label;
  float thr;
  __device__ bool operator()(i64 i) const { return fabsf(label[i]) < thr; }     // a NaN label is not selected
};

template <typename Pred>
__global__ __launch_bounds__(256) void chunk_count_kernel(Pred pred, i64 N, i64 tail_begin,
                                                          uint32_t* __restrict__ counts, uint32_t* __restrict__ tails,
                                                          i64 nchunks) {
  const i64 chunk = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;                                // wave-uniform
  const int lane = threadIdx.x & 63;
  uint32_t c = 0, t = 0;
  for (int step = 0; step < kChunk / 64; ++step) {
    const i64 i = chunk * kChunk + step * 64 + lane;
    const bool in = i < N && pred(i);
    c += (uint32_t)__popcll(__ballot(in));
    t += (uint32_t)__popcll(__ballot(in && i >= tail_begin));
  }
  if (lane == 0) {
    counts[chunk] = c;
    tails[chunk] = t;
  }
}

// one wave: exclusive scan of the chunk counts, the sum of the tail counts, both totals as 32-bit words for the read-back
__global__ __launch_bounds__(64) void chunk_scan_kernel(const uint32_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ tails, i64 nchunks,
                                                        i64* __restrict__ offsets, uint32_t* __restrict__ totals) {
  const int lane = threadIdx.x;
  i64 carry = 0, tail = 0;
  for (i64 base = 0; base < nchunks; base += 64) {
    const i64 j = base + lane;
    const i64 own = j < nchunks ? (i64)counts[j] : 0;
    i64 v = own, tv = j < nchunks ? (i64)tails[j] : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const i64 u = __shfl_up(v, off, 64), tu = __shfl_up(tv, off, 64);
      if (lane >= off) {
        v += u;
        tv += tu;
      }
    }
    if (j < nchunks) offsets[j] = carry + v - own;
    carry += __shfl(v, 63, 64);
    tail += __shfl(tv, 63, 64);
  }
  if (lane == 0) {
    totals[0] = (uint32_t)((u64)carry & 0xFFFFFFFFull);
    totals[1] = (uint32_t)((u64)carry >> 32);
    totals[2] = (uint32_t)((u64)tail & 0xFFFFFFFFull);
    totals[3] = (uint32_t)((u64)tail >> 32);
  }
}

template <typename Pred>
int count_and_read(Pred pred, i64 n, i64 tail, const Scratch& w, i64* total, i64* tail_total, hipStream_t st) {
  i64 tail_begin = n - tail;
  if (tail_begin < 0) tail_begin = 0;
  chunk_count_kernel<Pred><<<(unsigned)((w.nchunks + 3) / 4), 256, 0, st>>>(pred, n, tail_begin, w.counts, w.tails,
                                                                            w.nchunks);
  PINGS_LAUNCH_CHECK();
  chunk_scan_kernel<<<1, 64, 0, st>>>(w.counts, w.tails, w.nchunks, w.offsets, w.totals);
  PINGS_LAUNCH_CHECK();
  const uint32_t* src[4] = {w.totals, w.totals + 1, w.totals + 2, w.totals + 3};
  uint32_t got[4] = {0u, 0u, 0u, 0u};
  if (int e = pings::host_read_words(src, 4, got, st)) return e;
  *total = (i64)(((u64)got[1] << 32) | got[0]);
  *tail_total = (i64)(((u64)got[3] << 32) | got[2]);
  return PINGS_OK;
}

// ------------------------------------------------------------------ compaction
struct CompactK {
  const uint8_t* src[MAX_JOBS];
  uint8_t* dst[MAX_JOBS];
  i64 row_bytes[MAX_JOBS];
  i64 dst_rows[MAX_JOBS];
  const uint8_t* keep;
  const i64* offsets;
  i64 N, nchunks;
};

// blockIdx.y = tensor, a wave = one chunk of rows; rows of 4-byte multiples move as words, the others as bytes
__global__ __launch_bounds__(256) void pool_compact_kernel(CompactK k) {
  const i64 chunk = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= k.nchunks) return;                              // wave-uniform
  const int g = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const i64 rb = k.row_bytes[g], cap = k.dst_rows[g];
  const bool words = (rb & 3) == 0 && ((uintptr_t)k.src[g] & 3) == 0 && ((uintptr_t)k.dst[g] & 3) == 0;
  const i64 rw = words ? rb >> 2 : rb;
  i64 pos = k.offsets[chunk];
  for (int step = 0; step < kChunk / 64; ++step) {
    const i64 i = chunk * kChunk + step * 64 + lane;
    const bool in = i < k.N && k.keep[i] != 0;
    const u64 m = __ballot(in);
    const i64 at = pos + __popcll(m & (((u64)1 << lane) - 1));
    if (in && at < cap) {                                      // never past the destination
      if (words) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(k.src[g]) + i * rw;
        uint32_t* d = reinterpret_cast<uint32_t*>(k.dst[g]) + at * rw;
        for (i64 c = 0; c < rw; ++c) d[c] = s[c];
      } else {
        const uint8_t* s = k.src[g] + i * rw;
        uint8_t* d = k.dst[g] + at * rw;
        for (i64 c = 0; c < rw; ++c) d[c] = s[c];
      }
    }
    pos += __popcll(m);
  }
}

// ------------------------------------------------------------------ update points
template <typename PT, bool ALL>
__global__ __launch_bounds__(256) void pool_select_kernel(pings_pool_select_args a, const i64* __restrict__ offsets,
                                                          i64 nchunks, float thr) {
  const i64 chunk = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;                                // wave-uniform
  const int lane = threadIdx.x & 63;
  const Pose p = load_pose<PT>(a.pose);
  const int C = a.color_channels;
  i64 pos = ALL ? chunk * kChunk : offsets[chunk];
  for (int step = 0; step < kChunk / 64; ++step) {
    const i64 i = chunk * kChunk + step * 64 + lane;
    const bool in = i < a.n && (ALL || fabsf(a.sdf_label[i]) < thr);
    const u64 m = __ballot(in);
    const i64 at = pos + __popcll(m & (((u64)1 << lane) - 1));
    if (in && at < a.capacity) {                               // never past the caller's buffers
      rigid(p, a.coord + 3 * i, a.out_points + 3 * at, true);
      if (a.out_color)
        for (int c = 0; c < C; ++c) a.out_color[at * C + c] = a.color[i * C + c];
      if (a.out_normal) rigid(p, a.normal + 3 * i, a.out_normal + 3 * at, false);
    }
    pos += __popcll(m);
  }
}

}  // namespace

PINGS_API int pings_pool_append(const pings_pool_append_args* args, void* stream) {
  PINGS_ARG_CHECK(args != nullptr, "null pointer");
  const pings_pool_append_args& a = *args;
  PINGS_ARG_CHECK(a.n >= 0 && a.m >= 0 && a.capacity >= 0 && a.n <= a.capacity && a.m <= a.capacity - a.n,
                  "bad sizes: n + m rows must fit the capacity");
  PINGS_ARG_CHECK(a.capacity < (int64_t)0x7FFFFFF0, "too many rows");
  if (a.m == 0) return PINGS_OK;
  PINGS_ARG_CHECK(a.pose && a.coord && a.sdf_label && a.weight, "null pointer");
  PINGS_ARG_CHECK(a.global_coord_pool && a.sdf_label_pool && a.weight_pool && a.time_pool, "null pointer (pool)");
  PINGS_ARG_CHECK((a.sem_label_pool != nullptr) == (a.sem != nullptr), "sem and its pool go together");
  PINGS_ARG_CHECK((a.color_pool != nullptr) == (a.color != nullptr), "colour and its pool go together");
  PINGS_ARG_CHECK((a.normal_label_pool != nullptr) == (a.normal != nullptr), "normal and its pool go together");
  PINGS_ARG_CHECK(!a.color_pool || (a.color_channels >= 1 && a.color_channels <= 4), "colour: 1..4 channels");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_append", st);
  if (a.pose_is_f64)
    pool_append_kernel<double><<<blocks_for(a.m), 256, 0, st>>>(a);
  else
    pool_append_kernel<float><<<blocks_for(a.m), 256, 0, st>>>(a);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_pool_discard_mark(const int64_t* r, int64_t discard_count, int64_t n, uint8_t* keep,
                                      int32_t* status, void* stream) {
  PINGS_ARG_CHECK(discard_count >= 0 && n >= 0, "bad sizes");
  if (discard_count == 0) return PINGS_OK;
  PINGS_ARG_CHECK(r && (keep || n == 0), "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_discard_mark", st);
  const unsigned nb = blocks_for(discard_count) < 4096u ? blocks_for(discard_count) : 4096u;
  pool_discard_kernel<<<nb, 256, 0, st>>>(reinterpret_cast<const i64*>(r), discard_count, n, keep, status);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API size_t pings_pool_compact_scratch_bytes(int64_t n) { return carve(nullptr, n).total; }

PINGS_API int pings_pool_compact_count(const uint8_t* keep, int64_t n, int64_t tail, void* scratch, int64_t* counts2,
                                       void* stream) {
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFF0 && tail >= 0 && counts2, "null pointer or bad size");
  counts2[0] = counts2[1] = 0;
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(keep && scratch, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_compact_count", st);
  i64 total = 0, tail_total = 0;
  if (int e = count_and_read(KeepPred{keep}, n, tail, carve(scratch, n), &total, &tail_total, st)) return e;
  counts2[0] = total;
  counts2[1] = tail_total;
  return PINGS_OK;
}

PINGS_API int pings_pool_compact(const pings_gather_job* jobs, int njobs, const uint8_t* keep, int64_t n,
                                 const void* scratch, void* stream) {
  PINGS_ARG_CHECK(jobs && njobs > 0 && njobs <= MAX_JOBS, "null pointer or not 1..16 jobs");
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFF0, "bad size");
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(keep && scratch, "null pointer");
  const Scratch w = carve(const_cast<void*>(scratch), n);
  CompactK k{};
  for (int g = 0; g < njobs; ++g) {
    PINGS_ARG_CHECK(jobs[g].row_bytes > 0 && jobs[g].rows >= 0, "job: row_bytes > 0 and rows >= 0");
    PINGS_ARG_CHECK(jobs[g].src && (jobs[g].dst || jobs[g].rows == 0), "null pointer in job");
    const char* s = reinterpret_cast<const char*>(jobs[g].src);
    const char* d = reinterpret_cast<const char*>(jobs[g].dst);
    PINGS_ARG_CHECK(!d || d + jobs[g].rows * jobs[g].row_bytes <= s || s + n * jobs[g].row_bytes <= d,
                    "job: source and destination overlap (the pass is out of place)");
    k.src[g] = reinterpret_cast<const uint8_t*>(jobs[g].src);
    k.dst[g] = reinterpret_cast<uint8_t*>(jobs[g].dst);
    k.row_bytes[g] = jobs[g].row_bytes;
    k.dst_rows[g] = jobs[g].rows;
  }
  k.keep = keep;
  k.offsets = w.offsets;
  k.N = n;
  k.nchunks = w.nchunks;
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_compact", st);
  pool_compact_kernel<<<dim3((unsigned)((w.nchunks + 3) / 4), (unsigned)njobs), 256, 0, st>>>(k);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API size_t pings_pool_select_scratch_bytes(int64_t n) { return carve(nullptr, n).total; }

PINGS_API int pings_pool_select_count(const float* sdf_label, int64_t n, double thr, void* scratch, int64_t* count,
                                      void* stream) {
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFF0 && count, "null pointer or bad size");
  *count = 0;
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(sdf_label && scratch, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_select_count", st);
  i64 total = 0, tail_total = 0;
  if (int e = count_and_read(LabelPred{sdf_label, (float)thr}, n, 0, carve(scratch, n), &total, &tail_total, st))
    return e;
  *count = total;
  return PINGS_OK;
}

PINGS_API int pings_pool_select_update(const pings_pool_select_args* args, void* stream) {
  PINGS_ARG_CHECK(args != nullptr, "null pointer");
  const pings_pool_select_args& a = *args;
  PINGS_ARG_CHECK(a.n >= 0 && a.n < (int64_t)0x7FFFFFF0 && a.capacity >= 0, "bad size");
  if (a.n == 0 || a.capacity == 0) return PINGS_OK;
  PINGS_ARG_CHECK(a.pose && a.coord && a.out_points, "null pointer");
  PINGS_ARG_CHECK(a.select_all || (a.sdf_label && a.scratch), "null pointer (sdf_label / scratch)");
  PINGS_ARG_CHECK(!a.out_color || (a.color && a.color_channels >= 1 && a.color_channels <= 4), "colour: 1..4 channels");
  PINGS_ARG_CHECK(!a.out_normal || a.normal, "null pointer (normal)");
  const Scratch w = carve(const_cast<void*>(a.scratch), a.n);
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("pool_select_update", st);
  const dim3 grid((unsigned)((w.nchunks + 3) / 4));
  const float thr = (float)a.thr;
  if (a.select_all) {
    if (a.pose_is_f64) pool_select_kernel<double, true><<<grid, 256, 0, st>>>(a, nullptr, w.nchunks, thr);
    else pool_select_kernel<float, true><<<grid, 256, 0, st>>>(a, nullptr, w.nchunks, thr);
  } else {
    if (a.pose_is_f64) pool_select_kernel<double, false><<<grid, 256, 0, st>>>(a, w.offsets, w.nchunks, thr);
    else pool_select_kernel<float, false><<<grid, 256, 0, st>>>(a, w.offsets, w.nchunks, thr);
  }
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}
