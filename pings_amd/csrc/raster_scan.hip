// Prefix sums of the rasteriser: out[i] = f(in[0]) + .. + f(in[i - 1]) (exclusive; inclusive adds f(in[i])), modulo 2^32,
// in two launches with no state that outlives them: nothing to clear, no workgroup waits for another, no look-back
// chain, and no atomic decides a value, so two runs (and the library scan) give the same bits.
//
//   reduce  workgroup b owns elements [b * SCAN_BLOCK, (b + 1) * SCAN_BLOCK), four consecutive ones per thread, read
//           through the functor: their sum -> totals[b]
//   apply   the same blocks: a workgroup adds up the totals in front of it itself (at most SCAN_BLOCK words, one uint4
//           per thread), scans its own elements (in the thread, in the wave, over the waves through LDS) and stores them
//
// A scan that fits one workgroup skips the reduce launch.  One launch carries unlike work of the backward's prelude
// with it: the reduce launch of the live scan has one extra workgroup that computes the backward's tile order
// (tile_order_body: the same 1,024 threads, no data in common with the scan).
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "raster_common.hpp"

namespace pings {
namespace raster {

namespace {

constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr size_t SCAN_TOTALS_BYTES = (size_t)SCAN_BLOCK * sizeof(uint32_t);   // the whole table, whatever n: uint4 reads stay inside

struct Identity {
  __host__ __device__ uint32_t operator()(const uint32_t& v) const { return v; }
};
struct Counting {};   // in place of an input pointer: the element is its own index

template <typename T>
struct alignas(4 * sizeof(T)) Quad {
  T v[4];
};

// elements i0 .. i0 + 3 through the functor, 0 past the end; `in` is aligned to four elements and so is i0
template <typename T, typename Op>
__device__ inline void load4(const T* __restrict__ in, const Op& op, uint32_t i0, uint32_t n, uint32_t (&v)[4]) {
  if (i0 + 4u <= n) {
    const Quad<T> q = *reinterpret_cast<const Quad<T>*>(in + i0);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = op(q.v[k]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? op(in[i0 + k]) : 0u;
  }
}
// The chunk counts of ranks i0 .. i0 + 3 (RowRanges::operator()), with every load of one level issued before the first
// of the next is waited for: the offsets of all four ranks, then their eight cidx words.  Ranks past the end read slot
// 0 and count 0.
__device__ inline void load4(Counting, const RowRanges& rr, uint32_t i0, uint32_t n, uint32_t (&v)[4]) {
  const uint32_t P = min((uint32_t)rr.P, n);
  uint32_t e[4], t[4];
  if (i0 + 4u <= P) {
    const uint4 qe = *reinterpret_cast<const uint4*>(rr.offsets_sorted + i0);
    const uint4 qt = *reinterpret_cast<const uint4*>(rr.tiles_sorted + i0);
    e[0] = qe.x; e[1] = qe.y; e[2] = qe.z; e[3] = qe.w;
    t[0] = qt.x; t[1] = qt.y; t[2] = qt.z; t[3] = qt.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool in = i0 + k < P;
      e[k] = in ? rr.offsets_sorted[i0 + k] : 0u;
      t[k] = in ? rr.tiles_sorted[i0 + k] : 0u;
    }
  }
  uint32_t rb[4], re[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rb[k] = rr.cidx[e[k] - t[k]];
    re[k] = rr.cidx[e[k]];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = i0 + k < P ? (re[k] - rb[k] + (uint32_t)CH - 1u) / (uint32_t)CH : 0u;
}

// ORDER: workgroup 0 is the tile-order workgroup, the scan's workgroups follow it
template <typename In, typename Op, bool ORDER>
__global__ __launch_bounds__(SCAN_THREADS) void scan_reduce_kernel(In in, Op op, uint32_t n, uint32_t* __restrict__ totals,
                                                                    TileOrderJob job) {
  if constexpr (ORDER) {
    if (blockIdx.x == 0) {   // first: the longest workgroup of the launch
      tile_order_body<false>(job.work, nullptr, job.num_tiles, job.order, job.n_long, job.long_thr, job.long_max);
      return;
    }
  }
  __shared__ uint32_t wsum[SCAN_WAVES];
  const uint32_t tid = threadIdx.x, b = blockIdx.x - (ORDER ? 1u : 0u);
  uint32_t v[4];
  load4(in, op, b * (uint32_t)SCAN_BLOCK + tid * 4u, n, v);
  const uint32_t s = wave_reduce_sum_u32_dpp((v[0] + v[1]) + (v[2] + v[3]));
  if ((tid & 63u) == 63u) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0u;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) t += wsum[w];
    totals[b] = t;
  }
}

template <typename In, typename Op, bool INCLUSIVE>
__global__ __launch_bounds__(SCAN_THREADS) void scan_apply_kernel(In in, Op op, uint32_t n,
                                                                   const uint32_t* __restrict__ totals,
                                                                   uint32_t* __restrict__ out) {
  __shared__ uint32_t wsum[SCAN_WAVES], wfront[SCAN_WAVES];
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  // totals[0 .. b): b <= SCAN_BLOCK, and the table is SCAN_BLOCK words whatever the scan's length
  uint32_t front = 0u;
  if (tid * 4u < b) {
    const uint4 q = reinterpret_cast<const uint4*>(totals)[tid];
    front = q.x + (tid * 4u + 1u < b ? q.y : 0u) + (tid * 4u + 2u < b ? q.z : 0u) + (tid * 4u + 3u < b ? q.w : 0u);
  }
  const uint32_t i0 = b * (uint32_t)SCAN_BLOCK + tid * 4u;
  uint32_t v[4];
  load4(in, op, i0, n, v);
  const uint32_t sum = (v[0] + v[1]) + (v[2] + v[3]);
  const uint32_t incl = wave_inclusive_sum(sum, lane);
  const uint32_t wave_front = wave_reduce_sum_u32_dpp(front);   // lane 63
  if (lane == 63) {
    wsum[wave] = incl;
    wfront[wave] = wave_front;
  }
  __syncthreads();
  uint32_t run = incl - sum;
#pragma unroll
  for (int w = 0; w < SCAN_WAVES; ++w) run += wfront[w] + (w < wave ? wsum[w] : 0u);
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o[k] = INCLUSIVE ? run + v[k] : run;
    run += v[k];
  }
  if (i0 + 4u <= n) {
    *reinterpret_cast<uint4*>(out + i0) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < n) out[i0 + k] = o[k];
  }
}

__global__ __launch_bounds__(256) void pair_owner_kernel(int P, const uint32_t* __restrict__ pair_off,
                                                          uint32_t* __restrict__ pair_owner) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= P) return;
  const uint32_t a = pair_off[r], b = pair_off[r + 1];
  for (uint32_t q = a; q < b; ++q) pair_owner[q] = (uint32_t)r;
}

template <typename T>
bool aligned4(const T* p) { return reinterpret_cast<uintptr_t>(p) % (4 * sizeof(T)) == 0; }
bool aligned4(Counting) { return true; }

template <typename It>
int scan_library(It it, int64_t n, bool inclusive, uint32_t* out, void* temp, size_t temp_bytes, hipStream_t st) {
  if (inclusive) PINGS_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, it, out, (int)n, st));
  else PINGS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, it, out, (int)n, st));
  return PINGS_OK;
}
template <typename T, typename Op>
auto library_input(const T* in, Op op) { return hipcub::TransformInputIterator<uint32_t, Op, const T*>(in, op); }
template <typename Op>
auto library_input(Counting, Op op) {
  return hipcub::TransformInputIterator<uint32_t, Op, hipcub::CountingInputIterator<uint32_t>>(
      hipcub::CountingInputIterator<uint32_t>(0u), op);
}
inline const uint32_t* library_input(const uint32_t* in, Identity) { return in; }

bool own_scan(int64_t n, bool library) { return !library && n <= SCAN_MAX; }

// the project's two launches; `job` (nullable): the tile-order workgroup
template <typename In, typename Op>
int scan_launches(In in, Op op, int64_t n, bool inclusive, uint32_t* out, void* temp, size_t temp_bytes,
                  const TileOrderJob* job, hipStream_t st) {
  PINGS_ARG_CHECK(n > 0 && n <= SCAN_MAX && out && temp && temp_bytes >= SCAN_TOTALS_BYTES, "scan: size or scratch out of range");
  PINGS_ARG_CHECK(aligned4(in) && aligned4(out) && aligned4(static_cast<const uint32_t*>(temp)), "scan: unaligned array");
  const uint32_t nblk = ceil_div<uint32_t>((uint32_t)n, SCAN_BLOCK);
  uint32_t* totals = static_cast<uint32_t*>(temp);
  if (job) {
    if (int e = launch(scan_reduce_kernel<In, Op, true>, dim3(nblk + 1), SCAN_THREADS, 0, st, in, op, (uint32_t)n, totals, *job))
      return e;
  } else if (nblk > 1) {   // a single workgroup has nothing in front of it: the apply kernel reads no totals
    if (int e = launch(scan_reduce_kernel<In, Op, false>, dim3(nblk), SCAN_THREADS, 0, st, in, op, (uint32_t)n, totals,
                       TileOrderJob{}))
      return e;
  }
  return with_flag(inclusive, [&](auto f) {
    return launch(scan_apply_kernel<In, Op, f()>, dim3(nblk), SCAN_THREADS, 0, st, in, op, (uint32_t)n,
                  (const uint32_t*)totals, out);
  });
}

template <typename In, typename Op>
int scan(In in, Op op, int64_t n, bool inclusive, uint32_t* out, void* temp, size_t temp_bytes, bool library,
         hipStream_t st) {
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFFF, "scan: element count out of range");
  if (n == 0) return PINGS_OK;
  if (own_scan(n, library)) return scan_launches(in, op, n, inclusive, out, temp, temp_bytes, nullptr, st);
  return scan_library(library_input(in, op), n, inclusive, out, temp, temp_bytes, st);
}

// the live scan and, with it or behind it, the backward's tile order
template <typename T, typename Op>
int scan_with_order(const T* in, Op op, int64_t n, uint32_t* cidx, void* temp, size_t temp_bytes, bool library,
                    const TileOrderJob& job, hipStream_t st) {
  if (!job.work) return scan(in, op, n, false, cidx, temp, temp_bytes, library, st);
  if (n > 0 && own_scan(n, library))
    return scan_launches(in, op, n, false, cidx, temp, temp_bytes, &job, st);
  if (int e = scan(in, op, n, false, cidx, temp, temp_bytes, library, st)) return e;
  return launch_tile_order(job.work, job.num_tiles, job.order, st, job.n_long, job.long_thr, job.long_max);
}

}  // namespace

size_t raster_scan_bytes(int64_t n) {
  const int m = (int)std::min<int64_t>(std::max<int64_t>(n, 1), 0x7FFFFFFF);
  size_t a = 0, b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, m);
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, m);
  return align_up(std::max(std::max(a, b), SCAN_TOTALS_BYTES)) + 256;
}

int raster_scan_u32(const uint32_t* in, int64_t n, bool inclusive, uint32_t* out, void* temp, size_t temp_bytes,
                    bool library, hipStream_t st) {
  return scan(in, Identity(), n, inclusive, out, temp, temp_bytes, library, st);
}

int raster_scan_live(const float* inst_w, int64_t n, uint32_t* cidx, void* temp, size_t temp_bytes, bool library,
                     const TileOrderJob& job, hipStream_t st) {
  return scan_with_order(inst_w, LiveOp(), n, cidx, temp, temp_bytes, library, job, st);
}

int raster_scan_pop(const uint8_t* inst_qmask, int64_t n, uint32_t* cidx, void* temp, size_t temp_bytes, bool library,
                    const TileOrderJob& job, hipStream_t st) {
  return scan_with_order(inst_qmask, PopOp(), n, cidx, temp, temp_bytes, library, job, st);
}

int raster_scan_chunks(const RowRanges& rr, uint32_t* pair_off, uint32_t* pair_owner, void* temp, size_t temp_bytes,
                       bool library, hipStream_t st) {
  const int64_t n = (int64_t)rr.P + 1;
  if (own_scan(n, library)) {
    if (int e = scan_launches(Counting(), rr, n, false, pair_off, temp, temp_bytes, nullptr, st)) return e;
  } else if (int e = scan_library(library_input(Counting(), rr), n, false, pair_off, temp, temp_bytes, st)) {
    return e;
  }
  return launch(pair_owner_kernel, dim3(ceil_div(rr.P + 1, 256)), 256, 0, st, rr.P, (const uint32_t*)pair_off, pair_owner);
}

}  // namespace raster
}  // namespace pings

using namespace pings::raster;

PINGS_API size_t pings_raster_scan_bytes(int64_t n) { return raster_scan_bytes(n); }

PINGS_API int pings_raster_scan_u32(const void* in, int64_t n, int kind, int inclusive, uint32_t* out, void* temp,
                                    size_t temp_bytes, void* stream) {
  PINGS_ARG_CHECK(kind >= 0 && kind <= 2, "kind: 0 = uint32, 1 = float live flag, 2 = byte popcount");
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFFF, "element count out of range");
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(in && out && temp && temp_bytes >= raster_scan_bytes(n), "null pointer or too little scratch");
  hipStream_t st = pings::as_stream(stream);
  const bool library = read_knobs().library_scan;
  if (kind == 0) return scan(static_cast<const uint32_t*>(in), Identity(), n, inclusive != 0, out, temp, temp_bytes, library, st);
  if (kind == 1) return scan(static_cast<const float*>(in), LiveOp(), n, inclusive != 0, out, temp, temp_bytes, library, st);
  return scan(static_cast<const uint8_t*>(in), PopOp(), n, inclusive != 0, out, temp, temp_bytes, library, st);
}
