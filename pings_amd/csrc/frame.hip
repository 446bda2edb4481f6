// Frame-time point tests on the device, for gfx950.
//
// Three query steps of the reference's `Mapper` that run once per frame around the mapping iterations:
//   frame_new_count / frame_new_rows   the new-sample test of process_frame (utils/mapper.py:447-513): the own-cell
//                   lookup of `query_certainty` (model/neural_gaussians.py:1117-1133 with the one-cell neighbourhood of
//                   :1026-1058), the two comparisons and the `torch.where`, as an ascending int64 row list with the pool
//                   offset added.  Two passes in the scheme of pool.hip's window: per-wave counts and keep bits, a
//                   one-wave scan of the counts, one read-back of the total, per-wave ballot compaction.
//   frame_static_mask   the decision of dynamic_filter / dynamic_filter_neural_points (:554-564) from the fused query's
//                   sdf, certainty and gradient, and the number of dynamic points on the device.
//   frame_valid_scatter the two masked assignments of check_invalid_neural_points (:1647-1655) as one row scatter.
// The thresholds the reference forms between python scalars arrive as doubles and are rounded to fp32 once, which is
// what torch does with a python scalar against an fp32 tensor.  No LDS, no float atomics; no wave waits for another, and
// every result is bitwise reproducible (the dynamic count is an integer sum).
#include "knn_common.hpp"

namespace {

using namespace pings_knn;
using i64 = long long;
using u64 = unsigned long long;

// ------------------------------------------------------------------ new-sample test
constexpr int kChunk = 512;                                    // rows per wave: 8 steps of 64 lanes
constexpr int kSteps = kChunk / 64;

struct NewK {
  pings_knn_map m;
  const float* certs;          // point_certainties[num_points]
  i64 num_points;
  const float *coord, *label;  // [n,3], [n]
  i64 n;
  float max_d2, cert_thr, label_thr;
};

// `query_certainty` of one sample through its own cell, then the two comparisons of :482-488.  The cell, the hash and
// the distance are those of knn_cells_kernel (knn_sdf.hip) with K = 1, dx = 0 and no time window.
__device__ inline bool new_keep(const NewK& k, i64 r, double inv_S) {
  const pings_knn_map& m = k.m;
  const float qx = k.coord[3 * r], qy = k.coord[3 * r + 1], qz = k.coord[3 * r + 2];
  const i64 gx = (i64)floorf(qx / m.resolution);
  const i64 gy = (i64)floorf(qy / m.resolution);
  const i64 gz = (i64)floorf(qz / m.resolution);
  const i64 h = hash_slot(gx * P0 + gy * P1 + gz * P2, m.buffer_size, inv_S);
  i64 i = -1;
  if (h >= 0 && h < m.buffer_size) i = table_lookup(m, h);     // a non-finite coordinate must not leave the table
  if (i >= k.num_points) i = -1;                               // a stale table entry is never dereferenced
  float cert = 0.f;                                            // certainty[idx < 0] = 0 (:1127)
  if (i >= 0) {
    const float sx = m.neural_points[3 * i] - qx, sy = m.neural_points[3 * i + 1] - qy, sz = m.neural_points[3 * i + 2] - qz;
    const float dd = (sx * sx + sy * sy) + sz * sz;
    if (!(dd > k.max_d2)) cert = k.certs[i];                   // a hash collision clears the index (:1105)
  }
  return cert < k.cert_thr && fabsf(k.label[r]) < k.label_thr;
}

__global__ __launch_bounds__(256) void new_count_kernel(NewK k, uint32_t* __restrict__ counts, u64* __restrict__ bits,
                                                        i64 nchunks) {
  const i64 chunk = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;                                // wave-uniform
  const int lane = threadIdx.x & 63;
  const double inv_S = 1.0 / (double)k.m.buffer_size;
  bool keep[kSteps];
#pragma unroll
  for (int step = 0; step < kSteps; ++step) {                  // independent gather chains: all in flight together
    const i64 r = chunk * kChunk + step * 64 + lane;
    keep[step] = r < k.n && new_keep(k, r, inv_S);
  }
  uint32_t c = 0;
#pragma unroll
  for (int step = 0; step < kSteps; ++step) {
    const u64 b = __ballot(keep[step]);
    c += (uint32_t)__popcll(b);
    if (lane == 0) bits[chunk * kSteps + step] = b;
  }
  if (lane == 0) counts[chunk] = c;
}

// one wave: exclusive scan of the per-wave counts, the total as two 32-bit words for the read-back
__global__ __launch_bounds__(64) void new_scan_kernel(const uint32_t* __restrict__ counts, i64 nchunks,
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

__global__ __launch_bounds__(256) void new_rows_kernel(const u64* __restrict__ bits, const i64* __restrict__ offsets,
                                                       i64 nchunks, i64 n, i64 pool_offset, i64* __restrict__ rows,
                                                       i64 cap) {
  const i64 chunk = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;                                // wave-uniform
  const int lane = threadIdx.x & 63;
  i64 pos = offsets[chunk];
#pragma unroll
  for (int step = 0; step < kSteps; ++step) {
    const u64 b = bits[chunk * kSteps + step];
    const i64 r = chunk * kChunk + step * 64 + lane;
    const i64 at = pos + __popcll(b & (((u64)1 << lane) - 1));
    if (((b >> lane) & 1ull) && r < n && at >= 0 && at < cap) rows[at] = r + pool_offset;   // never past the caller's buffer
    pos += __popcll(b);
  }
}

struct NewScratch {
  uint32_t* counts;
  i64* offsets;
  uint32_t* total2;
  u64* bits;
  i64 nchunks;
  size_t total;
};
NewScratch carve_new(void* blob, i64 n) {
  pings::Carver c(blob);
  NewScratch w;
  w.nchunks = n > 0 ? (n + kChunk - 1) / kChunk : 0;
  const size_t nc = (size_t)(w.nchunks > 0 ? w.nchunks : 1);
  w.counts = c.take<uint32_t>(nc);
  w.offsets = c.take<i64>(nc);
  w.total2 = c.take<uint32_t>(2);
  w.bits = c.take<u64>(nc * kSteps);
  w.total = c.total();
  return w;
}

// ------------------------------------------------------------------ static mask
template <bool GRAD>
__global__ __launch_bounds__(256) void static_mask_kernel(const float* __restrict__ sdf, const float* __restrict__ cert,
                                                          const float* __restrict__ grad, i64 n, float cert_thr,
                                                          float sdf_thr, float grad_thr, uint8_t* __restrict__ mask,
                                                          u64* __restrict__ dynamic_count) {
  const int lane = threadIdx.x & 63;
  const i64 stride = (i64)gridDim.x * 256;
  uint32_t dyn = 0;
  for (i64 base = (i64)blockIdx.x * 256 + (threadIdx.x & ~63); base < n; base += stride) {   // wave-uniform bound
    const i64 i = base + lane;
    const bool in = i < n;
    bool keep = false;
    if (in) {
      const float c = cert[i];
      const bool uncertain = c < cert_thr;
      keep = uncertain || sdf[i] < sdf_thr;                    // strategy 1 (:554-556)
      if (GRAD) {                                              // strategy 2 (:563): norm as torch, then IEEE sqrt
        const float gx = grad[3 * i], gy = grad[3 * i + 1], gz = grad[3 * i + 2];
        const float norm = sqrtf((gx * gx + gy * gy) + gz * gz);
        keep = keep && (norm > grad_thr || uncertain);
      }
      mask[i] = keep ? 1 : 0;
    }
    dyn += (uint32_t)__popcll(__ballot(in && !keep));
  }
  if (lane == 0 && dyn) atomicAdd(dynamic_count, (u64)dyn);    // integer: the order does not matter
}

// ------------------------------------------------------------------ valid scatter
__global__ __launch_bounds__(256) void valid_scatter_kernel(const i64* __restrict__ rows, i64 n,
                                                            const float* __restrict__ sdf, const i64* __restrict__ nn,
                                                            float sdf_thr, i64 min_nn, const i64* __restrict__ local_idx,
                                                            i64 n_local, i64 n_global, uint8_t* __restrict__ local_valid,
                                                            uint8_t* __restrict__ valid) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const i64 r = rows[i];
  if (r < 0 || r >= n_local) return;                           // a stale row is never dereferenced
  const uint8_t v = (fabsf(sdf[i]) < sdf_thr && nn[i] >= min_nn) ? 1 : 0;
  local_valid[r] = v;
  const i64 g = local_idx[r];
  if (g >= 0 && g < n_global) valid[g] = v;
}

inline unsigned blocks_for(i64 n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

}  // namespace

PINGS_API size_t pings_frame_new_scratch_bytes(int64_t n) { return carve_new(nullptr, n).total; }

PINGS_API int pings_frame_new_count(const pings_knn_map* m, const float* point_certainties, int64_t num_points,
                                    const float* coord, const float* sdf_label, int64_t n, double max_valid_dist2,
                                    double new_certainty_thre, double label_thre, void* scratch, int64_t* count,
                                    void* stream) {
  PINGS_ARG_CHECK(m != nullptr && count != nullptr, "null pointer");
  *count = 0;
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFF0 && num_points >= 0, "bad size");
  PINGS_ARG_CHECK(m->resolution > 0.f, "resolution must be positive");
  PINGS_ARG_CHECK((m->table || m->compact) && m->buffer_size > 0 && m->buffer_size < (1LL << 31), "bad table");
  PINGS_ARG_CHECK(!m->compact || ((m->compact_mask & (m->compact_mask + 1u)) == 0u), "compact_mask must be 2^k - 1");
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(coord && sdf_label && scratch, "null pointer");
  PINGS_ARG_CHECK(num_points == 0 || (m->neural_points && point_certainties), "null pointer (map)");
  NewK k;
  k.m = *m;
  k.certs = point_certainties;
  k.num_points = num_points;
  k.coord = coord;
  k.label = sdf_label;
  k.n = n;
  k.max_d2 = (float)max_valid_dist2;
  k.cert_thr = (float)new_certainty_thre;
  k.label_thr = (float)label_thre;
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("frame_new_count", st);
  NewScratch w = carve_new(scratch, n);
  new_count_kernel<<<(unsigned)((w.nchunks + 3) / 4), 256, 0, st>>>(k, w.counts, w.bits, w.nchunks);
  PINGS_LAUNCH_CHECK();
  new_scan_kernel<<<1, 64, 0, st>>>(w.counts, w.nchunks, w.offsets, w.total2);
  PINGS_LAUNCH_CHECK();
  const uint32_t* src[2] = {w.total2, w.total2 + 1};
  uint32_t got[2] = {0u, 0u};
  if (int e = pings::host_read_words(src, 2, got, st)) return e;
  *count = (int64_t)(((u64)got[1] << 32) | got[0]);
  return PINGS_OK;
}

PINGS_API int pings_frame_new_rows(const void* scratch, int64_t n, int64_t pool_offset, int64_t* rows,
                                   int64_t capacity, void* stream) {
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFF0 && capacity >= 0, "bad size");
  if (n == 0 || capacity == 0) return PINGS_OK;
  PINGS_ARG_CHECK(scratch && rows, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("frame_new_rows", st);
  NewScratch w = carve_new(const_cast<void*>(scratch), n);
  new_rows_kernel<<<(unsigned)((w.nchunks + 3) / 4), 256, 0, st>>>(w.bits, w.offsets, w.nchunks, n, pool_offset,
                                                                   reinterpret_cast<i64*>(rows), capacity);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_frame_static_mask(const float* sdf, const float* certainty, const float* grad, int64_t n,
                                      double certainty_thre, double sdf_thre, double min_grad_norm, uint8_t* mask,
                                      int64_t* dynamic_count, void* stream) {
  PINGS_ARG_CHECK(n >= 0 && dynamic_count, "null pointer or negative n");
  PINGS_ARG_CHECK(n == 0 || (sdf && certainty && mask), "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("frame_static_mask", st);
  PINGS_HIP_CHECK(hipMemsetAsync(dynamic_count, 0, sizeof(int64_t), st));
  if (n == 0) return PINGS_OK;
  const unsigned nb = blocks_for(n) < 2048u ? blocks_for(n) : 2048u;
  u64* cnt = reinterpret_cast<u64*>(dynamic_count);
  if (grad)
    static_mask_kernel<true><<<nb, 256, 0, st>>>(sdf, certainty, grad, n, (float)certainty_thre, (float)sdf_thre,
                                                 (float)min_grad_norm, mask, cnt);
  else
    static_mask_kernel<false><<<nb, 256, 0, st>>>(sdf, certainty, nullptr, n, (float)certainty_thre, (float)sdf_thre,
                                                  0.f, mask, cnt);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_frame_valid_scatter(const int64_t* rows, int64_t n, const float* sdf, const int64_t* nn_count,
                                        double sdf_thre, int64_t min_nn_count, const int64_t* local_idx,
                                        int64_t n_local, int64_t n_global, uint8_t* local_valid, uint8_t* valid,
                                        void* stream) {
  PINGS_ARG_CHECK(n >= 0 && n_local >= 0 && n_global >= 0, "negative count");
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(rows && sdf && nn_count && local_idx && local_valid && valid, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  pings::prof::Scope sc("frame_valid_scatter", st);
  valid_scatter_kernel<<<blocks_for(n), 256, 0, st>>>(reinterpret_cast<const i64*>(rows), n, sdf,
                                                      reinterpret_cast<const i64*>(nn_count), (float)sdf_thre,
                                                      min_nn_count, reinterpret_cast<const i64*>(local_idx), n_local,
                                                      n_global, local_valid, valid);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}
