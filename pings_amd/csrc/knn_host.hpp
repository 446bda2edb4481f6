// Host side of the neural-point kernels (device side: knn_common.hpp): the map check and the two grid rules.
#pragma once
#include <mutex>
#include <unordered_map>

#include "knn_common.hpp"

namespace pings_knn {

inline int check_map(const pings_knn_map* m) {
  PINGS_ARG_CHECK(m != nullptr, "null map");
  PINGS_ARG_CHECK((m->table || m->compact) && m->buffer_size > 0 && m->neural_points && m->neighbor_dx,
                  "null map pointer");
  PINGS_ARG_CHECK(m->buffer_size < (1LL << 31), "buffer_size must be below 2^31");
  PINGS_ARG_CHECK(!m->compact || ((m->compact_mask & (m->compact_mask + 1u)) == 0u), "compact_mask must be 2^k - 1");
  PINGS_ARG_CHECK(m->K > 0 && m->K <= 128, "K must be in 1..128");
  PINGS_ARG_CHECK(m->nn_k > 0 && m->nn_k <= MAX_NNK && m->nn_k <= m->K, "nn_k must be in 1..16");
  PINGS_ARG_CHECK(!m->time_filtering || (m->point_ts_create && m->travel_dist), "time filtering needs ts / travel_dist");
  PINGS_ARG_CHECK(!m->use_free_mask || m->free_mask, "use_free_mask without mask");
  PINGS_ARG_CHECK(!m->use_valid_mask || m->valid_mask, "use_valid_mask without mask");
  PINGS_ARG_CHECK(m->resolution > 0.f, "resolution must be positive");
  PINGS_ARG_CHECK(!m->blocks || (m->block_records && m->blocks_ok && ((m->block_mask & (m->block_mask + 1u)) == 0u)),
                  "cell-block index needs its records, its status word and a 2^k - 1 mask");
  return PINGS_OK;
}

// Workgroups of a wave-per-query kernel: ONE resident round (what the occupancy calculator says fits on the chip at
// once), the waves loop over the remaining queries.  Measured on the fused SDF forward (1M points): B = 16,384 0.066 ->
// 0.047 ms, B = 131,072 0.310 -> 0.268 ms against a fixed 8,192-workgroup grid — the per-wave prologue (decoder weights,
// lane constants) is paid once per resident wave, and a second, nearly empty round is the worst case.
// The occupancy of a kernel is asked for once and kept.
inline unsigned resident_grid(long long B, const void* kernel) {
  const long long blocks = (B + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  static std::mutex mu;
  static std::unordered_map<const void*, long long> resident;
  std::lock_guard<std::mutex> lock(mu);
  auto it = resident.find(kernel);
  if (it == resident.end()) {
    long long v = 256LL * 4;
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, 64 * WAVES_PER_BLOCK, 0) == hipSuccess &&
        cus > 0 && per > 0)
      v = (long long)cus * per;
    it = resident.emplace(kernel, v).first;
  }
  return (unsigned)(blocks < it->second ? blocks : it->second);
}

// The search-only kernels (knn_search, query_feature forward) have next to no prologue and measured the other way
// round (1M points, B = 131,072: 0.105 ms with 8,192 short-lived workgroups, 0.134 ms with one resident round): they
// get a fixed 8,192 cap.
inline unsigned capped_grid(long long B) {
  const long long blocks = (B + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  return (unsigned)(blocks < 8192 ? blocks : 8192);
}

}  // namespace pings_knn
