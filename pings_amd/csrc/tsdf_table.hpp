// The block key and the open-addressing table of the sparse TSDF volume, shared by the depth-view kernels
// (tsdf.hip) and the point-cloud kernels (tsdf_points.hip).
#pragma once

#include "common.hpp"

namespace pings {
namespace tsdf {

using i64 = int64_t;
using u64 = unsigned long long;
constexpr int kBlock = 256;
constexpr int kB = PINGS_TSDF_BLOCK;             // voxels per block edge
constexpr int kVox = kB * kB * kB;               // 512
constexpr i64 kBias = (i64)1 << 20;              // block coordinates live in [-2^20, 2^20)
constexpr i64 kFree = -1;
static_assert(kB == 8, "the voxel index packs three 3-bit coordinates");

__host__ __device__ inline i64 pack_key(i64 bx, i64 by, i64 bz) {
  return (bx + kBias) << 42 | (by + kBias) << 21 | (bz + kBias);
}
__host__ __device__ inline bool in_extent(i64 b) { return b >= -kBias && b < kBias; }

__device__ __forceinline__ i64 table_home(i64 key, i64 mask) {
  u64 h = (u64)key * 0x9E3779B97F4A7C15ull;     // Fibonacci hashing: neighbouring blocks spread over the table
  return (i64)(h >> 20) & mask;
}

// Entry of `key`, or -1 when it is absent.  Keys are written by earlier launches only.
__device__ __forceinline__ i64 table_find(const i64* __restrict__ tkeys, i64 tsize, i64 key) {
  const i64 mask = tsize - 1;
  i64 e = table_home(key, mask);
  for (i64 probe = 0; probe < tsize; ++probe) {
    const i64 cur = tkeys[e];
    if (cur == key) return e;
    if (cur == kFree) return -1;
    e = (e + 1) & mask;
  }
  return -1;
}

// Entry of `key`, inserted when absent; -1 only when the table has no free entry.
__device__ __forceinline__ i64 table_find_or_insert(i64* tkeys, i64 tsize, i64 key) {
  const i64 mask = tsize - 1;
  i64 e = table_home(key, mask);
  for (i64 probe = 0; probe < tsize; ++probe) {
    i64 cur = __hip_atomic_load(&tkeys[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kFree) cur = (i64)atomicCAS(reinterpret_cast<u64*>(&tkeys[e]), (u64)kFree, (u64)key);
    if (cur == kFree || cur == key) return e;
    e = (e + 1) & mask;
  }
  return -1;
}

inline bool table_ok(const void* tkeys, const void* tslots, i64 tsize) {
  return tkeys && tslots && tsize >= 64 && tsize < ((i64)1 << 31) && (tsize & (tsize - 1)) == 0;
}

}  // namespace tsdf
}  // namespace pings
