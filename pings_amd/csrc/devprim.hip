// The library's device-wide primitives (devprim.hpp): each function is one hipcub call with the types spelled out.
#include "devprim.hpp"

#include <hipcub/hipcub.hpp>

namespace pings {
namespace devprim {
namespace {

inline int items(int64_t n) { return (int)(n > 0 ? n : 1); }

}  // namespace

size_t exclusive_sum_u32_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const u32*)nullptr, (u32*)nullptr, items(n));
  return b;
}
int exclusive_sum_u32(void* temp, size_t temp_bytes, const u32* in, u32* out, int64_t n, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, (int)n, st));
  return PINGS_OK;
}

size_t exclusive_sum_i32_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, items(n));
  return b;
}
int exclusive_sum_i32(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int64_t n, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, (int)n, st));
  return PINGS_OK;
}

size_t inclusive_sum_u32_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (const u32*)nullptr, (u32*)nullptr, items(n));
  return b;
}
int inclusive_sum_u32(void* temp, size_t temp_bytes, const u32* in, u32* out, int64_t n, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, in, out, (int)n, st));
  return PINGS_OK;
}

size_t inclusive_sum_i32_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, items(n));
  return b;
}
int inclusive_sum_i32(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int64_t n, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, in, out, (int)n, st));
  return PINGS_OK;
}

size_t inclusive_sum_i64_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr, items(n));
  return b;
}
int inclusive_sum_i64(void* temp, size_t temp_bytes, const int64_t* in, int64_t* out, int64_t n, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, in, out, (int)n, st));
  return PINGS_OK;
}

size_t inclusive_max_u32_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::InclusiveScan(nullptr, b, (const u32*)nullptr, (u32*)nullptr, hipcub::Max(), items(n));
  return b;
}
int inclusive_max_u32(void* temp, size_t temp_bytes, const u32* in, u32* out, int64_t n, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceScan::InclusiveScan(temp, temp_bytes, in, out, hipcub::Max(), (int)n, st));
  return PINGS_OK;
}

size_t sort_pairs_u32_u32_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const u32*)nullptr, (u32*)nullptr, (const u32*)nullptr,
                                           (u32*)nullptr, items(n));
  return b;
}
int sort_pairs_u32_u32(void* temp, size_t temp_bytes, const u32* keys, u32* keys_out, const u32* vals, u32* vals_out,
                       int64_t n, int begin_bit, int end_bit, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, vals, vals_out, (int)n,
                                                     begin_bit, end_bit, st));
  return PINGS_OK;
}

size_t sort_pairs_u64_u32_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr,
                                           (u32*)nullptr, items(n));
  return b;
}
int sort_pairs_u64_u32(void* temp, size_t temp_bytes, const u64* keys, u64* keys_out, const u32* vals, u32* vals_out,
                       int64_t n, int begin_bit, int end_bit, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, vals, vals_out, (int)n,
                                                     begin_bit, end_bit, st));
  return PINGS_OK;
}

size_t sort_pairs_i64_u64_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const long long*)nullptr, (long long*)nullptr,
                                           (const u64*)nullptr, (u64*)nullptr, items(n));
  return b;
}
int sort_pairs_i64_u64(void* temp, size_t temp_bytes, const long long* keys, long long* keys_out, const u64* vals,
                       u64* vals_out, int64_t n, int begin_bit, int end_bit, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, vals, vals_out, (int)n,
                                                     begin_bit, end_bit, st));
  return PINGS_OK;
}

size_t sort_keys_i64_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr, items(n));
  return b;
}
int sort_keys_i64(void* temp, size_t temp_bytes, const int64_t* keys, int64_t* keys_out, int64_t n, int begin_bit,
                  int end_bit, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, keys, keys_out, (int)n, begin_bit, end_bit, st));
  return PINGS_OK;
}

size_t reduce_min_by_key_i64_u64_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceReduce::ReduceByKey(nullptr, b, (const long long*)nullptr, (long long*)nullptr,
                                          (const u64*)nullptr, (u64*)nullptr, (int*)nullptr, hipcub::Min(), items(n));
  return b;
}
int reduce_min_by_key_i64_u64(void* temp, size_t temp_bytes, const long long* keys, long long* keys_out,
                              const u64* vals, u64* vals_out, int* runs_out, int64_t n, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceReduce::ReduceByKey(temp, temp_bytes, keys, keys_out, vals, vals_out, runs_out,
                                                    hipcub::Min(), (int)n, st));
  return PINGS_OK;
}

size_t select_flagged_iota_i64_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceSelect::Flagged(nullptr, b, hipcub::CountingInputIterator<long long>(0), (const uint8_t*)nullptr,
                                      (long long*)nullptr, (long long*)nullptr, items(n));
  return b;
}
int select_flagged_iota_i64(void* temp, size_t temp_bytes, const uint8_t* flags, long long* out, long long* count_out,
                            int64_t n, hipStream_t st) {
  PINGS_HIP_CHECK(hipcub::DeviceSelect::Flagged(temp, temp_bytes, hipcub::CountingInputIterator<long long>(0), flags,
                                                out, count_out, (int)n, st));
  return PINGS_OK;
}

}  // namespace devprim
}  // namespace pings
