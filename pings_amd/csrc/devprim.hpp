// Device-wide scans, sorts, reductions and selections of the library (rocPRIM through hipcub), as plain functions: a
// closed list, one entry per type combination some call site uses.  devprim.hip is the only translation unit outside
// the 3D rasteriser that includes hipcub, so these kernels are compiled once.
//
// For each primitive: X_temp_bytes(n) is the temporary storage rocPRIM asks for at n items (n < 1 counts as 1), and
// X(temp, temp_bytes, ..., n, stream) runs it with the storage the caller reserved and returns a PINGS status;
// storage that is too small is rocPRIM's own error.  n fits an int.  Radix sorts compare key bits [begin_bit, end_bit).
#pragma once
#include "common.hpp"

namespace pings {
namespace devprim {

using u32 = uint32_t;
using u64 = unsigned long long;

size_t exclusive_sum_u32_temp_bytes(int64_t n);
int exclusive_sum_u32(void* temp, size_t temp_bytes, const u32* in, u32* out, int64_t n, hipStream_t st);
size_t exclusive_sum_i32_temp_bytes(int64_t n);
int exclusive_sum_i32(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int64_t n, hipStream_t st);

size_t inclusive_sum_u32_temp_bytes(int64_t n);
int inclusive_sum_u32(void* temp, size_t temp_bytes, const u32* in, u32* out, int64_t n, hipStream_t st);
size_t inclusive_sum_i32_temp_bytes(int64_t n);
int inclusive_sum_i32(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int64_t n, hipStream_t st);
size_t inclusive_sum_i64_temp_bytes(int64_t n);
int inclusive_sum_i64(void* temp, size_t temp_bytes, const int64_t* in, int64_t* out, int64_t n, hipStream_t st);

// out[i] = max(in[0..i])
size_t inclusive_max_u32_temp_bytes(int64_t n);
int inclusive_max_u32(void* temp, size_t temp_bytes, const u32* in, u32* out, int64_t n, hipStream_t st);

size_t sort_pairs_u32_u32_temp_bytes(int64_t n);
int sort_pairs_u32_u32(void* temp, size_t temp_bytes, const u32* keys, u32* keys_out, const u32* vals, u32* vals_out,
                       int64_t n, int begin_bit, int end_bit, hipStream_t st);
size_t sort_pairs_u64_u32_temp_bytes(int64_t n);
int sort_pairs_u64_u32(void* temp, size_t temp_bytes, const u64* keys, u64* keys_out, const u32* vals, u32* vals_out,
                       int64_t n, int begin_bit, int end_bit, hipStream_t st);
size_t sort_pairs_i64_u64_temp_bytes(int64_t n);
int sort_pairs_i64_u64(void* temp, size_t temp_bytes, const long long* keys, long long* keys_out, const u64* vals,
                       u64* vals_out, int64_t n, int begin_bit, int end_bit, hipStream_t st);
size_t sort_keys_i64_temp_bytes(int64_t n);
int sort_keys_i64(void* temp, size_t temp_bytes, const int64_t* keys, int64_t* keys_out, int64_t n, int begin_bit,
                  int end_bit, hipStream_t st);

// runs of equal neighbouring keys: keys_out[r] = the run's key, vals_out[r] = the smallest of its values, *runs_out =
// the number of runs
size_t reduce_min_by_key_i64_u64_temp_bytes(int64_t n);
int reduce_min_by_key_i64_u64(void* temp, size_t temp_bytes, const long long* keys, long long* keys_out,
                              const u64* vals, u64* vals_out, int* runs_out, int64_t n, hipStream_t st);

// out = the i in [0, n) with flags[i] != 0, ascending; *count_out = how many
size_t select_flagged_iota_i64_temp_bytes(int64_t n);
int select_flagged_iota_i64(void* temp, size_t temp_bytes, const uint8_t* flags, long long* out, long long* count_out,
                            int64_t n, hipStream_t st);

}  // namespace devprim
}  // namespace pings
