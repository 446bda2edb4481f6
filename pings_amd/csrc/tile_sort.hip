// Tile sort of the rasteriser: a stable LSD radix sort of (key, element index) pairs over the low `bits` bits of the
// key, one digit (bits <= 8) or two (bits <= 16).  A pass is three launches — histogram, scan, scatter — with no state
// that outlives the pass: nothing to clear, no workgroup waits for another, and no atomic decides a position, so two
// runs (and the library sort) give the same bits.
//
//   histogram  workgroup b owns pairs [b * TS_BLOCK, (b + 1) * TS_BLOCK): digit counts in LDS -> table[digit][b]
//   scan       exclusive scan of the table into a second one (digit-major: base[d][b] is the first destination of
//              block b's pairs of digit d); every workgroup sums what lies in front of its chunk itself
//   scatter    the same blocks: wave w of a block owns its pairs [w * TS_WAVE, (w + 1) * TS_WAVE) in rounds of 64, so
//              the order (wave, round, lane) IS the input order; the rank of a pair among the block's pairs of its
//              digit = pairs of the digit in earlier waves (per-wave LDS counts) + in earlier rounds of its wave (a
//              running per-wave LDS counter, advanced by one lane per digit and round) + in lower lanes of its round
//              (ballots).  Pairs are staged in LDS in block-sorted order and leave in runs of equal digit, which are
//              contiguous in the destination.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "raster_common.hpp"

namespace pings {
namespace raster {

constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_WAVE = TS_BLOCK / TS_WAVES;    // pairs per wave
constexpr int TS_ROUNDS = TS_WAVE / 64;
constexpr int TS_BINS = 256;                    // widest digit
constexpr int TS_SCAN_THREADS = 1024, TS_SCAN_CHUNK = 4 * TS_SCAN_THREADS;   // words per workgroup of the scan
static_assert(TS_THREADS == TS_BINS, "the scatter kernel scans the block's digit counts one thread per bin");

template <typename KeyT>
__global__ __launch_bounds__(TS_THREADS) void tile_sort_hist_kernel(const KeyT* __restrict__ keys, uint32_t n, int shift,
                                                                     uint32_t nbins, uint32_t nblk,
                                                                     uint32_t* __restrict__ table) {
  __shared__ uint32_t cnt[TS_BINS];
  const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)TS_BLOCK;
  cnt[tid] = 0u;
  __syncthreads();
  // every load of the thread in flight before the first count
  constexpr int R = TS_BLOCK / TS_THREADS;
  uint32_t k[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = base + (uint32_t)r * TS_THREADS + tid;
    k[r] = i < n ? (uint32_t)keys[i] : 0u;
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (base + (uint32_t)r * TS_THREADS + tid < n) atomicAdd(&cnt[(k[r] >> shift) & (nbins - 1u)], 1u);   // counts only
  __syncthreads();
  if (tid < nbins) table[(size_t)tid * nblk + blockIdx.x] = cnt[tid];
}

// bases[i] = counts[0] + .. + counts[i - 1].  A workgroup owns TS_SCAN_CHUNK words and adds up everything in front of
// them itself (whole chunks: 16-byte loads, workgroup g reads g of them per thread): no carry is handed from workgroup
// to workgroup, so none waits and there is no state to clear.  The reads in front grow with the square of the table;
// at 64 k words (2 M pairs) the last workgroup reads 256 KB out of L2, and at 100 M pairs the launch would cost a few
// milliseconds next to a blend of tens of milliseconds.
__global__ __launch_bounds__(TS_SCAN_THREADS) void tile_sort_scan_kernel(const uint32_t* __restrict__ counts, uint32_t total,
                                                                         uint32_t* __restrict__ bases) {
  __shared__ uint32_t wsum[TS_SCAN_THREADS / 64], wfront[TS_SCAN_THREADS / 64];
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const uint4* front4 = reinterpret_cast<const uint4*>(counts);
  uint32_t front = 0u;
#pragma unroll 4
  for (uint32_t g = 0; g < blockIdx.x; ++g) {
    const uint4 q = front4[g * TS_SCAN_THREADS + tid];
    front += q.x + q.y + q.z + q.w;
  }
  const uint32_t i0 = blockIdx.x * (uint32_t)TS_SCAN_CHUNK + tid * 4u;
  uint32_t v[4];
  const bool full = i0 + 4u <= total;
  if (full) {
    const uint4 q = *reinterpret_cast<const uint4*>(counts + i0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < total ? counts[i0 + k] : 0u;
  }
  const uint32_t sum = v[0] + v[1] + v[2] + v[3];
  const uint32_t incl = wave_inclusive_sum(sum, lane);
  const uint32_t wave_front = wave_inclusive_sum(front, lane);
  if (lane == 63) {
    wsum[wave] = incl;
    wfront[wave] = wave_front;
  }
  __syncthreads();
  uint32_t run = incl - sum;
#pragma unroll
  for (int w = 0; w < TS_SCAN_THREADS / 64; ++w) run += wfront[w] + (w < wave ? wsum[w] : 0u);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = v[k];
    v[k] = run;
    run += x;
  }
  if (full) {
    *reinterpret_cast<uint4*>(bases + i0) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < total) bases[i0 + k] = v[k];
  }
}

// FIRST: the values are the element indices themselves (vals_in is not read)
template <typename KeyT, bool FIRST>
__global__ __launch_bounds__(TS_THREADS) void tile_sort_scatter_kernel(const KeyT* __restrict__ keys_in,
                                                                        const uint32_t* __restrict__ vals_in, uint32_t n,
                                                                        int shift, int dbits, uint32_t nblk,
                                                                        const uint32_t* __restrict__ table,
                                                                        KeyT* __restrict__ keys_out,
                                                                        uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t wcnt[TS_WAVES * TS_BINS];   // per (wave, digit): count, then the wave's next block-local position
  __shared__ uint32_t gbase[TS_BINS];             // per digit: destination of the block's first pair - its local position
  __shared__ uint32_t wtot[TS_WAVES];
  __shared__ uint32_t sval[TS_BLOCK];
  __shared__ KeyT skey[TS_BLOCK];
  const uint32_t tid = threadIdx.x, nbins = 1u << dbits, dmask = nbins - 1u;
  const int lane = tid & 63, wave = tid >> 6;
  const uint32_t base = blockIdx.x * (uint32_t)TS_BLOCK;
  const uint32_t first = base + (uint32_t)wave * TS_WAVE + (uint32_t)lane;
#pragma unroll
  for (int w = 0; w < TS_WAVES; ++w) wcnt[w * TS_BINS + tid] = 0u;
  __syncthreads();

  uint32_t k[TS_ROUNDS], v[TS_ROUNDS];
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const uint32_t i = first + (uint32_t)r * 64u;
    k[r] = i < n ? (uint32_t)keys_in[i] : 0u;
    if constexpr (FIRST) v[r] = i;
    else v[r] = i < n ? vals_in[i] : 0u;
  }
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r)
    if (first + (uint32_t)r * 64u < n) atomicAdd(&wcnt[wave * TS_BINS + ((k[r] >> shift) & dmask)], 1u);   // counts only
  __syncthreads();

  {
    // thread = digit: the block's pairs of smaller digits (exclusive scan over the digits), then wave by wave
    uint32_t c[TS_WAVES], tot = 0u;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) {
      c[w] = wcnt[w * TS_BINS + tid];
      tot += c[w];
    }
    const uint32_t incl = wave_inclusive_sum(tot, lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t loc = incl - tot;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) loc += w < wave ? wtot[w] : 0u;
    gbase[tid] = (tid < nbins ? table[(size_t)tid * nblk + blockIdx.x] : 0u) - loc;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) {
      wcnt[w * TS_BINS + tid] = loc;
      loc += c[w];
    }
  }
  __syncthreads();

  // LDS operations of a wave execute in order: a round reads the counter its predecessor advanced
  volatile uint32_t* next = wcnt + wave * TS_BINS;
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const bool valid = first + (uint32_t)r * 64u < n;
    const uint32_t d = (k[r] >> shift) & dmask;
    unsigned long long peers = __ballot(valid);   // lanes of this round with the same digit
    for (int b = 0; b < dbits; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    if (valid) {
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
      const uint32_t count = (uint32_t)__popcll(peers);
      const uint32_t start = next[d];
      if (below + 1u == count) next[d] = start + count;   // the digit's highest lane of the round
      const uint32_t pos = start + below;
      skey[pos] = (KeyT)k[r];
      sval[pos] = v[r];
    }
  }
  __syncthreads();

  const uint32_t count = n - base < (uint32_t)TS_BLOCK ? n - base : (uint32_t)TS_BLOCK;
  for (uint32_t i = tid; i < count; i += TS_THREADS) {
    const KeyT key = skey[i];
    const uint32_t dest = gbase[((uint32_t)key >> shift) & dmask] + i;
    if (dest < n) {   // always, when the table is the scan of this input's histogram
      keys_out[dest] = key;
      vals_out[dest] = sval[i];
    }
  }
}

size_t tile_sort_table_bytes(int64_t n) {
  // the counts and, behind them, their scan
  return 2 * align_up((size_t)TS_BINS * (size_t)ceil_div<int64_t>(std::max<int64_t>(n, 1), TS_BLOCK) * sizeof(uint32_t));
}

size_t tile_sort_library_bytes(int64_t n) {
  // the values come from a counting iterator: asked for with the iterator types of the call below
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                  rocprim::counting_iterator<uint32_t>(0u), (uint32_t*)nullptr, (size_t)n, 0u, 32u);
  (void)rocprim::radix_sort_pairs(nullptr, b, (uint16_t*)nullptr, (uint16_t*)nullptr,
                                  rocprim::counting_iterator<uint32_t>(0u), (uint32_t*)nullptr, (size_t)n, 0u, 16u);
  return std::max(a, b);
}

template <typename KeyT>
int tile_sort_library(const KeyT* keys_in, int64_t n, int bits, KeyT* keys_out, uint32_t* vals_out, void* temp,
                      size_t temp_bytes, hipStream_t st) {
  // the values are the slots themselves: a counting iterator, not an array of n words written to be read once
  PINGS_HIP_CHECK(rocprim::radix_sort_pairs(temp, temp_bytes, const_cast<KeyT*>(keys_in), keys_out,
                                            rocprim::counting_iterator<uint32_t>(0u), vals_out, (size_t)n, 0u,
                                            (unsigned)bits, st));
  return PINGS_OK;
}

template <typename KeyT>
static int tile_sort_pass(bool first, const KeyT* keys_in, const uint32_t* vals_in, uint32_t n, int shift, int dbits,
                          uint32_t* table, KeyT* keys_out, uint32_t* vals_out, hipStream_t st) {
  const uint32_t nblk = ceil_div<uint32_t>(n, TS_BLOCK), nbins = 1u << dbits;
  if (int e = launch(tile_sort_hist_kernel<KeyT>, dim3(nblk), TS_THREADS, 0, st, keys_in, n, shift, nbins, nblk, table))
    return e;
  uint32_t* bases = table + (size_t)TS_BINS * nblk;   // tile_sort_table_bytes: a multiple of 1 KB in front, 16-byte loads stay aligned
  if (int e = launch(tile_sort_scan_kernel, dim3(ceil_div<uint32_t>(nbins * nblk, TS_SCAN_CHUNK)), TS_SCAN_THREADS, 0, st,
                     (const uint32_t*)table, nbins * nblk, bases))
    return e;
  return with_flag(first, [&](auto f) {
    return launch(tile_sort_scatter_kernel<KeyT, f()>, dim3(nblk), TS_THREADS, 0, st, keys_in, vals_in, n, shift, dbits,
                  nblk, (const uint32_t*)bases, keys_out, vals_out);
  });
}

template <typename KeyT>
int tile_sort(const KeyT* keys_in, int64_t n, int bits, KeyT* keys_tmp, uint32_t* vals_tmp, KeyT* keys_out,
              uint32_t* vals_out, uint32_t* table, hipStream_t st) {
  PINGS_ARG_CHECK(bits >= 1 && bits <= 16 && n >= 0 && n < (int64_t)0x7FFFFFFF, "tile sort: 1..16 bits, fewer than 2^31 pairs");
  if (n == 0) return PINGS_OK;
  if (bits <= 8) return tile_sort_pass<KeyT>(true, keys_in, nullptr, (uint32_t)n, 0, bits, table, keys_out, vals_out, st);
  const int lo = (bits + 1) / 2;
  if (int e = tile_sort_pass<KeyT>(true, keys_in, nullptr, (uint32_t)n, 0, lo, table, keys_tmp, vals_tmp, st)) return e;
  return tile_sort_pass<KeyT>(false, keys_tmp, vals_tmp, (uint32_t)n, lo, bits - lo, table, keys_out, vals_out, st);
}

template int tile_sort<uint16_t>(const uint16_t*, int64_t, int, uint16_t*, uint32_t*, uint16_t*, uint32_t*, uint32_t*, hipStream_t);
template int tile_sort<uint32_t>(const uint32_t*, int64_t, int, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, hipStream_t);
template int tile_sort_library<uint16_t>(const uint16_t*, int64_t, int, uint16_t*, uint32_t*, void*, size_t, hipStream_t);
template int tile_sort_library<uint32_t>(const uint32_t*, int64_t, int, uint32_t*, uint32_t*, void*, size_t, hipStream_t);

namespace {
struct TileSortScratch {
  uint32_t* table;
  uint32_t *keys_tmp, *vals_tmp;
  char* temp;
  size_t temp_bytes, total;
};
TileSortScratch carve_tile_sort(void* blob, int64_t n) {
  Carver c(blob);
  TileSortScratch s;
  const size_t m = (size_t)std::max<int64_t>(n, 1);
  s.table = c.take<uint32_t>(tile_sort_table_bytes(n) / sizeof(uint32_t));
  s.keys_tmp = c.take<uint32_t>(m);
  s.vals_tmp = c.take<uint32_t>(m);
  s.temp_bytes = align_up(tile_sort_library_bytes(n)) + 256;
  s.temp = c.take<char>(s.temp_bytes);
  s.total = c.total();
  return s;
}
}  // namespace

}  // namespace raster
}  // namespace pings

using namespace pings::raster;

PINGS_API size_t pings_raster_tile_sort_bytes(int64_t n, int32_t* block_pairs) {
  if (block_pairs) *block_pairs = TS_BLOCK;
  return carve_tile_sort(nullptr, n).total;
}

PINGS_API int pings_raster_tile_sort(const void* keys, int64_t n, int key_bytes, int bits, void* keys_sorted,
                                     uint32_t* values, void* scratch, int library, void* stream) {
  PINGS_ARG_CHECK(key_bytes == 2 || key_bytes == 4, "keys of 2 or 4 bytes");
  PINGS_ARG_CHECK(bits >= 1 && bits <= 8 * key_bytes, "bits out of range");
  PINGS_ARG_CHECK(n >= 0 && n < (int64_t)0x7FFFFFFF, "pair count out of range");
  if (n == 0) return PINGS_OK;
  PINGS_ARG_CHECK(keys && keys_sorted && values && scratch, "null pointer");
  hipStream_t st = pings::as_stream(stream);
  const TileSortScratch s = carve_tile_sort(scratch, n);
  auto run = [&](auto* out) -> int {
    using KeyT = std::remove_pointer_t<decltype(out)>;
    const KeyT* in = static_cast<const KeyT*>(keys);
    if (library || bits > 16) return tile_sort_library<KeyT>(in, n, bits, out, values, s.temp, s.temp_bytes, st);
    return tile_sort<KeyT>(in, n, bits, reinterpret_cast<KeyT*>(s.keys_tmp), s.vals_tmp, out, values, s.table, st);
  };
  return key_bytes == 2 ? run(static_cast<uint16_t*>(keys_sorted)) : run(static_cast<uint32_t*>(keys_sorted));
}
