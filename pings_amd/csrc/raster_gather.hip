// Gaussian(-surfel) rasteriser, tile lists without a tile sort, for gfx950.
//
// Where every tile saturates (the headline, close views of dense maps) the kept (Gaussian, tile) instances all lie in
// a FRONT of a few thousand depth ranks (GeomState::occ_front, from frame_summary_kernel), each of which keeps hundreds
// of tiles.  The sort path writes those instances out in depth order and radix-sorts them by tile, only to learn which
// front ranks cover which tile; here every tile reads that off the front directly, in three launches:
//   front_rows_kernel          a wave per front rank: an 8-byte entry (rectangle, rank bucket), the first slot of every
//                              rectangle row (slots number a Gaussian's kept tiles row-major, as duplicate_kernel does),
//                              gval over the rank's slots; trailing workgroups store the zeros of per_gaussian
//   tile_gather_kernel<true>   a wave per tile walks the entries in ascending rank and counts the ranks that keep it
//   tile_gather_kernel<false>  the same walk again, now storing point_list[begin + k] = slot of the k-th keeper; every
//                              workgroup sums the counts in front of its tiles itself (no scan launch) and writes their
//                              ranges, and one more workgroup sorts the tiles by count: the forward dispatch order
// A (rank, tile) pair is kept iff the tile lies in the rank's rectangle and rank_bucket(rank) <= occ_bsat[tile]: the
// rule the tile bitmasks encode.  Ranks are visited in ascending order, so a tile's list is in depth order with ties by
// index, which is what the stable tile sort yields: gval, ranges and point_list are the sort path's, word for word.
// No atomics on global memory, and no workgroup waits for another.
#include <algorithm>

#include "raster_common.hpp"

namespace pings {
namespace raster {

// front entry: x = xmin | ymin << 8 | (width - 1) << 16 | (height - 1) << 24 in tiles (gather_fits: at most 256 tiles
// a side), y = the rank's bucket (below 256: occlusion_buckets) | rank << 8; FRONT_EMPTY in x's place marks a rank
// inside the front that keeps nothing (no rectangle has xmin = ymin = 255 and a width and height of 256).
constexpr uint32_t FRONT_EMPTY = 0xFFFFFFFFu;
constexpr int GATHER_WAVES = 16;   // tiles (waves) of a workgroup of tile_gather_kernel: they share the staged entries
constexpr int GATHER_THREADS = GATHER_WAVES * 64;

// The row table is [gy][front_cap], by ABSOLUTE tile row: the wave of a tile reads one row of it at consecutive ranks.
__global__ __launch_bounds__(256) void front_rows_kernel(int P, int gx, int nb, int words, uint32_t front_cap, int64_t I,
                                                         int rank_blocks, const uint32_t* __restrict__ gidx_sorted,
                                                         const uint32_t* __restrict__ offsets_sorted,
                                                         const uint32_t* __restrict__ tiles_sorted,
                                                         const uint4* __restrict__ rect,
                                                         const unsigned long long* __restrict__ mask,
                                                         const uint32_t* __restrict__ nvalid,
                                                         const uint32_t* __restrict__ front_dev,
                                                         uint2* __restrict__ entries, uint32_t* __restrict__ rowbase,
                                                         uint32_t* __restrict__ gval,
                                                         uint32_t* __restrict__ per_gaussian) {
  if ((int)blockIdx.x >= rank_blocks) {
    // the zeros of the per-Gaussian sums (per_gaussian_sum_kernel stores only where a Gaussian kept a tile), by the
    // workgroups behind the ranks'
    const size_t stride = (size_t)(gridDim.x - rank_blocks) * 256u;
    for (size_t i = (size_t)((int)blockIdx.x - rank_blocks) * 256u + threadIdx.x; i < (size_t)P; i += stride)
      per_gaussian[i] = 0u;
    return;
  }
  const int lane = threadIdx.x & 63;
  const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= min(*front_dev, front_cap)) return;
  const uint32_t kept = tiles_sorted[r];
  const uint32_t bk = rank_bucket((int)r, nb, *nvalid);
  if (kept == 0u) {
    if (lane == 0) entries[r] = make_uint2(FRONT_EMPTY, bk | (r << 8));
    return;
  }
  const uint32_t g = gidx_sorted[r];
  const uint4 rc = rect[g];
  const int xmin = (int)(rc.y & 0xFFFF), ymin = (int)(rc.y >> 16);
  const int wdt = max((int)(rc.z & 0xFFFF) - xmin, 1), hgt = max((int)(rc.z >> 16) - ymin, 1);
  if (lane == 0)
    entries[r] = make_uint2((uint32_t)xmin | ((uint32_t)ymin << 8) | ((uint32_t)(wdt - 1) << 16) | ((uint32_t)(hgt - 1) << 24),
                            bk | (r << 8));
  // kept tiles per rectangle row, lanes as rows, and their exclusive sum from the rank's first slot on
  const unsigned long long* mrow = mask + (size_t)bk * words;
  const uint32_t first = offsets_sorted[r] - kept;
  uint32_t run = first;
  for (int y0 = 0; y0 < hgt; y0 += 64) {
    const int y = y0 + lane;
    uint32_t c = 0u;
    if (y < hgt) {
      const int s = (ymin + y) * gx + xmin;
      for (int x = 0; x < wdt; x += 64) c += (uint32_t)__popcll(kept_bits(mrow, s + x, min(64, wdt - x)));
    }
    const uint32_t incl = wave_inclusive_sum_dpp(c);
    if (y < hgt) rowbase[(size_t)(ymin + y) * front_cap + r] = run + (incl - c);
    run += lane_value(incl, 63);
  }
  // slots [first, first + kept) belong to this Gaussian: one contiguous run
  for (uint32_t i = (uint32_t)lane; i < kept; i += 64u)
    if ((int64_t)first + i < I) gval[first + i] = g;
}

// COUNT: counts[tile] = ranks of the front that keep the tile.  !COUNT: their slots, in ascending rank, from the sum of
// the counts in front of the tile on, and the tile's range; workgroup 0 does not gather but orders the tiles by count.
// A workgroup owns GATHER_WAVES consecutive tiles, a wave each.  It stages the front entries in LDS, GATHER_CHUNK at a
// time, and keeps only those that can matter to one of its tiles: a rectangle that meets the tiles' rows (and columns,
// where they lie in one row) and a bucket up to the last one any of them needs — a front rank keeps a tenth of the
// image, so the waves walk a fraction of the front.  The order of the ranks survives the compaction.  A wave leaves
// the walk at the first step whose first rank lies in a bucket behind its tile's last needed one (buckets ascend with
// the rank), but keeps meeting the workgroup's barriers.
template <bool COUNT>
__global__ __launch_bounds__(GATHER_THREADS) void tile_gather_kernel(int gx, int num_tiles, int words, uint32_t front_cap,
                                                                     int64_t I, const uint32_t* __restrict__ front_dev,
                                                                     const uint2* __restrict__ entries,
                                                                     const uint32_t* __restrict__ rowbase,
                                                                     const uint16_t* __restrict__ bsat,
                                                                     const unsigned long long* __restrict__ mask,
                                                                     uint32_t* __restrict__ counts,
                                                                     uint2* __restrict__ ranges,
                                                                     uint32_t* __restrict__ point_list,
                                                                     uint32_t* __restrict__ order) {
  __shared__ uint2 sEnt[GATHER_CHUNK];
  __shared__ uint32_t sWave[GATHER_WAVES];
  __shared__ uint32_t sSat[GATHER_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int group = (int)blockIdx.x;
  if constexpr (!COUNT) {
    if (group == 0) {   // first in the grid: one workgroup's serial job runs beside the others' walks
      tile_order_body<false>(counts, nullptr, num_tiles, order, nullptr, 0u, 0u);
      return;
    }
    --group;
  }
  const int tile0 = group * GATHER_WAVES, tile = tile0 + wave;
  const bool live = tile < num_tiles;
  const uint32_t F = min(*front_dev, front_cap);
  const int ty = live ? tile / gx : 0, tx = live ? tile - ty * gx : 0;
  const uint32_t sat = live ? (uint32_t)bsat[tile] : 0u;
  // the workgroup's tiles: rows ty0 .. ty1, columns tx0 .. tx1 where that is one row; the last bucket any of them needs
  const int tlast = min(tile0 + GATHER_WAVES, num_tiles) - 1;
  const int ty0 = tile0 / gx, ty1 = tlast / gx;
  const int tx0 = ty0 == ty1 ? tile0 - ty0 * gx : 0, tx1 = ty0 == ty1 ? tlast - ty0 * gx : gx - 1;
  if (lane == 0) sSat[wave] = live ? min(sat, 255u) : 0u;
  uint32_t begin = 0u;
  if constexpr (!COUNT) {
    // tiles in front of the workgroup's: every thread a strided share, summed over the workgroup; then those of the
    // workgroup's own tiles in front of the wave's
    uint32_t s = 0u;
    for (int t = (int)threadIdx.x; t < tile0; t += GATHER_THREADS) s += counts[t];
    s = wave_reduce_sum_u32_dpp(s);
    if (lane == 63) sWave[wave] = s;
    __syncthreads();
    const int t = tile0 + lane;
    uint32_t b = lane < GATHER_WAVES ? sWave[lane] : 0u;
    if (lane < wave && t < num_tiles) b += counts[t];
    begin = lane_value(wave_reduce_sum_u32_dpp(b), 63);
  }
  __syncthreads();
  uint32_t wgsat = 0u;
#pragma unroll
  for (int w = 0; w < GATHER_WAVES; ++w) wgsat = max(wgsat, sSat[w]);
  uint32_t running = 0u;
  bool done = !live;
  for (uint32_t c0 = 0u; c0 < F; c0 += (uint32_t)GATHER_CHUNK) {
    const uint32_t n = min((uint32_t)GATHER_CHUNK, F - c0);
    // stage and compact the chunk, GATHER_THREADS entries a round, in rank order
    uint32_t ncomp = 0u;
    for (uint32_t k0 = 0u; k0 < n; k0 += (uint32_t)GATHER_THREADS) {
      const uint32_t k = k0 + threadIdx.x;
      uint2 e = make_uint2(FRONT_EMPTY, 0u);
      if (k < n) e = entries[c0 + k];
      const int x0 = (int)(e.x & 255u), y0 = (int)((e.x >> 8) & 255u);
      const int x1 = x0 + (int)((e.x >> 16) & 255u), y1 = y0 + (int)(e.x >> 24);
      const bool keep = e.x != FRONT_EMPTY && (e.y & 255u) <= wgsat && y0 <= ty1 && y1 >= ty0 && x0 <= tx1 && x1 >= tx0;
      const unsigned long long m = __ballot(keep);
      __syncthreads();   // the walks of the previous chunk, and the previous round's reads of sWave, are over
      if (lane == 0) sWave[wave] = (uint32_t)__popcll(m);
      __syncthreads();
      uint32_t at = ncomp, tot = 0u;
#pragma unroll
      for (int w = 0; w < GATHER_WAVES; ++w) {
        const uint32_t c = sWave[w];
        at += w < wave ? c : 0u;
        tot += c;
      }
      if (keep) sEnt[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = e;
      ncomp += tot;
    }
    __syncthreads();
    if (done) continue;
    for (uint32_t k0 = 0u; k0 < ncomp; k0 += 64u) {
      const uint32_t k = k0 + (uint32_t)lane;
      const uint2 e = sEnt[min(k, ncomp - 1u)];
      if ((lane_value(e.y, 0) & 255u) > sat) { done = true; break; }
      const uint32_t dx = (uint32_t)tx - (e.x & 255u), dy = (uint32_t)ty - ((e.x >> 8) & 255u);
      const bool hit = k < ncomp && (e.y & 255u) <= sat && dx <= ((e.x >> 16) & 255u) && dy <= (e.x >> 24);
      const unsigned long long m = __ballot(hit);
      if constexpr (!COUNT) {
        if (hit) {
          // the tile's slot: first slot of its rectangle row + kept tiles of that row to its left
          uint32_t slot = rowbase[(size_t)ty * front_cap + (e.y >> 8)];
          if (dx != 0u) {
            const unsigned long long* mrow = mask + (size_t)(e.y & 255u) * words;
            const int s = tile - (int)dx;
            for (int x = 0; x < (int)dx; x += 64) slot += (uint32_t)__popcll(kept_bits(mrow, s + x, min(64, (int)dx - x)));
          }
          const uint32_t pos = begin + running + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          if ((int64_t)pos < I) point_list[pos] = slot;
        }
      }
      running += (uint32_t)__popcll(m);
    }
  }
  if (live && lane == 0) {
    if constexpr (COUNT) {
      counts[tile] = running;
    } else if (running != 0u) {
      // a tile without an instance keeps the zeros of the frame's clear, as tile_ranges_kernel leaves them
      ranges[tile] = make_uint2(begin, begin + running);
    }
  }
}

int launch_tile_gather(const KParams& kp, int P, int64_t I, uint32_t front, const GeomState& gs, const BinState& bs,
                       void* per_gaussian, hipStream_t st) {
  const int num_tiles = kp.gx * kp.gy;
  PINGS_ARG_CHECK(gather_fits(front, kp.gx, kp.gy, gs.occ_nb, I), "the gather tables do not fit this frame");
  // tables in what only the sort path uses: front entries in slot_val (8 front <= 4 I bytes), the row table
  // [gy][front] in tile_key and tile_key_sorted behind it (front gy <= 2 I words); the counts in tile_work, which the
  // backward fills much later
  uint2* entries = reinterpret_cast<uint2*>(bs.slot_val);
  uint32_t* rowbase = bs.tile_key;
  uint32_t* counts = bs.tile_work;
  {
    pings::prof::Scope ps("front_rows", st);
    const int rank_blocks = (int)pings::ceil_div<uint32_t>(front, 4u);
    const int zero_blocks = std::min(std::max(pings::ceil_div(P, 2048), 1), 1024);
    hipLaunchKernelGGL(front_rows_kernel, dim3(rank_blocks + zero_blocks), dim3(256), 0, st, P, kp.gx, gs.occ_nb,
                       gs.occ_words, front, I, rank_blocks, gs.gidx_sorted, gs.offsets_sorted, gs.tiles_sorted, gs.rect,
                       gs.occ_mask, gs.nvalid, gs.occ_front, entries, rowbase, bs.gval,
                       reinterpret_cast<uint32_t*>(per_gaussian));
    PINGS_LAUNCH_CHECK();
  }
  const int groups = pings::ceil_div(num_tiles, GATHER_WAVES);
  {
    pings::prof::Scope ps("tile_gather", st);
    hipLaunchKernelGGL(tile_gather_kernel<true>, dim3(groups), dim3(GATHER_THREADS), 0, st, kp.gx, num_tiles,
                       gs.occ_words, front, I, gs.occ_front, entries, rowbase, gs.occ_bsat, gs.occ_mask, counts, bs.ranges,
                       bs.point_list, bs.tile_order);
    PINGS_LAUNCH_CHECK();
    // + the workgroup of the forward tile order
    hipLaunchKernelGGL(tile_gather_kernel<false>, dim3(groups + 1), dim3(GATHER_THREADS), 0, st, kp.gx, num_tiles,
                       gs.occ_words, front, I, gs.occ_front, entries, rowbase, gs.occ_bsat, gs.occ_mask, counts, bs.ranges,
                       bs.point_list, bs.tile_order);
    PINGS_LAUNCH_CHECK();
  }
  return PINGS_OK;
}

}  // namespace raster
}  // namespace pings
