// Gaussian(-surfel) rasteriser, what the host decides before any kernel runs: the layout of the opaque blobs (carve_*,
// the *_bytes entry points, the debug taps that read a blob back), the PINGS_* environment knobs (read_knobs) and
// which blend kernels a view runs, forward and backward (blend_plan).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "raster_common.hpp"

namespace pings {
namespace raster {

// ---------------------------------------------------------------- blob carving
static size_t sort_temp_bytes(int64_t n) {
  size_t a = 0, b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                     (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 32);
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                         (int)std::max<int64_t>(n, DS_NB + n / 256 + 2));
  size_t c = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, c, (uint16_t*)nullptr, (uint16_t*)nullptr,
                                           (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 16);
  if (c > a) a = c;
  // the tile sort: the library's scratch (its values come from a counting iterator: its own size) or the digit table
  a = std::max(a, std::max(tile_sort_library_bytes(n), tile_sort_table_bytes(n)));
  // the scans: the library's scratch or the totals table
  a = std::max(a, raster_scan_bytes(std::max<int64_t>(n, DS_NB + n / 256 + 2)));
  return align_up(a > b ? a : b) + 256;
}

// rank buckets per tile of the occlusion budget: ~2M counters in total, 32..256 per tile
int occlusion_buckets(int num_tiles) {
  int nb = 256;
  while (nb > 32 && (size_t)nb * (size_t)num_tiles > ((size_t)1 << 21)) nb >>= 1;
  return nb;
}

GeomState carve_geom(void* blob, int P, int num_tiles) {
  Carver c(blob);
  GeomState g;
  const size_t n = (size_t)(P > 0 ? P : 1);
  const size_t nt = (size_t)(num_tiles > 0 ? num_tiles : 1);
  g.rec = c.take<float4>(4 * n);
  g.rect = c.take<uint4>(n);
  g.depth_key = c.take<uint32_t>(n);
  g.depth_key_sorted = c.take<uint32_t>(n);
  g.gidx = c.take<uint32_t>(n);
  g.gidx_sorted = c.take<uint32_t>(n);
  g.rank_of = c.take<uint32_t>(n);
  g.tiles_sorted = c.take<uint32_t>(n);
  g.offsets_sorted = c.take<uint32_t>(n);
  g.occ_nb = occlusion_buckets((int)nt);
  // occ_bucket, stats and ds_head start every frame at zero: adjacent, ONE memset (zero_begin .. zero_end)
  g.occ_bucket = c.take<uint32_t>(nt * (size_t)g.occ_nb);
  // sharded pairs before culling, visible Gaussians, kept pairs, then one word: occ_bmax (STAT_*: raster_common.hpp)
  g.stats = c.take<unsigned long long>(STAT_WORDS);
  g.occ_bmax = g.stats ? reinterpret_cast<uint32_t*>(g.stats + STAT_BMAX) : nullptr;
  g.occ_front = g.occ_bmax ? g.occ_bmax + 1 : nullptr;   // the other half of that word
  const size_t nblk = (n + 255) / 256;                  // workgroups of the per-Gaussian kernels
  g.ds_words = DS_HEAD + (size_t)DS_NB + nblk;          // header, counts (+ per-block culled)
  g.ds_head = c.take<uint32_t>(g.ds_words);
  g.ds_cnt = g.ds_head ? g.ds_head + DS_HEAD : nullptr;
  g.zero_begin = reinterpret_cast<char*>(g.occ_bucket);
  // up to the 256-byte boundary the next field starts at: a clear whose size is not a multiple of 16 bytes costs the
  // runtime a second fill launch for the tail
  g.zero_bytes = g.ds_head ? align_up((size_t)(reinterpret_cast<char*>(g.ds_head + g.ds_words) - g.zero_begin)) : 0;
  g.occ_bsat = c.take<uint16_t>(nt);
  // + 1: the row walks read a bit range as two neighbouring words, the second of which may lie one past the table
  g.occ_words = (int)((nt + 63) / 64);
  g.occ_mask = c.take<unsigned long long>((size_t)g.occ_nb * (size_t)g.occ_words + 1);
  g.nvalid = c.take<uint32_t>(1);
  g.ds_off = c.take<uint32_t>((size_t)DS_NB + nblk + 1);
  g.ds_idx = c.take<uint32_t>(n);
  g.summary = c.take<FrameSummary>(1);            // what the frame's one read-back fetches
  g.temp_bytes = sort_temp_bytes((int64_t)n);
  g.temp = c.take<char>(g.temp_bytes);
  g.total = c.total();
  return g;
}

BinState carve_binning(void* blob, int64_t I, int num_tiles, uint32_t seg) {
  Carver c(blob);
  BinState b;
  const size_t n = (size_t)(I > 0 ? I : 1);
  b.point_list = c.take<uint32_t>(n);
  // ranges, inst_w, inst_qmask (and inst_cnt, 3DGS) start at zero: adjacent, ONE memset from `ranges`
  b.ranges = c.take<uint2>((size_t)num_tiles);
  b.inst_w = c.take<float>(n + 1);
  b.inst_qmask = c.take<uint8_t>(n + 1);
  b.inst_cnt = c.take<uint32_t>(n);
  b.inst_wq = c.take<float>(4 * n);
  b.inst_cntq = c.take<uint32_t>(4 * n);
  b.tile_key = c.take<uint32_t>(n);
  b.tile_key_sorted = c.take<uint32_t>(n);
  b.gval = c.take<uint32_t>(n);
  // the fields up to tile_maxc keep their offsets, which tests/test_raster_glue.py reads straight out of the blob
  b.slot_val = c.take<uint32_t>(n);
  b.tile_order = c.take<uint32_t>(2 * (size_t)num_tiles + 4);   // + the backward pass' long-list tile count
  b.tile_work = c.take<uint32_t>((size_t)num_tiles);
  b.tile_maxc = c.take<uint32_t>((size_t)num_tiles);
  // units of SEG entries for lists beyond 2 SEG: at most I / SEG + I / (2 SEG) of them
  const size_t sg = (size_t)seg;
  b.seg_max_units = sg ? (uint32_t)(n / sg + n / (2 * sg) + 64) : 1u;
  if (b.seg_max_units > (1u << 20)) b.seg_max_units = 1u << 20;   // forced tiny segments (tests): capacity is checked on device
  b.seg_head = c.take<uint32_t>(4);
  b.seg_unit_tile = c.take<uint32_t>(b.seg_max_units);
  b.seg_unit_seg = c.take<uint32_t>(b.seg_max_units);
  b.seg_tile_unit0 = c.take<uint32_t>((size_t)num_tiles);
  b.seg_P = c.take<float>((size_t)b.seg_max_units * 256);
  b.seg_slab = c.take<float>((size_t)b.seg_max_units * 256 * 10);
  const bool reuse = sg > 0 && sg <= 65535;    // 16-bit offsets
  b.seg_rel = c.take<uint16_t>(reuse ? (size_t)b.seg_max_units * 4 * sg : 1);
  b.seg_nrel = c.take<uint32_t>((size_t)b.seg_max_units * 4);
  b.temp_bytes = sort_temp_bytes((int64_t)n);
  b.temp = c.take<char>(b.temp_bytes);
  b.total = c.total();
  return b;
}

ImageState carve_image(void* blob, int W, int H) {
  Carver c(blob);
  ImageState im;
  im.final_T = c.take<float>((size_t)W * H);
  im.n_contrib = c.take<uint32_t>((size_t)W * H);
  im.total = c.total();
  return im;
}

BwdState carve_bwd(void* blob, int P, int64_t I) {
  Carver c(blob);
  BwdState b;
  // gradient rows: one per live (instance, 8x8 quadrant) pair in the Gaussian-per-lane kernel, i.e. at most 4 I
  const size_t ni = (size_t)(I > 0 ? I : 1), n = 4 * ni, np = (size_t)(P > 0 ? P : 1);
  b.np_max = n / CH + np + 1;
  b.cidx = c.take<uint32_t>(ni + 2);
  b.pair_off = c.take<uint32_t>(np + 1);
  b.pair_owner = c.take<uint32_t>(b.np_max);
  b.partials = c.take<float>(b.np_max * GRAD_ROW);
  b.tau_partials = c.take<float>(ceil_div<size_t>(std::max(np, b.np_max), 256) * 6);   // per workgroup of the chain: over P or over the pairs
  b.temp_bytes = std::max(raster_scan_bytes((int64_t)ni + 1), raster_scan_bytes((int64_t)np + 1));
  b.temp = c.take<char>(b.temp_bytes);
  b.rows = c.take<float>(n * GRAD_ROW);
  b.total = c.total();
  return b;
}

// ---------------------------------------------------------------- environment knobs and the launch plan
// The product sets none of these: the defaults ARE the product; tests and A/B tools force the other branches.
//   knob                    values (default first)    set by        meaning
//   PINGS_BLEND_PPL         0 | 4 | other             tests         forward blend kernel: 0 = by blend_plan; 4 = wave per tile (four pixels
//                                                                   per lane); other (-1) = wave per quadrant
//   PINGS_BLEND_BWD         unset | pixel | other     tests         blend backward: unset = by footprint class; "pixel" = pixel-per-lane
//                                                                   (wave per tile); anything else = scan
//   PINGS_BLEND_SEG         512 | n | 0               tests         entries per segment of the segmented forward of long tile lists, 0 = off;
//                                                                   also sizes the segment tables of the binning blob (carve_binning)
//   PINGS_BLEND_SEG_REUSE   1 | 0                     tests         0: pass B re-tests every entry instead of walking pass T's compacted lists
//   PINGS_BWD_LONG          3072 | n | <= 0           tests, A/B    contributor count from which the scan backward splits a tile over four
//                                                                   waves per quadrant, rounded up to 16; <= 0 = never
//   PINGS_RASTER_OCCLUSION  1 | 0                     tests         0 keeps every (Gaussian, tile) instance (list-parity tests)
//   PINGS_DEPTH_SORT        bucket | l(ibrary)        tests         first letter l: rocPRIM radix sort instead of the bucket sort
//   PINGS_TILE_SORT         radix | l(ibrary)         tests, A/B    first letter l: rocPRIM radix sort instead of the two-pass sort of
//                                                                   tile_sort.hip (more than 65,536 tiles: always the library)
//   PINGS_RASTER_SCAN       own | l(ibrary)           tests, A/B    first letter l: hipcub::DeviceScan instead of the two-launch scans of
//                                                                   raster_scan.hip (more than 16,777,216 elements: always the library)
//   PINGS_OCC_AMIN          0.15 | x                  A/B           alpha below which a tile stays out of the occlusion budget, in [1/255, 0.99]
//   PINGS_OCC_WALK          dense | l(anes)           tests, A/B    first letter l: occl_budget_kernel deals one rank to a lane (walk_rects)
//                                                                   instead of the workgroup's pairs densely to its threads; same table
//   PINGS_RASTER_RECT       tight | 3(sigma) | e(llipse)  bench, tests  tile-rectangle rule of preprocess_kernel, by first letter
//   PINGS_MARK_VISIBLE      frustum | d(epth)         tests         first letter d: mark_visible tests depth only, the variant in which
//                                                                   upstream's frustum test stays commented out (assumption 2)
//   PINGS_ROWSUM_WGS        2048 | n                  tests         workgroups of row_chunk_sum_kernel, which stride over the (Gaussian,
//                                                                   chunk) pairs, 1 .. 65535 (1: one workgroup walks them all)
//   PINGS_GRAD_FILL         512 | n | l(aunch)        tests, A/B    zeros of the six gradient arrays behind the pixel-per-lane backward: n
//                                                                   workgroups behind the tiles of its launch, 1 .. 65535; first letter l:
//                                                                   grad_zero_kernel, a launch of its own (always when there is no instance)
//   PINGS_CHAIN_SUM         group | l(anes)           tests, A/B    first letter l: gaussian_bwd_rank_kernel sums an owner's chunk partials
//                                                                   in the owner's lane instead of by 16-lane groups; same bits
//   PINGS_BLEND_INTERIOR    1 | 0                     tests, A/B    the lean trip of blend_bwd_tile_kernel for surfel records interior to
//                                                                   their tile (blend_interior); 0 = every record through the general trip;
//                                                                   same bits
//   PINGS_BIN               auto | s(ort) | g(ather)  tests, A/B    how pings_raster_render builds the tile lists: s = always duplicate and
//                                                                   sort; g = gather from the front ranks (raster_gather.hip) whenever its
//                                                                   tables fit (gather_fits), else sort; auto = gather only a class-2 frame
//                                                                   with front * tiles <= GATHER_COST * instances; same bits
RasterKnobs read_knobs() {
  RasterKnobs k;   // the defaults: raster_common.hpp
  if (const char* e = getenv("PINGS_BLEND_PPL")) k.blend_ppl = atoi(e);
  if (const char* e = getenv("PINGS_BLEND_BWD")) k.blend_bwd = strcmp(e, "pixel") != 0 ? RasterKnobs::BWD_SCAN : RasterKnobs::BWD_PIXEL;
  if (const char* e = getenv("PINGS_BLEND_SEG")) k.blend_seg = (uint32_t)atoi(e);
  if (const char* e = getenv("PINGS_BLEND_SEG_REUSE")) k.seg_reuse = atoi(e) != 0;
  // blend_bwd_scan_kernel: tiles whose largest per-pixel contributor count reaches the threshold get four waves per
  // quadrant (0 = never); at most LONG_TILES_MAX tiles per frame, taken as whole bins of tile_order_kernel (work / 16,
  // clamped to 1023) from the top down, so that the set of split tiles depends on the per-tile work alone — when the
  // bins at or above the threshold hold more than the cap, the lowest of them stay unsplit, and a threshold above
  // 16,368 splits nothing.  C3 street sweep (r03, kernel ms): never 0.72, 256 0.65, 768 0.59, 2048 0.535, 3072 0.53,
  // 4096 0.52, 8192 0.57 — the split costs four queue walks and two barriers per chunk, so only the lists that set
  // the kernel's duration should pay it.
  if (const char* e = getenv("PINGS_BWD_LONG")) {
    const long v = atol(e);
    k.bwd_long = v <= 0 ? 0xFFFFFFF0u : (uint32_t)((v + 15) / 16 * 16);
  }
  if (const char* e = getenv("PINGS_RASTER_OCCLUSION")) k.occlusion = atoi(e) != 0;
  if (const char* e = getenv("PINGS_DEPTH_SORT")) k.library_sort = e[0] == 'l';
  if (const char* e = getenv("PINGS_TILE_SORT")) k.library_tile_sort = e[0] == 'l';
  if (const char* e = getenv("PINGS_RASTER_SCAN")) k.library_scan = e[0] == 'l';
  // Tiles a Gaussian covers with less than this alpha everywhere are left out of the occlusion budget: fewer entries
  // is still a lower bound of the opacity in front (conservative: the kept lists can only grow, results unchanged),
  // and the faint rim of every footprint was most of the budget pass's atomics.  Metric-1 sweep (r03): 1/255 -> 0.15
  // takes occl_budget 0.116 -> 0.053 ms and the step 1.136 -> 1.072 ms for 7.8 % more instances (0.2: 17 % more for
  // 0.005 ms); C2 / C3 unchanged.  1/255 = every covered tile, the round-2 behaviour.
  if (const char* e = getenv("PINGS_OCC_AMIN")) k.occ_amin = fminf(fmaxf((float)atof(e), 1.0f / 255.0f), 0.99f);
  if (const char* e = getenv("PINGS_OCC_WALK")) k.occ_walk_lanes = e[0] == 'l';
  if (const char* e = getenv("PINGS_RASTER_RECT")) k.rect_rule = e[0] == '3' ? RECT_3SIGMA : e[0] == 'e' ? RECT_ELLIPSE : RECT_TIGHT;
  if (const char* e = getenv("PINGS_MARK_VISIBLE")) k.mark_depth_only = e[0] == 'd';
  if (const char* e = getenv("PINGS_ROWSUM_WGS")) k.rowsum_wgs = (unsigned)std::min(std::max(atoi(e), 1), 65535);
  if (const char* e = getenv("PINGS_GRAD_FILL")) k.grad_fill_wgs = e[0] == 'l' ? 0u : (unsigned)std::min(std::max(atoi(e), 1), 65535);
  if (const char* e = getenv("PINGS_CHAIN_SUM")) k.chain_sum_lanes = e[0] == 'l';
  if (const char* e = getenv("PINGS_BLEND_INTERIOR")) k.blend_interior = atoi(e) != 0;
  if (const char* e = getenv("PINGS_BIN")) k.bin = e[0] == 's' ? RasterKnobs::BIN_SORT : e[0] == 'g' ? RasterKnobs::BIN_GATHER : RasterKnobs::BIN_AUTO;
  return k;
}

BlendPlan blend_plan(const RasterKnobs& k, int footprint_class, int64_t I, int num_tiles) {
  BlendPlan p;
  // Blend backward kernel: Gaussian-per-lane wave scans when footprints are small (lanes of the pixel-per-lane kernel
  // would idle: 2.25x faster on a street-like surfel scene), pixel-per-lane when they are large (chunks of the scan
  // kernel would stay half empty and every instance would need four rows: 25 % faster on the Metric-1 cloud).
  // `footprint_class` comes from pings_raster_preprocess.
  p.bwd_scan = k.blend_bwd == RasterKnobs::BWD_AUTO ? footprint_class != 2 : k.blend_bwd == RasterKnobs::BWD_SCAN;
  // the scan backward reads the exact per-quadrant masks, so the forward of the same view has to write them: only
  // the wave-per-quadrant forward does
  p.want_qmask = p.bwd_scan;
  // The pixel-per-lane backward is one wave per tile with four pixels per lane (0.40 -> 0.35 ms on Metric-1 against
  // the removed two-waves-per-tile kernel with two).
  // The wave-per-quadrant kernel is the forward of footprint class 1 (against the removed workgroup-per-tile kernels:
  // Metric-1 0.244 vs 0.265 ms with two pixels per lane; street-like scene 0.86 vs 1.31 ms with one).  Footprint
  // class 2 with the pixel-per-lane backward to follow (no quadrant masks needed): wave per TILE, four pixels per
  // lane (Metric-1: 0.245 -> see DESIGN).
  const bool tile_wave = k.blend_ppl == 4 || (k.blend_ppl == 0 && footprint_class == 2 && !p.want_qmask);
  p.fwd = tile_wave ? BlendPlan::FWD_TILE : BlendPlan::FWD_WAVE;
  // long lists in parallel segments (see blend_fwd_seg_kernel); pass B walks pass T's compacted lists (16-bit offsets)
  p.seg = k.blend_seg;
  p.seg_on = p.seg > 0 && I > (int64_t)num_tiles * (p.seg / 4) && I > 2 * (int64_t)p.seg;
  p.seg_reuse = p.seg <= 65535u && k.seg_reuse;
  p.long_thr = k.bwd_long;
  p.interior_bwd = k.blend_interior;
  return p;
}

}  // namespace raster
}  // namespace pings

using namespace pings::raster;

PINGS_API size_t pings_raster_geom_bytes(int P, int image_height, int image_width) {
  const int nt = pings::ceil_div(image_width, TILE) * pings::ceil_div(image_height, TILE);
  return carve_geom(nullptr, P, nt).total;
}

PINGS_API size_t pings_raster_binning_bytes(int64_t num_instances, int image_height,
                                            int image_width) {
  const int nt = pings::ceil_div(image_width, TILE) * pings::ceil_div(image_height, TILE);
  return carve_binning(nullptr, num_instances, nt, read_knobs().blend_seg).total;
}

PINGS_API size_t pings_raster_backward_bytes(int P, int64_t num_instances) {
  return carve_bwd(nullptr, P, num_instances).total;
}

PINGS_API size_t pings_raster_image_bytes(int image_height, int image_width) {
  return carve_image(nullptr, image_width, image_height).total;
}

__global__ void slots_to_ids_kernel(int64_t I, const uint32_t* __restrict__ list, const uint32_t* __restrict__ gval,
                                    uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < I) out[i] = gval[list[i]];
}


PINGS_API int pings_raster_debug_lists(const void* binning_blob, int64_t I, int image_height,
                                       int image_width, uint32_t* point_list, uint32_t* ranges_xy,
                                       void* stream) {
  PINGS_ARG_CHECK(binning_blob && ranges_xy, "null pointer");
  const int nt = pings::ceil_div(image_width, TILE) * pings::ceil_div(image_height, TILE);
  BinState bs = carve_binning(const_cast<void*>(binning_blob), I, nt, read_knobs().blend_seg);
  hipStream_t st = pings::as_stream(stream);
  if (I > 0 && point_list) {  // sorted list holds instance slots; the tap returns Gaussian ids
    hipLaunchKernelGGL(slots_to_ids_kernel, dim3((unsigned)pings::ceil_div<int64_t>(I, 256)), dim3(256), 0, st, I,
                       bs.point_list, bs.gval, point_list);
    PINGS_LAUNCH_CHECK();
  }
  PINGS_HIP_CHECK(hipMemcpyAsync(ranges_xy, bs.ranges, sizeof(uint2) * (size_t)nt,
                                 hipMemcpyDeviceToDevice, st));
  return PINGS_OK;
}

PINGS_API int pings_raster_debug_occlusion(const void* geom_blob, int P, int image_height, int image_width,
                                           uint32_t* occ_bucket, uint16_t* occ_bsat, int32_t* occ_nb, void* stream) {
  PINGS_ARG_CHECK(occ_nb, "null pointer");
  const int nt = pings::ceil_div(image_width, TILE) * pings::ceil_div(image_height, TILE);
  *occ_nb = occlusion_buckets(nt);
  if (!occ_bucket && !occ_bsat) return PINGS_OK;   // the table's height alone: what the caller sizes its copies by
  PINGS_ARG_CHECK(geom_blob && occ_bucket && occ_bsat, "null pointer");
  GeomState gs = carve_geom(const_cast<void*>(geom_blob), P, nt);
  hipStream_t st = pings::as_stream(stream);
  PINGS_HIP_CHECK(hipMemcpyAsync(occ_bucket, gs.occ_bucket, sizeof(uint32_t) * (size_t)nt * (size_t)gs.occ_nb,
                                 hipMemcpyDeviceToDevice, st));
  PINGS_HIP_CHECK(hipMemcpyAsync(occ_bsat, gs.occ_bsat, sizeof(uint16_t) * (size_t)nt, hipMemcpyDeviceToDevice, st));
  return PINGS_OK;
}

PINGS_API int pings_raster_debug_image(const void* image_blob, int image_height, int image_width,
                                       float* final_T, uint32_t* n_contrib, void* stream) {
  PINGS_ARG_CHECK(image_blob && final_T && n_contrib, "null pointer");
  ImageState im = carve_image(const_cast<void*>(image_blob), image_width, image_height);
  hipStream_t st = pings::as_stream(stream);
  const size_t n = (size_t)image_height * image_width;
  PINGS_HIP_CHECK(hipMemcpyAsync(final_T, im.final_T, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
  PINGS_HIP_CHECK(hipMemcpyAsync(n_contrib, im.n_contrib, sizeof(uint32_t) * n,
                                 hipMemcpyDeviceToDevice, st));
  return PINGS_OK;
}
