// Shared definitions of the Gaussian(-surfel) rasteriser kernels.
//
// HBM layout (all buffers caller-owned, carved out of three opaque blobs):
//   geom blob   (per Gaussian)  rec[P][4] float4  : {mx,my,opacity,pz} {conic_x,conic_y,conic_z,rz}
//                                                    {r,g,b,q} {nx,ny,nz,-}
//                               rect[P]   uint4   : {inst_base, xmin|ymin<<16, xmax|ymax<<16, tiles}
//                               depth keys / ids (+ sorted copies), tiles-in-depth-order, their scan,
//                               radix-sort / scan scratch
//   binning blob (per instance) sorted Gaussian ids, ranges[num_tiles] uint2, per-instance blend-weight sums,
//                               tile keys / ids before sorting, scratch
//   image blob   (per pixel)    final_T[HW] float, n_contrib[HW] uint32
//
// Instances (Gaussian x touched tile) are created in DEPTH order (the P Gaussians are
// radix-sorted by their fp32 view depth first) and then stably radix-sorted by tile id
// only, so the final order inside a tile is (depth, Gaussian index) — the same order a
// 64-bit (tile<<32 | depth) key sort gives, at a quarter of the sort traffic.
#pragma once
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"

namespace pings {
namespace raster {

constexpr int TILE = 16;
constexpr int BLOCK = TILE * TILE;  // 256 threads = 4 waves; wave w owns rows 4w..4w+3
constexpr float NEAR_Z = 0.2f;
constexpr float LOWPASS = 0.3f;
constexpr float ALPHA_MAX = 0.99f;
constexpr float ALPHA_MIN = 1.0f / 255.0f;
constexpr float T_EPS = 1e-4f;
constexpr float DEPTH_ALPHA_EPS = 1e-10f;
constexpr float DEN_EPS = 1e-6f;
constexpr uint32_t CULLED_KEY = 0xFFFFFFFFu;
constexpr int DS_NB = 1 << 20;        // depth-sort buckets (2^18 left ~1.5k surfels per bucket on a rough fronto-parallel wall at 60 m: 0.43 ms of ranking)
constexpr uint32_t DS_LIMIT = 4096u;  // bucket population beyond which the library sort takes over
constexpr int DS_SHARDS = 64;  // single-address atomics serialise at ~12 ns each on this part: spread them
// header words: [0, 64) max key shards, [64, 128) max ~key shards, 128 kmin, 129 shift, 130 overflow flag
constexpr int DS_KMIN = 2 * DS_SHARDS, DS_SHIFT = DS_KMIN + 1, DS_FLAG = DS_KMIN + 2, DS_HEAD = DS_KMIN + 8;
// The frame statistics (GeomState::stats), STAT_SHARDS words each so that thousands of waves do not add to one word:
// [STAT_PAIRS + shard] (Gaussian, tile) pairs before occlusion culling and [STAT_VISIBLE + shard] Gaussians with a
// tile, both from preprocess_kernel; [STAT_KEPT + shard] kept pairs from count_kept_kernel; word STAT_WORDS - 1 holds
// occ_bmax in its low half and occ_front (the front depth F of the frame) in its high half.  The kept words come last,
// next to that word: a retry of the depth sort clears those (STAT_RETRY_WORDS from STAT_KEPT on) and keeps what the
// preprocess pass, which does not run again, left in the others.
constexpr int STAT_SHARDS = 256;
constexpr int STAT_PAIRS = 0, STAT_VISIBLE = STAT_SHARDS, STAT_KEPT = 2 * STAT_SHARDS;
constexpr int STAT_BMAX = 3 * STAT_SHARDS, STAT_WORDS = STAT_BMAX + 1, STAT_RETRY_WORDS = STAT_WORDS - STAT_KEPT;
static_assert((STAT_SHARDS & (STAT_SHARDS - 1)) == 0, "the shard of a wave is its number modulo a power of two");
// occlusion culling of instances (see occl_budget_kernel)
constexpr float OCC_THR = 9.5f;     // > -ln(T_EPS) = 9.21: transmittance bound that guarantees every pixel has stopped
constexpr float OCC_FIX = 4096.f;   // fixed-point scale of the budget (integer atomics: order independent)
constexpr uint16_t OCC_ALL = 0xFFFFu;

constexpr int MODE_SURFEL = 0;
constexpr int MODE_3DGS = 1;
// tile-rectangle rule of preprocess_kernel (raster_fwd.hip)
constexpr int RECT_TIGHT = 0, RECT_3SIGMA = 1, RECT_ELLIPSE = 2;

// 16 floats of per-instance gradient accumulated by the blend backward pass
// (one 64-B row per (tile, Gaussian) instance, summed per Gaussian afterwards).
// G_CONX/Y/Z hold dL/d(cov2D xx, xy, yy) — NOT the gradient w.r.t. the conic (see blend_bwd_tile_kernel).
constexpr int GRAD_ROW = 16;
constexpr int CH = 64;  // rows per first-level chunk of the per-Gaussian sum
enum GradSlot {
  G_MX = 0, G_MY = 1, G_CONX = 2, G_CONY = 3, G_CONZ = 4, G_OPAC = 5,
  G_R = 6, G_G = 7, G_B = 8, G_NX = 9, G_NY = 10, G_NZ = 11, G_Q = 12, G_PZ = 13,
  G_ZLO = 14, G_ZHI = 15
};

struct FrameSummary {   // the record of a frame's one host read-back (frame_summary_kernel)
  uint32_t overflow, front;      // depth-sort overflow flag; front depth F = 1 + the last depth rank that keeps a tile
                                 // (FRONT_UNKNOWN where the frame cannot gather and nobody looked for it)
  unsigned long long stats[3];   // pairs before occlusion culling, visible Gaussians, kept pairs (= instances)
  int32_t aux[8];
  uint32_t seq;   // written last (system-scope release): the host polls it instead of blocking in the runtime
  uint32_t pad;
};

struct GeomState {
  float4* rec;
  uint4* rect;
  uint32_t *depth_key, *depth_key_sorted, *gidx, *gidx_sorted;
  uint32_t* rank_of;                        // [P] depth rank of each surviving Gaussian (inverse of gidx_sorted)
  uint32_t *tiles_sorted, *offsets_sorted;  // per depth rank: KEPT tiles of the Gaussian and their inclusive scan
  uint32_t* occ_bucket;                     // [occ_nb][num_tiles] fixed-point opacity budget per (rank bucket, tile)
  uint16_t* occ_bsat;                       // [num_tiles] last rank bucket a tile still needs (0xFFFF = all)
  unsigned long long* occ_mask;             // [occ_nb][occ_words] bit (tile % 64) of word tile / 64: bucket <= occ_bsat[tile]
  uint32_t* nvalid;                         // [1] Gaussians that survived culling (= ranks with a real depth key)
  uint32_t* occ_bmax;                       // [1] largest occ_bsat over the tiles, occ_nb - 1 if one never saturates;
                                            //     behind `stats`, cleared with them
  uint32_t* occ_front;                      // [1] front depth F: 1 + the largest depth rank that keeps a tile, 0 if none
                                            //     does (count_kept_kernel); the other half of occ_bmax's 8-byte word
  uint32_t* ds_head;                        // depth sort: header (key range shards, range, overflow flag), then
  uint32_t *ds_cnt, *ds_fill, *ds_off;      //   [DS_NB + blocks] bucket / per-block culled counts, [DS_NB] fill cursors,
  char* zero_begin; size_t zero_bytes;      // occ_bucket .. stats .. ds_head: the frame's one memset
  size_t ds_words;                          //   [DS_NB + blocks + 1] their exclusive scan; ds_words = memset extent
  uint32_t* ds_idx;                         //   [P] Gaussian ids in bucket order (keys go to depth_key_sorted)
  unsigned long long* stats;                // [3][shards] pairs before occlusion culling, Gaussians with a tile (both from
                                            //     preprocess_kernel), kept pairs (count_kept_kernel); then occ_bmax
  FrameSummary* summary;
  int occ_nb, occ_words;                    // rank buckets per tile; 64-bit words per bucket of occ_mask
  char* temp;
  size_t temp_bytes;
  size_t total;
};

struct BinState {
  // pre-sort, slot order (= depth rank, then tile order inside the Gaussian's rectangle): tile_key[slot],
  // gval[slot] = Gaussian id;  sorted by tile: point_list[i] = slot (the sort's values are the element indices, no iota array)
  uint32_t *tile_key, *tile_key_sorted, *gval, *point_list;
  uint32_t* slot_val;  // [I] the tile sort's values between its two passes (tile_sort.hip)
  uint2* ranges;
  float* inst_w;       // [I+1] per-instance sum of blend weights (0 = instance never blended)
  uint8_t* inst_qmask; // [I+1] 8x8 quadrants of the tile in which the instance blended something (bit q = qx + 2 qy)
  float* inst_wq;      // [I][4] per-(instance, quadrant) sums of the wave-per-quadrant forward kernel, folded into
  uint32_t* inst_cntq; //        inst_w / inst_cnt / inst_qmask by combine_quadrants_kernel
  uint32_t* inst_cnt;  // [I]   per-instance pixel count with transmittance > 0.5 (3DGS)
  uint32_t* tile_order;  // [2][num_tiles] tiles by descending work: [0] by list length (forward), [1] by the largest
                         // per-pixel contributor count (backward) — longest-processing-time-first dispatch order
  uint32_t* tile_work;   // [num_tiles] work of the backward ordering: a tile's largest per-pixel contributor count,
  uint32_t* tile_maxc;   //             from tile_max_contrib_kernel | left by blend_fwd_tile_kernel (BlendPlan::FWD_TILE)
  // segmented blend of long tile lists (raster_blend_fwd.hip, "forward of LONG tile lists")
  uint32_t seg_max_units;      // capacity: every list of more than 2 * SEG entries cut into SEG-entry units
  uint32_t *seg_head, *seg_unit_tile, *seg_unit_seg, *seg_tile_unit0;
  float *seg_P, *seg_slab;
  uint16_t* seg_rel;           // [units][4][SEG] pass T's compacted list: offsets (in the segment) of the entries that can
  uint32_t* seg_nrel;          // [units][4]      reach the quadrant, and how many — pass B walks these instead of re-testing
  char* temp;
  size_t temp_bytes;
  size_t total;
};

struct ImageState {
  float* final_T;
  uint32_t* n_contrib;
  size_t total;
};

// Camera and image parameters of a frame, passed BY VALUE to the kernels: field order and layout are part of every
// kernel's argument block.  BParams (backward kernels) is KParams (forward kernels) without the binning-only fields;
// fill_camera fills what they share.
struct KParams {
  int P, W, H, gx, gy;
  int front_only;
  float occ_amin;    // smallest per-tile alpha bound that is worth an occlusion-budget entry (see preprocess_kernel)
  int rect_rule;     // RECT_TIGHT (default) | RECT_3SIGMA | RECT_ELLIPSE, see preprocess_kernel (PINGS_RASTER_RECT)
  float fx, fy, limx, limy, scale_mod;
  const float* view;
  const float* proj_raw;
  const float* bg;
  const float* prcp;
  const int32_t* live;   // device word: of the first `dyn_rows` Gaussians only rows [0, *live) exist (nullable)
  int dyn_rows;
};

struct BParams {
  int P, W, H, gx, gy;
  int front_only;
  float fx, fy, limx, limy, scale_mod;
  const float* view;
  const float* proj_raw;
  const float* bg;
  const float* prcp;
};

// Checks the settings and fills the fields KParams and BParams have in common.
template <typename Params>
int fill_camera(const pings_raster_settings* s, int P, Params& kp) {
  PINGS_ARG_CHECK(s != nullptr, "null settings");
  PINGS_ARG_CHECK(s->image_height > 0 && s->image_width > 0, "empty image");
  PINGS_ARG_CHECK(s->image_height < 65536 * TILE / 16 && s->image_width < 65536, "image too large");
  PINGS_ARG_CHECK(s->mode == PINGS_RASTER_SURFEL || s->mode == PINGS_RASTER_3DGS, "unknown mode");
  PINGS_ARG_CHECK(s->viewmatrix && s->projmatrix_raw && s->bg, "null camera pointer");
  PINGS_ARG_CHECK(s->tanfovx > 0 && s->tanfovy > 0, "non-positive tanfov");
  kp.P = P;
  kp.W = s->image_width;
  kp.H = s->image_height;
  kp.gx = ceil_div(kp.W, TILE);
  kp.gy = ceil_div(kp.H, TILE);
  kp.front_only = s->front_only;
  kp.fx = (float)((double)kp.W / (2.0 * s->tanfovx));
  kp.fy = (float)((double)kp.H / (2.0 * s->tanfovy));
  kp.limx = (float)(1.3 * s->tanfovx);
  kp.limy = (float)(1.3 * s->tanfovy);
  kp.scale_mod = (float)s->scale_modifier;
  kp.view = s->viewmatrix;
  kp.proj_raw = s->projmatrix_raw;
  kp.bg = s->bg;
  kp.prcp = s->prcppoint;
  return PINGS_OK;
}

// f(std::integral_constant<int, MODE_...>{}) for the settings' mode: the one place a run-time mode becomes a kernel
// template argument (`[&](auto m) { ... kernel<m()> ... }`).
template <typename F>
decltype(auto) with_mode(int mode, F&& f) {
  if (mode == PINGS_RASTER_SURFEL) return f(std::integral_constant<int, MODE_SURFEL>{});
  return f(std::integral_constant<int, MODE_3DGS>{});
}

// Every PINGS_* environment knob of the rasteriser, parsed (raster_layout.hip: the table above read_knobs documents
// each, defaults included).  Read on every call, never cached: tests switch knobs between calls of one process.
struct RasterKnobs {
  enum Bwd { BWD_AUTO, BWD_PIXEL, BWD_SCAN };
  int blend_ppl = 0;             // PINGS_BLEND_PPL
  Bwd blend_bwd = BWD_AUTO;      // PINGS_BLEND_BWD
  uint32_t blend_seg = 512u;     // PINGS_BLEND_SEG
  bool seg_reuse = true;         // PINGS_BLEND_SEG_REUSE
  uint32_t bwd_long = 3072u;     // PINGS_BWD_LONG: the threshold itself (never = 0xFFFFFFF0)
  bool occlusion = true;         // PINGS_RASTER_OCCLUSION
  bool library_sort = false;     // PINGS_DEPTH_SORT
  bool library_tile_sort = false;  // PINGS_TILE_SORT
  bool library_scan = false;     // PINGS_RASTER_SCAN
  float occ_amin = 0.15f;        // PINGS_OCC_AMIN
  bool occ_walk_lanes = false;   // PINGS_OCC_WALK
  int rect_rule = RECT_TIGHT;    // PINGS_RASTER_RECT
  bool mark_depth_only = false;  // PINGS_MARK_VISIBLE
  unsigned rowsum_wgs = 2048u;   // PINGS_ROWSUM_WGS
  unsigned grad_fill_wgs = 512u; // PINGS_GRAD_FILL: fill workgroups behind the blend backward's tiles (0 = own launch)
  bool chain_sum_lanes = false;  // PINGS_CHAIN_SUM
  bool blend_interior = true;    // PINGS_BLEND_INTERIOR
  enum Bin { BIN_AUTO, BIN_SORT, BIN_GATHER };
  Bin bin = BIN_AUTO;            // PINGS_BIN
};
RasterKnobs read_knobs();

// Which blend kernels a view runs.  pings_raster_render and pings_raster_backward both derive it from the same
// arguments and branch on nothing else: the forward writes the exact quadrant masks iff the backward will scan them.
struct BlendPlan {
  enum Fwd { FWD_TILE, FWD_WAVE } fwd;  // wave per tile, wave per quadrant
  bool want_qmask;     // forward writes exact quadrant masks
  bool bwd_scan;       // Gaussian-per-lane backward; else pixel-per-lane (wave per tile)
  uint32_t seg;        // entries per segment of the segmented forward of long tile lists
  bool seg_on, seg_reuse;
  uint32_t long_thr;   // four-wave split threshold of the scan backward
  bool interior_bwd;   // the wave-per-tile backward classifies its records (blend_interior) and runs the lean trip
};
BlendPlan blend_plan(const RasterKnobs& k, int footprint_class, int64_t I, int num_tiles);

struct BwdState {
  uint32_t* cidx;        // [I+2] exclusive scan of live flags over instance slots (cidx[I] = #live)
  float* rows;           // [I][16] gradient rows of live instances (upper bound; only #live used)
  uint32_t *pair_off, *pair_owner;   // [P+1] exclusive scan of the Gaussians' chunk counts (by depth rank), [NPmax] owner rank of a chunk
  float* partials;       // [NPmax][16]
  float* tau_partials;   // [ceil(NPmax/256)][6] one row per workgroup of the per-Gaussian chain
  char* temp;
  size_t temp_bytes, np_max, total;
};

GeomState carve_geom(void* blob, int P, int num_tiles);
// tile_order[i] = i-th tile in descending `work` (ties in any order: scheduling only, results do not depend on it)
// n_long (optional): receives min(number of tiles with work >= long_thr, long_max) — they lead the order
int launch_tile_order(const uint32_t* work, int num_tiles, uint32_t* order, hipStream_t st, uint32_t* n_long = nullptr,
                      uint32_t long_thr = 0, uint32_t long_max = 0);
int occlusion_buckets(int num_tiles);
// `seg` = RasterKnobs::blend_seg of the call: the capacity of the segment tables depends on it
BinState carve_binning(void* blob, int64_t I, int num_tiles, uint32_t seg);
ImageState carve_image(void* blob, int W, int H);
BwdState carve_bwd(void* blob, int P, int64_t I);

// tile_sort.hip: stable sort of (key, element index) by the low `bits` <= 16 bits of the key, KeyT = uint16_t | uint32_t.
// One pass (bits <= 8) goes from keys_in straight to keys_out / vals_out; two passes go through keys_tmp / vals_tmp,
// and keys_out may then be keys_in.  `table`: tile_sort_table_bytes(n) bytes.  Workgroups of TS_THREADS own TS_BLOCK pairs.
constexpr int TS_THREADS = 256, TS_BLOCK = 4096;
size_t tile_sort_table_bytes(int64_t n);
template <typename KeyT>
int tile_sort(const KeyT* keys_in, int64_t n, int bits, KeyT* keys_tmp, uint32_t* vals_tmp, KeyT* keys_out,
              uint32_t* vals_out, uint32_t* table, hipStream_t st);
// rocprim::radix_sort_pairs of the same pairs, and the scratch it asks for (either key width)
size_t tile_sort_library_bytes(int64_t n);
template <typename KeyT>
int tile_sort_library(const KeyT* keys_in, int64_t n, int bits, KeyT* keys_out, uint32_t* vals_out, void* temp,
                      size_t temp_bytes, hipStream_t st);

// raster_gather.hip: the tile lists of a frame whose kept instances all lie in the first `front` depth ranks, gathered
// per tile from those ranks instead of sorted: writes gval, ranges, point_list and the forward tile order word for word
// as duplicate_kernel, the tile sort, tile_ranges_kernel and tile_order_kernel<true> do, and the zeros of per_gaussian.
// gather_fits: whether its tables fit into the arrays of the binning blob that only the sort path uses (front entries
// in slot_val, the row table in tile_key .. tile_key_sorted).  FRONT_MAX, the deepest front the plan takes: four
// staging chunks of tile_gather_kernel, 3.5 times the headline's 2,304; a front entry carries its rank in 24 bits, so
// the staging design would allow far more, but every workgroup of both passes reads the whole front (8 B a rank: 64 KB
// at FRONT_MAX, 33 MB out of L2 per pass at 1080p), and at 1080p a front of FRONT_MAX is a cost ratio of about 37,
// beyond GATHER_COST already: deeper fronts belong to the sort.
constexpr uint32_t FRONT_MAX = 8192u;
constexpr int GATHER_CHUNK = 2048;       // front entries a workgroup of tile_gather_kernel stages in LDS at a time
// The default plan gathers while front * tiles <= GATHER_COST * instances: half the ratio at which the two plans
// cost the same (profiles/r19/plan_sweep.json: the gather saves 30 - 33 us at ratios of 12 - 15, 23.5 us at 21.6 and
// 11.9 us at 35.5, the last frame below FRONT_MAX; the least-squares line through them meets zero at 49.5).
constexpr uint64_t GATHER_COST = 25u;
constexpr uint32_t FRONT_UNKNOWN = 0xFFFFFFFFu;   // frame_summary_kernel did not look for the front depth: no plan gathers
// nb: rank buckets per tile (a front entry holds the bucket in 8 bits)
inline bool gather_fits(uint32_t front, int gx, int gy, int nb, int64_t I) {
  return front >= 1u && front <= FRONT_MAX && gx <= 256 && gy <= 256 && nb <= 256 && (int64_t)front * gy <= 2 * I &&
         2 * (int64_t)front <= I;
}
int launch_tile_gather(const KParams& kp, int P, int64_t I, uint32_t front, const GeomState& gs, const BinState& bs,
                       void* per_gaussian, hipStream_t st);

// raster_blend_fwd.hip: the blend half of pings_raster_render — the forward kernels of `plan`, then the per-Gaussian sums
int launch_blend_fwd(int mode, const KParams& kp, const BlendPlan& plan, int P, int64_t I, const GeomState& gs,
                     const BinState& bs, const ImageState& im, float* out_color, float* out_normal, float* out_depth,
                     float* out_alpha, void* per_gaussian, hipStream_t st);

// value of `v` in lane `src`, `src` wave-uniform: v_readlane_b32 (scalar path) instead of the ds_bpermute_b32 a
// general __shfl compiles to — no LDS round trip, no lgkmcnt wait in the per-rectangle loops below
__device__ inline int lane_value(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ inline uint32_t lane_value(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ inline float lane_value(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

// Depth ranks -> lanes.  The nearest Gaussians cover the most tiles and sit at neighbouring ranks: dealt out in rank
// order they would all land in the first waves.  The first quarter of the ranks is therefore dealt round-robin,
// one rank per wave at a time (lane l < 16 of wave w: rank l num_waves + w); behind it the footprints are small and
// even, and ranks go out in runs of 16 (quarter q >= 1 of wave w: ranks 16 (q num_waves + w) .. + 15), so that the
// per-rank loads and stores are 64-byte segments instead of one memory transaction per lane.  (Runs of 16 from rank
// 0 on: Metric-1's duplicate pass 0.054 -> 0.168 ms — sixteen screen-filling footprints in one wave; C3 0.078 ->
// 0.037 ms either way.)
// `dealt_rank` deals the ranks [0, 64 num_waves) to the lanes of `num_waves` waves; strided_rank is the deal over a
// grid that covers P.
__device__ inline int dealt_rank(int num_waves, int wave, int lane) {
  return lane < 16 ? lane * num_waves + wave : ((lane >> 4) * num_waves + wave) * 16 + (lane & 15);
}
__device__ inline int strided_rank(int P) {
  const int num_waves = (int)(gridDim.x * (blockDim.x >> 6));
  const int wave = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const int r = dealt_rank(num_waves, wave, (int)(threadIdx.x & 63));
  return r < P ? r : -1;
}

// ---------------------------------------------------------------- rank buckets of the occlusion bound
// The occlusion budget is kept per (tile, rank bucket), and a tile keeps every rank up to the END of the bucket in
// which its budget saturates: the width of that bucket is what it keeps for nothing.  Where tiles saturate at all they
// do so within the first few hundred to few thousand depth ranks, whatever the number of survivors, so the buckets are
// fine at the front and pay for it with wider ones behind — a log-linear map in integer arithmetic:
//   * FRONT: ranks in units of w0 = 2^RB_LW; the first s = 2^RB_LS buckets hold one unit each, then every octave of
//     the unit number q = r / w0 is cut into s buckets: q in [s 2^k, s 2^(k+1)) has buckets of w0 2^k ranks.  A bucket
//     that starts at rank r is at most max(w0, r / s) ranks wide.  Section 0 is the s unit buckets, section j >= 1 the
//     octave k = j - 1; the front is the first J sections, ranks [0, w0 s 2^(J-1)), buckets [0, s J);
//   * J: as many sections as keep the bucket width at or below today's equal share eq = ceil(nvalid / nb) — a front
//     bucket is never wider than an equal one was — and at most nb / 2 buckets;
//   * BEHIND: the remaining ranks dealt equally to the remaining buckets, at least nb / 2 of them: no bucket is wider
//     than 2 eq, so a tile that saturates deep in the order keeps at most one equal share more than it did.
// Any monotone partition of the ranks is a valid bucket map (the bound only needs buckets in depth order); this one
// is a function of (r, nb, nvalid) alone, so the three kernels that call it agree without a table.  A rank from
// nvalid on (a culled Gaussian: no tiles) gets the last bucket.  pings_raster_rank_bucket exports it to the host tests.
constexpr int RB_LW = 4, RB_LS = 4;
__host__ __device__ inline uint32_t rank_bucket_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }   // x > 0
__host__ __device__ inline uint32_t rank_bucket(int r, int nb, uint32_t nvalid) {
  if (r < 0 || nvalid == 0u) return 0u;
  const uint32_t ur = (uint32_t)r, unb = (uint32_t)nb;
  if (ur >= nvalid) return unb - 1u;
  const uint32_t eq = (nvalid - 1u) / unb + 1u;
  uint32_t J = 0u;
  if ((eq >> RB_LW) != 0u) {
    J = rank_bucket_log2(eq >> RB_LW) + 2u;
    if (J > (unb >> (RB_LS + 1))) J = unb >> (RB_LS + 1);
  }
  const uint32_t front_ranks = J ? 1u << (RB_LW + RB_LS + J - 1u) : 0u, front_buckets = J << RB_LS;
  if (ur < front_ranks) {
    const uint32_t q = ur >> RB_LW;
    if ((q >> RB_LS) == 0u) return q;
    const uint32_t k = rank_bucket_log2(q) - RB_LS;
    return (k << RB_LS) + (q >> k);     // ((k + 1) s) + (q >> k) - s
  }
  // here front_ranks <= r < nvalid: at least one rank and nb / 2 buckets are left
  const uint32_t b = front_buckets + (uint32_t)(((unsigned long long)(ur - front_ranks) * (unb - front_buckets)) /
                                                (unsigned long long)(nvalid - front_ranks));
  return b < unb ? b : unb - 1u;
}

// bit i = tile s + i of the bucket whose mask row is `m` is kept, 0 <= i < w, 1 <= w <= 64 (GeomState::occ_mask; the row
// walks of raster_fwd.hip and raster_gather.hip).  The second word may belong to the next bucket's row, or be the one
// spare word behind the table: only bits of tiles below s + w survive the cut.
__device__ inline unsigned long long kept_bits(const unsigned long long* __restrict__ m, int s, int w) {
  const int i = s >> 6, sh = s & 63;
  const unsigned long long lo = m[i], hi = m[i + 1];
  const unsigned long long v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
  return v & (~0ull >> (64 - w));
}

// Two fp32 values in one VGPR pair: + - * on f2 compile to v_pk_add_f32 / v_pk_mul_f32, fma2 to v_pk_fma_f32.  Each
// component is rounded exactly as the scalar instruction rounds it, so a packed multiply or add may stand in for a
// scalar one wherever results must stay bit-identical (the class-2 blend kernels pair a lane's two x halves).
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ inline f2 f2s(float x) { return f2{x, x}; }
__device__ inline f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
// a * b rounded per component even inside a block that lets multiply-adds fuse
__device__ inline f2 mul_rounded(f2 a, f2 b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ inline f2 sel2(bool c0, bool c1, f2 a, f2 b) { return f2{c0 ? a.x : b.x, c1 ? a.y : b.y}; }

// ---------------------------------------------------------------- lane masks of the class-2 blend kernels
// A per-lane decision of a wave-per-tile kernel is kept as a 64-bit scalar (one bit per lane, an SGPR pair), never as a
// `bool`: hipcc carries a bool that lives across a wave-uniform branch as a 0/1 VGPR and turns it back into a mask with
// a second compare, and it compares again for the negation of a condition.  The compare helpers deliver the mask
// straight from a VOP3 v_cmp (llvm.amdgcn.fcmp: the ballot of the compare over the active lanes; ordered
// predicates, so a NaN operand gives 0 exactly as the C++ operators do).  The select helpers issue one
// v_cndmask_b32_e64 reading the mask; they are inline asm only because C++ has no select that takes a lane mask.
// HAZARD (gfx940 and later, gfx950 included): a VALU instruction that writes an SGPR pair must be followed by two wait
// states before a VALU instruction reads that pair, a select mask included.  hipcc pads its own v_cmp -> v_cndmask
// pairs with `s_nop 1` on this target; it does not look into an asm string.  The types keep the pair apart instead of a
// pad: a compare returns a `cmask`, which no select helper accepts; and / and-not / or / complement of cmasks (and of
// lmasks) are scalar-ALU instructions and return an `lmask`, the only thing a select helper takes, and a scalar-ALU
// result read by a vector instruction needs no wait state.  A condition that is compared and selected on directly, with
// no scalar logic in between, uses the compiler's own select (`sel2`, `?:`), which hipcc pads or fills.  The operands
// of the selects are never the direct result of a transcendental (exp, rcp) either.  The asm is not volatile: the
// compiler may schedule, merge or drop a select like any pure operation.  Callers run with every lane active.
typedef unsigned long long lmask;   // a mask written by the scalar ALU
struct cmask {                      // a mask written by a vector compare: combine it before any select reads it
  unsigned long long bits;
};
enum { LM_OGT = 2, LM_OGE = 3, LM_OLT = 4, LM_OLE = 5 };   // llvm::CmpInst predicate codes
__device__ inline cmask mask_lt(float a, float b) { return cmask{__builtin_amdgcn_fcmpf(a, b, LM_OLT)}; }
__device__ inline cmask mask_le(float a, float b) { return cmask{__builtin_amdgcn_fcmpf(a, b, LM_OLE)}; }
__device__ inline cmask mask_gt(float a, float b) { return cmask{__builtin_amdgcn_fcmpf(a, b, LM_OGT)}; }
__device__ inline cmask mask_ge(float a, float b) { return cmask{__builtin_amdgcn_fcmpf(a, b, LM_OGE)}; }
__device__ inline lmask operator&(cmask a, cmask b) { return a.bits & b.bits; }
__device__ inline lmask operator&(lmask a, cmask b) { return a & b.bits; }
__device__ inline lmask operator&(cmask a, lmask b) { return a.bits & b; }
__device__ inline lmask operator|(cmask a, cmask b) { return a.bits | b.bits; }
__device__ inline lmask operator~(cmask a) { return ~a.bits; }
__device__ inline int mask_count(lmask m) { return __builtin_popcountll(m); }
// m ? a : b per lane
__device__ inline float mask_sel(lmask m, float a, float b) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
  return r;
}
__device__ inline uint32_t mask_sel(lmask m, uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
  return r;
}
// m ? a : 0 and m ? 1 : 0 (the zero and the one are inline constants of the instruction)
__device__ inline float mask_sel0(lmask m, float a) {
  float r;
  asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(a), "s"(m));
  return r;
}
__device__ inline uint32_t mask_one(lmask m) {
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(r) : "s"(m));
  return r;
}
__device__ inline f2 mask_sel2(lmask m0, lmask m1, f2 a, f2 b) { return f2{mask_sel(m0, a.x, b.x), mask_sel(m1, a.y, b.y)}; }
__device__ inline f2 mask_sel2_0(lmask m0, lmask m1, f2 a) { return f2{mask_sel0(m0, a.x), mask_sel0(m1, a.y)}; }

// wave64 sum through DPP; the total ends up in lane 63.
template <int CTRL>
__device__ inline float dpp_mov(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// 4-way lane-dependent select t[(m + K) & 3], m = 2*m1 + m0 (3 v_cndmask).
template <int K>
__device__ inline float sel4(const float (&t)[4], bool m0, bool m1) {
  const float lo = m0 ? t[(1 + K) & 3] : t[K & 3];
  const float hi = m0 ? t[(3 + K) & 3] : t[(2 + K) & 3];
  return m1 ? hi : lo;
}

// Sums v[0..15] over the 64 lanes with a transposed reduce-scatter: two quad_perm exchange
// steps (16 -> 8 -> 4 values per lane), one rotate step inside each 16-lane row (4 -> 1) and
// two cross-row adds.  Afterwards lane l of EVERY row holds the wave total of slot
//   8*(l&1) + 4*((l>>1)&1) + ((l>>2)&3).
// Used by the forward kernels only (the per-Gaussian weight and contribution sums).  The class-2 backward uses
// wave_reduce16_swap below; the forward keeps this one because another order of the adds would change the bits of
// `contributions` and of the weight sums.
__device__ inline float wave_reduce16(const float (&v)[16], int lane) {
  const bool b0 = lane & 1, b1 = lane & 2;
  float u[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float send = b0 ? v[k] : v[k + 8];
    const float keep = b0 ? v[k + 8] : v[k];
    u[k] = keep + dpp_mov<0xb1>(send);  // quad_perm [1,0,3,2]
  }
  float t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float send = b1 ? u[k] : u[k + 4];
    const float keep = b1 ? u[k + 4] : u[k];
    t[k] = keep + dpp_mov<0x4e>(send);  // quad_perm [2,3,0,1]
  }
  // lanes {c, c+4, c+8, c+12} of a row share the slot base; lane c+4m ends with slot base+m.
  // row_ror:4k delivers the value of lane (l - 4k) mod 16, whose group index is m-k, so a
  // sender with group index m' offers t[(m'+k)&3].
  const bool m0 = lane & 4, m1 = lane & 8;
  float r = sel4<0>(t, m0, m1);
  r += dpp_mov<0x124>(sel4<1>(t, m0, m1));  // row_ror:4
  r += dpp_mov<0x128>(sel4<2>(t, m0, m1));  // row_ror:8
  r += dpp_mov<0x12c>(sel4<3>(t, m0, m1));  // row_ror:12
  // cross-row adds r[l] + r[l ^ 16], then + the same of l ^ 32, on the vector ALU: gfx950's v_permlane16_swap /
  // v_permlane32_swap exchange rows / halves between two registers, no LDS round trip (a ds_bpermute costs ~64 cycles
  // of latency, twice per record here).  Inline asm: this hipcc maps both results of the builtin to one register.
  {
    float a = r, b = r;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    r = a + b;
    a = r; b = r;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    r = a + b;
  }
  return r;
}

// The same 16 sums for the class-2 blend backward (blend_bwd_tile_kernel, raster_bwd.hip), which has the 16 terms as packed
// pairs and is bound by vector issue: the WIDE stages go through the swaps, the narrow ones through DPP.
//   fold           16 adds                       x + y of each pair
//   16 -> 8        8 x (v_permlane32_swap, add)  swap(a, b) leaves a = {a.lo, b.lo}, b = {a.hi, b.hi}: a + b is a's sum
//                                                over the halves in lanes 0-31 and b's in lanes 32-63
//   8 -> 4         4 x (v_permlane16_swap, add)  the same between rows 0|1 and 2|3
//   4 -> 2 -> 1    quad_perm exchanges as in wave_reduce16 (two v_cndmask and one DPP add per output)
//   row_ror:4, :8  sum over the row's four quads
// One output register costs two instructions on a swap stage and three on an exchange stage, and a swap's operands need
// no copies (wave_reduce16 swaps a value with itself).  55 vector instructions against 72 for fold + wave_reduce16; the
// forward kernels keep wave_reduce16, so every forward output keeps its bits.
// Values travel by POSITION p: positions p and p + 8 meet in the first stage, p and p + 4 in the second, and lane l
// ends with position 4*(l >> 4) + 2*(l & 1) + ((l >> 1) & 1); the 16 lanes with (l & 12) == 0 hold the row.  Slot
// red16_slot(p) travels at position p.  The map puts the six slots that are zero in 3DGS mode at positions 3, 7, 11, 15
// (zero meets zero in both stages) and 6, 14 (in the first): ZERO6 leaves out their folds, four swaps and four adds.
// Inline asm: this hipcc maps both results of __builtin_amdgcn_permlane32_swap to one register (v_add_f32 v1, v1, v1).
// The swaps of a stage stand behind ONE s_nop 1 (two wait states between a VALU write and a swap's read).
__host__ __device__ constexpr int red16_slot(int pos) {
  constexpr int m[16] = {G_MX, G_MY, G_CONX, G_NX, G_CONY, G_CONZ, G_ZLO, G_NY, G_OPAC, G_R, G_G, G_NZ, G_B, G_PZ, G_ZHI, G_Q};
  return m[pos];
}
__device__ inline int red16_lane_slot(int lane) {
  const int pos = 4 * (lane >> 4) + 2 * (lane & 1) + ((lane >> 1) & 1);
  // slot of position p in nibble p (a table indexed by a lane value would live in memory)
  constexpr unsigned long long packed = [] {
    unsigned long long w = 0;
    for (int q = 0; q < 16; ++q) w |= (unsigned long long)red16_slot(q) << (4 * q);
    return w;
  }();
  return (int)((packed >> (4 * pos)) & 15ull);
}

#define PINGS_SWAP3(op, a0, b0, a1, b1, a2, b2)                                     \
  asm volatile("s_nop 1\n\t" op " %0, %3\n\t" op " %1, %4\n\t" op " %2, %5"         \
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(b0), "+v"(b1), "+v"(b2))
#define PINGS_SWAP4(op, a0, b0, a1, b1, a2, b2, a3, b3)                             \
  asm volatile("s_nop 1\n\t" op " %0, %4\n\t" op " %1, %5\n\t" op " %2, %6\n\t" op " %3, %7" \
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3))
#define PINGS_SWAP5(op, a0, b0, a1, b1, a2, b2, a3, b3, a4, b4)                     \
  asm volatile("s_nop 1\n\t" op " %0, %5\n\t" op " %1, %6\n\t" op " %2, %7\n\t" op " %3, %8\n\t" op " %4, %9" \
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4))
#define PINGS_SWAP7(op, a0, b0, a1, b1, a2, b2, a3, b3, a4, b4, a5, b5, a6, b6)                                \
  asm volatile("s_nop 1\n\t" op " %0, %7\n\t" op " %1, %8\n\t" op " %2, %9\n\t" op " %3, %10\n\t"              \
               op " %4, %11\n\t" op " %5, %12\n\t" op " %6, %13"                                               \
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6),                          \
                 "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6))
#define PINGS_SWAP8(op, a0, b0, a1, b1, a2, b2, a3, b3, a4, b4, a5, b5, a6, b6, a7, b7)                        \
  asm volatile("s_nop 1\n\t" op " %0, %8\n\t" op " %1, %9\n\t" op " %2, %10\n\t" op " %3, %11\n\t"             \
               op " %4, %12\n\t" op " %5, %13\n\t" op " %6, %14\n\t" op " %7, %15"                             \
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7),               \
                 "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7))

// (r0, r1) = (a0 + b0, a1 + b1) as one packed add
__device__ inline void pair_add(float& r0, float& r1, float a0, float a1, float b0, float b1) {
  const f2 r = f2{a0, a1} + f2{b0, b1};
  r0 = r.x;
  r1 = r.y;
}

// ZEROS: which slots the caller knows to be +0 — RED_ZERO6 (3DGS, above) or RED_ZERO3 (a surfel record interior to its
// tile, blend_interior: G_ZLO, G_ZHI at positions 6 and 14, which meet in the first stage, and G_PZ at 13): their
// folds are left out, and the swap and the add where zero meets zero.  Where a zero meets a sum the add stays
// (-0 + 0 = +0), so the result has the bits of the full reduction.
enum { RED_FULL = 0, RED_ZERO6 = 1, RED_ZERO3 = 2 };
template <int ZEROS>
__device__ inline float wave_reduce16_swap(const f2 (&v2)[16], int lane) {
  constexpr bool ZERO6 = ZEROS == RED_ZERO6, ZERO3 = ZEROS == RED_ZERO3;
  float s[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const bool zero = (ZERO6 && ((q & 3) == 3 || (q & 7) == 6)) || (ZERO3 && (q == 6 || q == 13 || q == 14));
    s[q] = zero ? 0.f : v2[red16_slot(q)].x + v2[red16_slot(q)].y;
  }
  float u[8], t[4];
  if (ZERO6) {
    PINGS_SWAP5("v_permlane32_swap_b32", s[0], s[8], s[1], s[9], s[2], s[10], s[4], s[12], s[5], s[13]);
    // neighbouring positions are added as packed pairs (v_pk_add_f32)
    pair_add(u[0], u[1], s[0], s[1], s[8], s[9]);
    pair_add(u[4], u[5], s[4], s[5], s[12], s[13]);
    u[2] = s[2] + s[10];
    float z = 0.f;                                        // position 6 is zero: position 2 swaps with a zero register
    PINGS_SWAP3("v_permlane16_swap_b32", u[0], u[4], u[1], u[5], u[2], z);
    pair_add(t[0], t[1], u[0], u[1], u[4], u[5]);
    t[2] = u[2] + z;
    t[3] = 0.f;
  } else if (ZERO3) {
    PINGS_SWAP7("v_permlane32_swap_b32", s[0], s[8], s[1], s[9], s[2], s[10], s[3], s[11], s[4], s[12], s[5], s[13],
                s[7], s[15]);
    pair_add(u[0], u[1], s[0], s[1], s[8], s[9]);
    pair_add(u[2], u[3], s[2], s[3], s[10], s[11]);
    pair_add(u[4], u[5], s[4], s[5], s[12], s[13]);       // position 13 is a zero register: -0 + 0 = +0 as in the full form
    u[7] = s[7] + s[15];
    u[6] = 0.f;                                           // 6 and 14 are zero in both halves
    PINGS_SWAP4("v_permlane16_swap_b32", u[0], u[4], u[1], u[5], u[2], u[6], u[3], u[7]);
#pragma unroll
    for (int k = 0; k < 4; k += 2) pair_add(t[k], t[k + 1], u[k], u[k + 1], u[k + 4], u[k + 5]);
  } else {
    PINGS_SWAP8("v_permlane32_swap_b32", s[0], s[8], s[1], s[9], s[2], s[10], s[3], s[11], s[4], s[12], s[5], s[13],
                s[6], s[14], s[7], s[15]);
#pragma unroll
    for (int k = 0; k < 8; k += 2) pair_add(u[k], u[k + 1], s[k], s[k + 1], s[k + 8], s[k + 9]);
    PINGS_SWAP4("v_permlane16_swap_b32", u[0], u[4], u[1], u[5], u[2], u[6], u[3], u[7]);
#pragma unroll
    for (int k = 0; k < 4; k += 2) pair_add(t[k], t[k + 1], u[k], u[k + 1], u[k + 4], u[k + 5]);
  }
  const bool b0 = lane & 1, b1 = lane & 2;
  float x[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float send = b0 ? t[k] : t[k + 2];
    const float keep = b0 ? t[k + 2] : t[k];
    x[k] = keep + dpp_mov<0xb1>(send);  // quad_perm [1,0,3,2]
  }
  float r = (b1 ? x[1] : x[0]) + dpp_mov<0x4e>(b1 ? x[0] : x[1]);  // quad_perm [2,3,0,1]
  r += dpp_mov<0x124>(r);  // row_ror:4
  r += dpp_mov<0x128>(r);  // row_ror:8
  // keeps the last add a DPP add: behind the caller's store predicate it would become a move, a DPP move and an add
  asm volatile("" : "+v"(r));
  return r;
}

__device__ inline float wave_reduce_sum_dpp(float v) {
  // quad_perm [1,0,3,2], [2,3,0,1], row_ror:4, row_ror:8, row_bcast:15, row_bcast:31
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xb1, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4e, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));
  return v;
}

// wave64 integer sum through DPP; the total ends up in lane 63.
__device__ inline uint32_t wave_reduce_sum_u32_dpp(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
  return v;
}

__device__ inline float wave_sum_to_all(float v) {
  v = wave_reduce_sum_dpp(v);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// wave64 inclusive integer sum
__device__ inline uint32_t wave_inclusive_sum(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// the same sum by DPP row shifts and row broadcasts: six vector instructions, no LDS crossbar round trips
__device__ inline uint32_t wave_inclusive_sum_dpp(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
  return v;
}

// ---------------------------------------------------------------- longest-processing-time-first tile dispatch
// A tile's blend time is proportional to its list; the lists are very uneven (Metric-1: 0..374 blended records,
// mean 127), and workgroups are dispatched in grid order: with tiles in image order the long ones that start late
// run on an otherwise idle chip.  Dispatching tiles in descending work order fills the tail with short ones.
// One workgroup of 1,024 threads: counting sort of the tiles by min(work / 16, 1023), descending.  FROM_RANGES: a
// tile's work is the length of its list, taken from `ranges` directly (forward order) instead of from a `work` array.
// The body of tile_order_kernel (raster_fwd.hip) and of the extra workgroup of the backward's live-scan reduce launch
// (raster_scan.hip).
template <bool FROM_RANGES>
__device__ inline void tile_order_body(const uint32_t* __restrict__ work_in, const uint2* __restrict__ ranges,
                                       int num_tiles, uint32_t* __restrict__ order, uint32_t* __restrict__ n_long,
                                       uint32_t long_thr, uint32_t long_max) {
  __shared__ uint32_t hist[1024];
  __shared__ uint32_t base[1024];
  __shared__ uint32_t wtot[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto work = [&](int t) -> uint32_t {
    if constexpr (FROM_RANGES) { const uint2 r = ranges[t]; return r.y - r.x; }
    else return work_in[t];
  };
  hist[tid] = 0u;
  __syncthreads();
  for (int t = tid; t < num_tiles; t += 1024) atomicAdd(&hist[min(work(t) >> 4, 1023u)], 1u);
  __syncthreads();
  // scan over the bins in DESCENDING bin order (bin 1023 first); 1024 threads, one bin each: inside the wave, then
  // the totals of the waves in front out of LDS
  const uint32_t v = hist[1023 - tid];
  uint32_t incl = wave_inclusive_sum(v, lane);
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w) incl += w < wave ? wtot[w] : 0u;
  base[tid] = incl;
  hist[1023 - tid] = incl - v;   // hist[bin] = first output position of the bin
  __syncthreads();
  for (int t = tid; t < num_tiles; t += 1024) order[atomicAdd(&hist[min(work(t) >> 4, 1023u)], 1u)] = (uint32_t)t;
  // tiles with work >= long_thr (a multiple of 16: whole bins) are the first entries of the order: their number.
  // The order WITHIN a bin is the arrival order of the LDS atomics above, so a cap that cut through a bin would make
  // the set of tiles the backward splits depend on timing.  The cap therefore takes whole bins only: the longest
  // prefix of bins (from the top, down to the threshold's) whose tiles number at most long_max — if the top bin alone
  // holds more, nothing is split.  A threshold above the top bin (work >> 4 is clamped to 1023) splits nothing either.
  if (n_long) {
    const uint32_t bin = long_thr >> 4;
    if (bin > 1023u) {
      if (tid == 0) *n_long = 0u;
    } else {
      // base[k] = inclusive count of bins 1023 .. 1023 - k, non-decreasing in k: exactly one thread writes
      const uint32_t kmax = 1023u - bin;
      const uint32_t k = (uint32_t)tid;
      if (k <= kmax && base[k] <= long_max && (k == kmax || base[k + 1] > long_max)) *n_long = base[k];
      if (tid == 0 && base[0] > long_max) *n_long = 0u;
    }
  }
}

// ---------------------------------------------------------------- prefix sums (raster_scan.hip)
// what the scans of the backward read: the stored element -> uint32_t
struct LiveOp {
  __host__ __device__ uint32_t operator()(const float& w) const { return w > 0.f ? 1u : 0u; }
};
struct PopOp {
  __host__ __device__ uint32_t operator()(const uint8_t& m) const { return (uint32_t)__builtin_popcount((unsigned)m & 15u); }
};
// per depth rank r: the Gaussian's rows are the compact range [cidx[first slot], cidx[end slot]); its number of
// <= CH-row chunks is the input of the pair_off scan, computed as the scan reads it (entry P = 0) instead of by a
// pass of its own through an array
struct RowRanges {
  int P;
  const uint32_t *offsets_sorted, *tiles_sorted, *cidx;
  __host__ __device__ uint32_t row_begin(uint32_t r) const { return cidx[offsets_sorted[r] - tiles_sorted[r]]; }
  __host__ __device__ uint32_t row_end(uint32_t r) const { return cidx[offsets_sorted[r]]; }
  __host__ __device__ uint32_t operator()(const uint32_t& r) const {
    if (r >= (uint32_t)P) return 0u;
    return (row_end(r) - row_begin(r) + (uint32_t)CH - 1u) / (uint32_t)CH;
  }
};

// Sums modulo 2^32 of n elements read through the functor, exclusive unless said otherwise; out[n], 16-byte aligned
// like every blob field.  Up to SCAN_MAX elements: two launches of the project's own (reduce, apply; one when a single
// workgroup holds them all), beyond, or with `library` (PINGS_RASTER_SCAN=l): hipcub::DeviceScan.  temp: at least
// raster_scan_bytes(n) bytes.
constexpr int SCAN_THREADS = 1024, SCAN_BLOCK = 4 * SCAN_THREADS;   // elements a workgroup of the scan owns
constexpr int64_t SCAN_MAX = (int64_t)SCAN_BLOCK * SCAN_BLOCK;      // one uint4 of totals per thread
size_t raster_scan_bytes(int64_t n);
int raster_scan_u32(const uint32_t* in, int64_t n, bool inclusive, uint32_t* out, void* temp, size_t temp_bytes,
                    bool library, hipStream_t st);
// The backward's tile order, computed by one extra workgroup of the live scan's reduce launch (unlike work in one
// launch: it shares no data with the scan).  work == nullptr: no tile order.  With `library` it is a launch of its own.
struct TileOrderJob {
  const uint32_t* work = nullptr;
  int num_tiles = 0;
  uint32_t *order = nullptr, *n_long = nullptr;
  uint32_t long_thr = 0, long_max = 0;
};
int raster_scan_live(const float* inst_w, int64_t n, uint32_t* cidx, void* temp, size_t temp_bytes, bool library,
                     const TileOrderJob& job, hipStream_t st);
int raster_scan_pop(const uint8_t* inst_qmask, int64_t n, uint32_t* cidx, void* temp, size_t temp_bytes, bool library,
                    const TileOrderJob& job, hipStream_t st);
// pair_off[0 .. P], then pair_owner[q] = r for q in [pair_off[r], pair_off[r + 1]) (pair_owner_kernel)
int raster_scan_chunks(const RowRanges& rr, uint32_t* pair_off, uint32_t* pair_owner, void* temp, size_t temp_bytes,
                       bool library, hipStream_t st);

// ---------------------------------------------------------------- sub-tile culling
// A record contributes to a pixel only if alpha = min(0.99, o exp(power)) >= 1/255, i.e.
// q(d) = cx dx^2 + 2 cy dx dy + cz dy^2 <= 2 ln(255 o).  `footprint_misses_rect` is true when the smallest q over
// a closed pixel rectangle exceeds that bound by more than the fp32 error the blend kernels' own evaluation of
// `power` can have (the terms cancel for large anisotropic footprints, so the margin scales with their
// magnitude): no pixel of the rectangle can pass the alpha test, and skipping the record for the wave that owns
// the rectangle leaves every output bit unchanged.
// v_rcp_f32 / __expf on the device, 1 / x and expf on the host: the functions below that the host tests and tools call
// through the library (pings_raster_debug_interior) carry margins that cover either.
__host__ __device__ inline float fast_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(x);
#else
  return 1.0f / x;
#endif
}
__host__ __device__ inline float fast_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __expf(x);
#else
  return expf(x);
#endif
}

__host__ __device__ inline float edge_min_q(float a, float b, float c, float d_fixed, float lo, float hi) {
  // q along the edge {fixed offset d_fixed on one axis, free offset t in [lo, hi] on the other}:
  //   q(t) = a d^2 + 2 b d t + c t^2, minimised at t* = -b d / c, clamped to the edge
  // (1-ulp reciprocal: an error dt in t raises q by c dt^2 ~ 1e-14 c t^2, far below the margin)
  const float t = fminf(fmaxf(-(b * d_fixed) * fast_rcp(c), lo), hi);
  const float q0 = a * d_fixed * d_fixed, q1 = 2.f * b * d_fixed * t, q2 = c * t * t;
  return (q0 + q1 + q2) - 2e-5f * (q0 + fabsf(q1) + q2);
}

__device__ inline bool footprint_misses_rect(float mx, float my, float cx, float cy, float cz, float thr,
                                             float x0, float x1, float y0, float y1) {
  if (mx >= x0 && mx <= x1 && my >= y0 && my <= y1) return false;  // centre inside: q = 0
  const float lx = x0 - mx, hx = x1 - mx, ly = y0 - my, hy = y1 - my;
  float m = edge_min_q(cx, cy, cz, lx, ly, hy);             // edge x = x0
  m = fminf(m, edge_min_q(cx, cy, cz, hx, ly, hy));         // edge x = x1
  m = fminf(m, edge_min_q(cz, cy, cx, ly, lx, hx));         // edge y = y0
  m = fminf(m, edge_min_q(cz, cy, cx, hy, lx, hx));         // edge y = y1
  return m > thr;                                           // NaN -> false (keep)
}

// Bit q = 1 iff the record may touch the 8x8 pixel quadrant q = (qx + 2 qy) of the 16x16 tile at (X0, Y0).
__device__ inline uint32_t quadrant_mask(float mx, float my, float opacity, float cx, float cy, float cz,
                                         float X0, float Y0) {
  const float thr = 2.f * __logf(255.f * opacity) + 2e-3f;
  uint32_t m = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float x0 = X0 + (float)(8 * (q & 1)), y0 = Y0 + (float)(8 * (q >> 1));
    if (!footprint_misses_rect(mx, my, cx, cy, cz, thr, x0, x0 + 7.f, y0, y0 + 7.f)) m |= 1u << q;
  }
  return m;
}

// a_min = a lower bound of the alpha the blend kernels give ANY of the 256 pixel positions of the tile at (X0, Y0)
// (largest q at the tile corners, fp32 error margins included); 0 if some pixel might be rejected by the
// alpha >= 1/255 or power <= 0 tests, in particular for the tile that holds the centre.  The occlusion bound
// (raster_fwd.hip) and blend_interior below rest on it.
__host__ __device__ inline float tile_min_alpha(float mx, float my, float o, float cx, float cy, float cz, float X0, float Y0) {
  const float x1 = X0 + 15.f, y1 = Y0 + 15.f;
  if (mx >= X0 && mx <= x1 && my >= Y0 && my <= y1) return 0.f;
  float qmax = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float dx = ((c & 1) ? x1 : X0) - mx, dy = ((c & 2) ? y1 : Y0) - my;
    const float q0 = cx * dx * dx, q1 = 2.f * cy * dx * dy, q2 = cz * dy * dy;
    qmax = fmaxf(qmax, (q0 + q1 + q2) + 2e-5f * (q0 + fabsf(q1) + q2));
  }
  const float a = fminf(ALPHA_MAX, o * fast_exp(-0.5f * (qmax + 1e-3f)) * (1.f - 1e-5f));
  if (!(a >= ALPHA_MIN * 1.001f)) return 0.f;
  // the smallest q over the tile must be safely positive, or the kernel's `power <= 0` test might drop a pixel
  const float lx = X0 - mx, hx = x1 - mx, ly = Y0 - my, hy = y1 - my;
  float m = edge_min_q(cx, cy, cz, lx, ly, hy);
  m = fminf(m, edge_min_q(cx, cy, cz, hx, ly, hy));
  m = fminf(m, edge_min_q(cz, cy, cx, ly, lx, hx));
  m = fminf(m, edge_min_q(cz, cy, cx, hy, lx, hx));
  if (!(m > 1e-6f)) return 0.f;
  return a;
}

// ---------------------------------------------------------------- records interior to a tile (class-2 blend kernels)
// For most (record, tile) pairs the per-pixel decisions of the blend come out the same at all 256 pixel positions.
// blend_interior is true only if that is CERTAIN, for every position of the 16x16 tile (positions outside the image
// included), in the kernels' own fp32 evaluation; blend_bwd_tile_kernel then runs a trip without those decisions (the
// forward's such body was measured and is not kept: DESIGN §8 item 1, r18).  A wrong
// `true` changes output bits, a wrong `false` only costs time, and every comparison is written so that a NaN gives false.
//   (a) alpha: every pixel passes alpha >= ALPHA_MIN and power <= 0 (tile_min_alpha > 0: the smallest q over the tile
//       exceeds 1e-6, so power < -4e-7), and opacity < ALPHA_MAX: exp(power) <= 1 there (a result above 1 would take
//       an error of more than 4e-7, six ulp), rounding is monotone, so opacity * exp(power) <= ALPHA_MAX and
//       min(ALPHA_MAX, .) is the identity, as is the backward's `raw <= ALPHA_MAX`.
//   (b) surfel depth: den = nx rx + ny ry + nz < -DEN_EPS at every pixel and zlo < d0 = q / den < zhi, so that the
//       ray hit is taken and med3(d0, zlo, zhi) = d0.  rx = (x - cxp) / fx is a correctly rounded quotient, monotone
//       in x, so every pixel's (rx, ry) lies in the box of the tile's first and last column and row (TileRays: the
//       kernels' own expressions at those pixels).  den is affine in (rx, ry): in exact arithmetic its extremes over
//       the box are at the corners, and d0 is monotone in den while den keeps its sign, so its extremes are at the
//       corners with the largest and the smallest den.
//       Margins.  With u = 2^-24 and mag = |nx| max|rx| + |ny| max|ry| + |nz|: the forward's (nx rx + ny ry) + nz
//       rounds two products and two sums, the backward's fma(nx, rx, fma(ny, ry, nz)) two fmas; every intermediate is
//       at most mag (1 + 3u), so either is within 4 u mag = 2.4e-7 mag of the exact value, and so are the corner values
//       computed here.  E_DEN = 1e-6 mag is more than twice the sum of both.  For d0 = q * rcp(den): the relative error
//       of den is at most 2.4e-7 mag / |den|, v_rcp_f32 is good to one ulp (1.2e-7) and the product rounds once
//       (0.6e-7); the corner values here carry the same (1 / x and a product on the host).  The relative margin
//       1e-6 mag / |den|_min + 1e-6 is more than twice the sum of both again, taken of the larger |d0|.
struct TileRays {
  float rx0, rx1, ry0, ry1;   // (x - cxp) / fx at columns X0 and X0 + 15, (y - cyp) / fy at rows Y0 and Y0 + 15
};
__host__ __device__ inline TileRays tile_rays(float X0, float Y0, float cxp, float cyp, float fx, float fy) {
  return TileRays{(X0 - cxp) / fx, ((X0 + 15.f) - cxp) / fx, (Y0 - cyp) / fy, ((Y0 + 15.f) - cyp) / fy};
}
// the four wave-uniform values in scalar registers: they live across the whole record loop
__device__ inline TileRays tile_rays_uniform(const TileRays& t) {
  auto u = [](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); };
  return TileRays{u(t.rx0), u(t.rx1), u(t.ry0), u(t.ry1)};
}
constexpr float INTERIOR_DEN_MARGIN = 1e-6f, INTERIOR_D0_MARGIN = 1e-6f;
// a = {mx, my, opacity, pz}, b = {conic x, y, z, rz}, q and (nx, ny, nz) as in the record (see the top of the file)
__host__ __device__ inline bool blend_interior(float mx, float my, float opacity, float pz, float cx, float cy, float cz,
                                               float rz, float q, float nx, float ny, float nz, float X0, float Y0,
                                               const TileRays& t) {
  if (!(opacity < ALPHA_MAX)) return false;   // (0.99 itself would do; the strict test keeps the boundary out)
  const float ax = fmaxf(fabsf(t.rx0), fabsf(t.rx1)), ay = fmaxf(fabsf(t.ry0), fabsf(t.ry1));
  const float e_den = INTERIOR_DEN_MARGIN * (fabsf(nx) * ax + fabsf(ny) * ay + fabsf(nz));
  const float y0 = ny * t.ry0, y1 = ny * t.ry1, x0 = nx * t.rx0, x1 = nx * t.rx1;
  const float d00 = (x0 + y0) + nz, d10 = (x1 + y0) + nz, d01 = (x0 + y1) + nz, d11 = (x1 + y1) + nz;
  const float den_max = fmaxf(fmaxf(d00, d10), fmaxf(d01, d11)), den_min = fminf(fminf(d00, d10), fminf(d01, d11));
  if (!(den_max + e_den < -DEN_EPS)) return false;
  const float inv_max = fast_rcp(den_max);   // the largest |1 / den|
  const float da = q * inv_max, db = q * fast_rcp(den_min);
  const float dlo = fminf(da, db), dhi = fmaxf(da, db);
  const float m = fmaxf(fabsf(da), fabsf(db)) * (INTERIOR_D0_MARGIN - e_den * inv_max);   // inv_max < 0
  if (!(dlo - m > pz - rz && dhi + m < pz + rz)) return false;
  return tile_min_alpha(mx, my, opacity, cx, cy, cz, X0, Y0) > 0.f;
}

}  // namespace raster
}  // namespace pings
