/* pings_hip.h — C ABI of libpings_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary of the PINGS render + SDF-query hot path
 * (SURVEY.md §8b).  Every entry point is `extern "C"`, takes plain device
 * pointers, sizes and an opaque `hipStream_t` (passed as void*), returns an
 * integer status (0 = ok) and never throws.  All pointers are DEVICE pointers
 * unless a parameter is documented as host.  All floating point is fp32, all
 * tensors are dense row-major (the layout torch hands over).
 *
 * The reference binds this functionality through three CUDA torch extensions
 * whose sources are absent from the reference checkout (empty submodules,
 * /root/reference/.gitmodules:1-9) and through plain PyTorch code; each block
 * below cites the reference call site it replaces.
 */
#ifndef PINGS_HIP_H_
#define PINGS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__cplusplus)
#define PINGS_EXTERN_C extern "C"
#else
#define PINGS_EXTERN_C
#endif
#define PINGS_API PINGS_EXTERN_C __attribute__((visibility("default")))

/* status codes */
#define PINGS_OK 0
#define PINGS_ERR_ARG 1      /* bad shape / null pointer / unsupported option */
#define PINGS_ERR_HIP 2      /* a HIP runtime call failed                      */
#define PINGS_ERR_CAPACITY 3 /* caller-provided buffer too small               */

/* ------------------------------------------------------------------ general */

/* ABI version of this header (bumped on any signature change).  A binding compares pings_abi_version() of the
 * library it loaded with the PINGS_ABI_VERSION of the header it was written against (pings_amd/_lib.py does). */
#define PINGS_ABI_VERSION 11
PINGS_API int pings_abi_version(void);
/* Message of the last failing call on this thread ("" if none). Host string. */
PINGS_API const char* pings_last_error(void);

/* Per-stage HIP-event timing of everything this library launches (bench.py's roofline
 * figures).  pings_prof_report synchronises the device and writes "name count total_ms"
 * lines into a HOST buffer, then clears the record.  Each recorded stage costs two event packets on the stream
 * (~10 us of idle time between dependent launches): pings_prof_only("stage") restricts the record to one stage
 * (NULL / "" = all), which is what bench.py's timed region uses for the dominant kernel. */
PINGS_API int pings_prof_enable(int on);
PINGS_API int pings_prof_only(const char* stage);
PINGS_API int pings_prof_report(char* buf, size_t cap);

/* --------------------------------------------------------------- fused SSIM
 * Replaces `fused_ssim.fused_ssim(img1, img2, train=...)`
 * (reference call sites utils/mapper.py:1243,1922,1951; arithmetic of the
 * in-tree torch predecessor gaussian_splatting/utils/loss_utils.py:189-219:
 * 11x11 Gaussian window sigma 1.5, zero "same" padding, C1=0.01^2, C2=0.03^2,
 * mean over all elements).  Images are [planes, H, W] with planes = N*C.
 */

/* Number of floats of scratch `partials` needed by pings_ssim_forward. */
PINGS_API size_t pings_ssim_partials_count(int planes, int H, int W);

/* out_mean[1] <- mean SSIM.  If train != 0 the three partial-derivative maps
 * ([planes,H,W] each) are written for the backward pass; otherwise they may be
 * NULL.  Deterministic (two-stage reduction, no atomics). */
PINGS_API int pings_ssim_forward(const float* img1, const float* img2, int planes, int H, int W,
                                 int train, float* out_mean, float* dm_dmu1,
                                 float* dm_dsigma1_sq, float* dm_dsigma12, float* partials,
                                 void* stream);

/* dL_dimg1[planes,H,W] <- gradient of (dL_dmean * mean SSIM) w.r.t. img1.
 * dL_dmean is a 1-element device buffer (the upstream scalar gradient). */
PINGS_API int pings_ssim_backward(const float* img1, const float* img2, int planes, int H, int W,
                                  const float* dL_dmean, const float* dm_dmu1,
                                  const float* dm_dsigma1_sq, const float* dm_dsigma12,
                                  float* dL_dimg1, void* stream);


/* ------------------------------------------- Gaussian(-surfel) rasteriser
 * Replaces the `diff_gaussian_surfel_rasterization` / `diff_gaussian_rasterization`
 * torch extensions (absent CUDA submodules, /root/reference/.gitmodules:1-6) at the
 * interface the reference calls them through:
 *   GaussianRasterizationSettings(...)  gaussian_renderer/__init__.py:149-166, :185-199
 *   GaussianRasterizer.markVisible      gaussian_renderer/__init__.py:215
 *   GaussianRasterizer.__call__         gaussian_renderer/__init__.py:318-326, :415-423
 *   its autograd backward               triggered by utils/mapper.py:1581
 * Semantics are those of oracle/raster_cpu.py (assumptions listed in DESIGN.md).
 *
 * Memory protocol: three opaque scratch blobs sized by the *_bytes queries and
 * allocated by the caller (torch's caching allocator in the Python wrapper);
 * the same blobs must be handed unchanged to pings_raster_backward.
 */
#define PINGS_RASTER_SURFEL 0
#define PINGS_RASTER_3DGS 1
#define PINGS_RASTER_2DGS 2   /* only the pings_raster2d_* entry points below accept it */

typedef struct pings_raster_settings {
  int32_t image_height, image_width;
  int32_t mode;           /* PINGS_RASTER_SURFEL | PINGS_RASTER_3DGS | PINGS_RASTER_2DGS  */
  int32_t front_only;     /* config[4] of the surfel settings (surfel mode only)          */
  double tanfovx, tanfovy;
  double scale_modifier;
  const float* bg;             /* device [3]                                               */
  const float* viewmatrix;     /* device [4,4] row-major = T_cw^T   (cameras.py:214)       */
  const float* projmatrix;     /* device [4,4] = viewmatrix @ P^T   (cameras.py:216)       */
  const float* projmatrix_raw; /* device [4,4] = P^T                (cameras.py:68-70)     */
  const float* prcppoint;      /* device [2] = (cx/W, cy/H) (cameras.py:61); NULL = centre */
} pings_raster_settings;

/* present[N] (uint8) <- 1 where the point lies inside the view frustum. */
PINGS_API int pings_raster_mark_visible(const float* positions, int N,
                                        const pings_raster_settings* s, uint8_t* present,
                                        void* stream);

PINGS_API size_t pings_raster_geom_bytes(int P, int image_height, int image_width);
PINGS_API size_t pings_raster_binning_bytes(int64_t num_instances, int image_height,
                                            int image_width);
PINGS_API size_t pings_raster_image_bytes(int image_height, int image_width);

/* Stage 1: per-Gaussian projection, culling, depth sort, occlusion bound and tile counting.
 * Writes radii[P] (int32, 0 = culled) and *num_instances (HOST int64: number of
 * (Gaussian, tile) pairs that can still reach a pixel: pairs behind the depth rank at which a
 * conservative bound proves every pixel of the tile saturated are never created; set
 * PINGS_RASTER_OCCLUSION=0 in the environment to keep them all) and *footprint_class (HOST: 1 = footprints of a few
 * tiles, 2 = of many tiles; hand it unchanged to pings_raster_render / pings_raster_backward, which pick their blend
 * kernels by it: 1 -> one pixel per lane forward, Gaussian-per-lane wave scans backward; 2 -> two pixels per lane,
 * pixel-per-lane backward).  Synchronises `stream` once to return the two. */
PINGS_API int pings_raster_preprocess(const pings_raster_settings* s, int P, const float* means3D,
                                      const float* colors, const float* opacities,
                                      const float* scales, const float* rotations,
                                      void* geom_blob, int32_t* radii, int64_t* num_instances,
                                      int32_t* footprint_class, void* stream);
/* The same for a frame whose producer kernels left row counts on the DEVICE (`render`, gaussian_renderer/__init__.py:
 * 219,305,563-569,730-737 are four host synchronisations in the reference; this call is the one of the frame here):
 * of the first `dyn_rows` Gaussians only rows [0, *live_rows_dev) exist (the rest of that worst-case sized block is
 * culled without being read); rows [dyn_rows, P) are ordinary.  live_rows_dev NULL = every row exists.
 * aux_dev: HOST array of up to 8 DEVICE pointers to int32 words (NULL entries read as 0) that are copied to the HOST
 * array aux_host in the same read-back as the instance count. */
PINGS_API int pings_raster_preprocess_dyn(const pings_raster_settings* s, int P, const float* means3D,
                                          const float* colors, const float* opacities, const float* scales,
                                          const float* rotations, void* geom_blob, int32_t* radii,
                                          const int32_t* live_rows_dev, int dyn_rows,
                                          const int32_t* const* aux_dev, int aux_words, int32_t* aux_host,
                                          int64_t* num_instances, int32_t* footprint_class, void* stream);

/* Stage 2: instance binning (stable tile sort) and per-tile alpha blending.
 * Outputs are planar [C,H,W].  out_normal may be NULL in 3DGS mode.  `per_gaussian`
 * is float contributions[P] (surfel: sum of blend weights over pixels) or int32
 * n_touched[P] (3DGS: pixels where the Gaussian is seen with transmittance > 0.5).
 */
PINGS_API int pings_raster_render(const pings_raster_settings* s, int P, int64_t num_instances,
                                  void* geom_blob, void* binning_blob, void* image_blob,
                                  float* out_color, float* out_normal,
                                  float* out_depth, float* out_alpha, void* per_gaussian,
                                  int footprint_class, void* stream);

/* The tile sort of stage 2 on its own (tests): keys[n] of key_bytes = 2 | 4 bytes on the device -> keys_sorted[n] in
 * stable order of their low `bits` bits and values[n] = the element index each came from.  bits <= 16 runs the
 * project's two-pass radix sort unless `library` is non-zero; wider keys, or `library`, run rocprim::radix_sort_pairs.
 * scratch: device memory of pings_raster_tile_sort_bytes(n, ...) bytes, which also reports the pairs a workgroup of
 * the sort owns (block_pairs, nullable). */
PINGS_API size_t pings_raster_tile_sort_bytes(int64_t n, int32_t* block_pairs);
PINGS_API int pings_raster_tile_sort(const void* keys, int64_t n, int key_bytes, int bits, void* keys_sorted,
                                     uint32_t* values, void* scratch, int library, void* stream);

/* The prefix sums of stages 1, 2 and the backward on their own (tests): out[i] = f(in[0]) + .. + f(in[i - 1]) modulo
 * 2^32, plus f(in[i]) when `inclusive` is non-zero.  kind 0: in is uint32_t[n], f the identity; 1: float[n], f(w) =
 * w > 0; 2: uint8_t[n], f(m) = popcount(m & 15).  in and out are 16-byte aligned.  Up to 16,777,216 elements run the
 * project's two-launch scan unless PINGS_RASTER_SCAN=l is set; longer ones, or that, run hipcub::DeviceScan.
 * temp: device memory of pings_raster_scan_bytes(n) bytes. */
PINGS_API size_t pings_raster_scan_bytes(int64_t n);
PINGS_API int pings_raster_scan_u32(const void* in, int64_t n, int kind, int inclusive, uint32_t* out, void* temp,
                                    size_t temp_bytes, void* stream);

/* Scratch bytes pings_raster_backward needs (an upper bound in the instance count: the
 * gradient rows of the instances that actually blended are a data-dependent subset). */
PINGS_API size_t pings_raster_backward_bytes(int P, int64_t num_instances);

/* Backward of stage 1+2.  dL_d* of the outputs may be NULL (treated as zero).
 * bwd_blob: device scratch of pings_raster_backward_bytes(P, num_instances) bytes.
 * Gradient outputs are overwritten (not accumulated); dL_dmeans2D[P,3] receives the
 * screen-space positional gradient (xy, z = 0) the reference reads through
 * `viewspace_points`; dL_dtau[6] = [d rho, d theta] for T_cw <- SE3_exp(tau) T_cw
 * (utils/campose_utils.py:79-98).  Deterministic: no floating-point atomics. */
PINGS_API int pings_raster_backward(const pings_raster_settings* s, int P, int64_t num_instances,
                                    const float* means3D, const float* colors,
                                    const float* opacities, const float* scales,
                                    const float* rotations, const void* geom_blob,
                                    const void* binning_blob, const void* image_blob,
                                    const float* out_color, const float* out_normal,
                                    const float* out_depth, const float* out_alpha,
                                    const float* dL_dcolor, const float* dL_dnormal,
                                    const float* dL_ddepth, const float* dL_dalpha,
                                    void* bwd_blob, float* dL_dmeans3D, float* dL_dmeans2D,
                                    float* dL_dcolors, float* dL_dopacities, float* dL_dscales,
                                    float* dL_drotations, float* dL_dtau, int footprint_class,
                                    void* stream);

/* Debug / parity taps (tests only): copies of the sorted instance list and the
 * per-tile ranges out of the binning blob, and per-pixel state out of the image blob. */
PINGS_API int pings_raster_debug_lists(const void* binning_blob, int64_t num_instances,
                                       int image_height, int image_width, uint32_t* point_list,
                                       uint32_t* ranges_xy, void* stream);
PINGS_API int pings_raster_debug_image(const void* image_blob, int image_height, int image_width,
                                       float* final_T, uint32_t* n_contrib, void* stream);
/* The occlusion budget out of a geometry blob: `*occ_nb` (host) = rank buckets per tile for this image size;
 * occ_bucket [occ_nb x tiles] fixed-point budget words, bucket-major; occ_bsat [tiles] last rank bucket a tile
 * needs (0xFFFF = all).  With both device pointers null only `*occ_nb` is written (to size the copies). */
PINGS_API int pings_raster_debug_occlusion(const void* geom_blob, int P, int image_height, int image_width,
                                           uint32_t* occ_bucket, uint16_t* occ_bsat, int32_t* occ_nb,
                                           void* stream);
/* The rank bucket of the occlusion budget for each of `n` depth ranks, computed on the HOST by the function the
 * kernels call (host pointers, no GPU work): buckets[i] = bucket of ranks[i] among `nvalid` surviving Gaussians with
 * `occ_nb` buckets per tile.  Non-decreasing in the rank, 0 for rank 0, below occ_nb. */
PINGS_API int pings_raster_rank_bucket(const int32_t* ranks, int64_t n, int occ_nb, uint32_t nvalid,
                                       uint32_t* buckets);
/* How the calling thread's last pings_raster_render built its tile lists (host values, no GPU work): *plan = 1 if it
 * gathered them from the front depth ranks, 0 if it duplicated and sorted (or had no instance); *front = the front
 * depth (1 + the last depth rank that keeps a tile) the thread's last pings_raster_preprocess read back, 0xFFFFFFFF
 * if that frame cannot gather (footprint class 1 under the default rule, or PINGS_BIN=s) and nobody looked for it.  The
 * environment knob PINGS_BIN=s|g forces the sort, or the gather wherever its tables fit. */
PINGS_API int pings_raster_debug_bin_plan(int32_t* plan, uint32_t* front);
/* Which (surfel record, 16x16 tile) pairs the wave-per-tile blend backward treats as interior, computed on the HOST by
 * the function the kernel calls (host pointers, no GPU work).  records [n][16]: the four float4 of a record as the
 * geometry blob holds them ({mx, my, opacity, pz} {conic x, y, z, rz} {r, g, b, q} {nx, ny, nz, -}); tile_origins
 * [n][2]: pixel coordinates of the tile's first pixel; cxp = prcp.x * width - 0.5 and cyp likewise, fx, fy: the
 * camera terms of the per-pixel ray.  flags[i] = 1 only if, at all 256 pixel positions of the tile, the record passes
 * the alpha tests unclamped and takes the unclamped ray hit of its depth (csrc/raster_common.hpp: blend_interior). */
PINGS_API int pings_raster_debug_interior(const float* records, const float* tile_origins, int64_t n, float cxp,
                                          float cyp, float fx, float fy, uint8_t* flags);


/* ------------------------------------------- 2D Gaussian splatting rasteriser
 * Replaces the `diff_surfel_rasterization` torch extension (gaussian_renderer/__init__.py:88-89; settings :167-181;
 * outputs consumed :349-409): ray-splat intersection of Huang et al. 2024, restated in tests/raster2d_ref.py
 * (assumptions in DESIGN.md §3).  A parallel set of entry points with its own blobs: the settings struct is the one
 * above with mode = PINGS_RASTER_2DGS (projmatrix = full_proj_transform is what it reads; projmatrix_raw, prcppoint
 * and front_only are ignored); modes 0 / 1 are unchanged and the pings_raster_* entries reject mode 2.
 * Scales are [P,2] (two tangent axes).  Same memory protocol: geom / binning / image blobs sized by the queries,
 * handed unchanged to pings_raster2d_backward. */
PINGS_API size_t pings_raster2d_geom_bytes(int P, int image_height, int image_width);
PINGS_API size_t pings_raster2d_binning_bytes(int64_t num_instances, int image_height, int image_width);
PINGS_API size_t pings_raster2d_image_bytes(int image_height, int image_width);

/* Stage 1: per-Gaussian splat-to-pixel matrix, screen centre, radius (radii[P], 0 = culled), published tile square,
 * camera-frame normal, depth key, tiles-per-Gaussian scan.  Synchronises `stream` once: *num_instances (HOST, summed
 * in 64 bits; 2^31 - 1 pairs or more return PINGS_ERR_CAPACITY) and, in the same read-back, up to 6 device int32
 * words aux_dev[i] -> aux_host[i] (HOST arrays; aux_words = 0: unused).
 * live_rows_dev (nullable): of the first dyn_rows Gaussians only rows [0, *live_rows_dev) exist (as in
 * pings_raster_preprocess_dyn). */
PINGS_API int pings_raster2d_preprocess(const pings_raster_settings* s, int P, const float* means3D,
                                        const float* colors, const float* opacities, const float* scales,
                                        const float* rotations, void* geom_blob, int32_t* radii,
                                        const int32_t* live_rows_dev, int dyn_rows, const int32_t* const* aux_dev,
                                        int aux_words, int32_t* aux_host, int64_t* num_instances, void* stream);

/* Stage 2: binning (stable sort by tile, then depth, then Gaussian index) and front-to-back blending.
 * out_color [3,H,W] = C + T bg;  out_allmap [7,H,W] = {expected depth (not normalised), 1 - T, normal xyz,
 * median depth (0 = none), depth distortion}. */
PINGS_API int pings_raster2d_render(const pings_raster_settings* s, int P, int64_t num_instances, void* geom_blob,
                                    void* binning_blob, void* image_blob, float* out_color, float* out_allmap,
                                    void* stream);

PINGS_API size_t pings_raster2d_backward_bytes(int P, int64_t num_instances);

/* Backward of stage 1+2 w.r.t. means3D [P,3], colours [P,3], opacities [P,1], scales [P,2], rotations [P,4]
 * (overwritten).  dL_dcolor [3,H,W] / dL_dallmap [7,H,W] may be NULL (zero).  dL_dmeans2D [P,3] receives the
 * gradient w.r.t. the screen centre through the low-pass branch (xy, z = 0).  Deterministic: no float atomics. */
PINGS_API int pings_raster2d_backward(const pings_raster_settings* s, int P, int64_t num_instances,
                                      const float* scales, const float* rotations, const void* geom_blob,
                                      const void* binning_blob, const void* image_blob, const float* dL_dcolor,
                                      const float* dL_dallmap, void* bwd_blob, float* dL_dmeans3D,
                                      float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacities,
                                      float* dL_dscales, float* dL_drotations, void* stream);

/* Parity taps (tests only): sorted Gaussian ids and tile ranges; final T, last contributor (list position + 1,
 * relative to the tile's range) and median contributor (list position, -1 = none) per pixel. */
PINGS_API int pings_raster2d_debug_lists(const void* binning_blob, int64_t num_instances, int image_height,
                                         int image_width, uint32_t* point_list, uint32_t* ranges_xy, void* stream);
PINGS_API int pings_raster2d_debug_image(const void* image_blob, int image_height, int image_width, float* final_T,
                                         uint32_t* n_contrib, int32_t* median, void* stream);

/* -------------------------------------------- neural-point kNN + SDF decode
 * Replaces, for the query path, `NeuralPoints.radius_neighborhood_search`
 * (model/neural_gaussians.py:1061-1115), the search / filter / top-k part of
 * `NeuralPoints.query_feature` (:506-569) and, fused, the whole of `Mapper.sdf`
 * (utils/mapper.py:2273-2289 = query_feature + Decoder.sdf (model/decoder.py:62-104)
 * + inverse-distance weighting) with its analytic gradient (utils/tools.py:409-419).
 * All index tensors keep the reference's dtypes (int64 table / indices, int32
 * timestamps, uint8 bool masks) so the reference's own tensors are passed as they are.
 */
typedef struct pings_knn_map {
  const int64_t* table;          /* buffer_pt_index[buffer_size], -1 = empty (neural_gaussians.py:86-88) */
  int64_t buffer_size;
  const float* neural_points;    /* [Np,3] global positions                                   */
  const int32_t* point_ts_create;/* [Np]   (travel-distance window; may be NULL if !time_filtering) */
  const float* travel_dist;      /* [T]                                                        */
  int32_t cur_ts;
  int32_t time_filtering;        /* temporal_local_map_on && query_locally (:535)              */
  float diff_travel_dist_local;
  const uint8_t* free_mask;      /* [Np] free_gs_mask;  used iff use_free_mask  (:544-546)     */
  const uint8_t* valid_mask;     /* [Np] valid_gs_mask; used iff use_valid_mask (:548-550)     */
  int32_t use_free_mask, use_valid_mask;
  const int64_t* global2local;   /* [Np+1] or NULL for a global query (:553-554)               */
  const int32_t* neighbor_dx;    /* [K,3] cell offsets (:1030-1043)                            */
  int32_t K;
  int32_t nn_k;                  /* config.query_nn_k (<= 16)                                  */
  float resolution;              /* voxel size                                                 */
  float max_valid_dist2;         /* 3*((n+1)*res)^2 (:1058)                                    */
  const void* compact;           /* optional compact mirror of `table` (pings_knn_compact_build); when
                                    non-NULL the lookups go there (same results, cache resident)  */
  uint32_t compact_mask;         /* entries - 1                                                */
  const void* blocks;            /* optional cell-block index (pings_knn_blocks_build): block table ...   */
  const void* block_records;     /* ... its packed 32-byte point records ...                              */
  const int32_t* blocks_ok;      /* ... and its status word on the device: the kernels take the index only
                                    when it reads 1 and fall back to `compact` / `table` otherwise        */
  uint32_t block_mask;           /* block-table entries - 1                                               */
} pings_knn_map;

/* Compact, cache-resident mirror of the (>= 99 % empty) dense hash table: open addressing over
 * `entries` = pings_knn_compact_entries(num_points) 8-byte {slot+1, value} buckets.  A lookup
 * returns exactly table[slot] (or -1), so results are unchanged; the 81 random gathers of a
 * query then hit L2 / Infinity Cache instead of missing to HBM.  Rebuild after every change of
 * `table` (the wrapper keys it on the tensor's version counter). */
PINGS_API size_t pings_knn_compact_entries(int64_t num_points);
PINGS_API int pings_knn_compact_build(const int64_t* table, int64_t buffer_size, void* compact,
                                      size_t entries, void* stream);

/* Cell-block index: the search-side state of the map re-laid for locality.  The reference's table is keyed by a
 * hash of the CELL (neural_gaussians.py:1078-1084), so the 81 neighbour cells of a query are 81 unrelated 64-byte
 * sectors, and every live candidate costs further gathers (position, creation time, masks, local index).  The index
 * groups 4x4x4 cells into a block {packed block coordinate, 64-bit occupancy, first record} found through a small
 * open-addressing table, and keeps one 32-byte record per registered point {x, y, z, global index, global2local,
 * travel distance at creation, free / valid bits}: a query reads ~8 block entries and its ~10 live records instead
 * of ~120 sectors.  A point is registered iff table[hash(cell(point))] == point, i.e. iff the reference's lookup of
 * its own cell returns it.  Results equal the table path's exactly when (a) every non-empty table slot holds a
 * registered point and (b) no two distinct cells closer than the acceptance radius share a slot; the build verifies
 * (a) on the device and (b) on the host, writes status[0] = 1 only then, and the search kernels test that word.
 *
 * `m` carries the tensors to bake: table, buffer_size, neural_points, resolution, max_valid_dist2 and — each
 * optional, NULL = not baked, a query that needs it must then not pass the index — point_ts_create + travel_dist,
 * free_mask, valid_mask, global2local.  max_abs_dx = max |neighbor_dx| (host value).  blocks:
 * pings_knn_blocks_entries(num_points) * 32 bytes; records: max(num_points, 1) * 32 bytes; status: 8 int32
 * {ok, registered points, non-empty slots, out-of-range blocks, records, 0, 0, 0}.  Rebuild after ANY change of the
 * baked tensors. */
PINGS_API size_t pings_knn_blocks_entries(int64_t num_points);
PINGS_API int pings_knn_blocks_build(const pings_knn_map* m, int64_t num_points, int64_t num_timestamps,
                                     int32_t max_abs_dx, void* blocks, size_t entries, void* records,
                                     int32_t* status, void* stream);

/* idx[B,nn_k] (int64, -1 = none; local indices iff global2local != NULL), d2[B,nn_k]
 * (9e3 where idx = -1, :562), nn_counts[B] (int64: valid candidates over all K cells, :557).
 * Neighbours are ordered by squared distance, ties by candidate cell order.
 * global_idx[B,nn_k] (optional, may be NULL): the neighbours' indices before the
 * global2local mapping, i.e. the rows of `neural_points` the distances were measured to. */
PINGS_API int pings_knn_search(const pings_knn_map* m, const float* queries, int64_t B,
                               int64_t* idx, float* d2, int64_t* nn_counts, int64_t* global_idx,
                               void* stream);
/* `NeuralPoints.radius_neighborhood_search` itself (model/neural_gaussians.py:1061-1115): d2[B,K] (float) and idx[B,K]
 * (int64, -1 = no point) for every candidate cell, with the reference's step order (time window, python index -1 =
 * the last point, max_valid_dist2 for empty entries, collisions keep their distance).  num_points = rows of
 * neural_points.  The fused entry points never form this pair; `query_certainty` (:1117-1133) consumes it. */
PINGS_API int pings_knn_cells(const pings_knn_map* m, const float* queries, int64_t B, int64_t num_points, float* d2,
                              int64_t* idx, void* stream);

/* ---- NeuralPoints.query_feature (model/neural_gaussians.py:506-725): forward, backward, double backward ----
 * The tables are the LOCAL ones for a local query (local_geo_features [N_local+1, Fg], local_color_features,
 * local_neural_points, local_point_orientations, local_point_certainties) or the global ones; `m` carries the
 * search-side tensors (always the global neural_points / table / masks, plus global2local for a local query). */
typedef struct pings_qf_tables {
  const float* geo_features;    /* [rows, Fg] or NULL (query_geo_feature = False)                       */
  const float* color_features;  /* [rows, Fc] or NULL (query_color_feature = False / no colour table)   */
  int32_t Fg, Fc;               /* 0 when the table is NULL                                             */
  const float* points;          /* [rows - 1 .. rows, 3] positions in the index space of the features   */
  const float* orientations;    /* [.., 4] wxyz, read only when after_pgo (:627-630)                    */
  const float* certainties;     /* [..] read for the queried certainty (:691-695); may be NULL          */
  int32_t after_pgo;
  int32_t weighted_first;       /* config.weighted_first (:701-705): outputs are [B, F+3] weighted sums */
} pings_qf_tables;

/* Forward.  geo_out / color_out: [B, nn_k, F+3] (or [B, F+3] when weighted_first), NULL = not queried;
 * w_out [B, nn_k] normalised inverse-distance weights (:644-662; all 0 for a query without neighbours);
 * idx_out / gidx_out [B, nn_k] int64 (-1 = none): rows of the queried tables / of the global point array
 * (they differ for a local query: the weights are measured to the GLOBAL point, :1098-1101);
 * nn_counts [B] int64 over all K cells (:557); certainty [B] (optional).
 * Side effects of training mode (:664-689), each optional: certainty_accum[row] += w (float atomics, as the
 * reference's scatter_add_; pass a zeroed DELTA buffer distinct from t->certainties and add it to the table
 * afterwards: the queried certainty must see the values from before the accumulation, :615-620 vs :664-689),
 * ts_update[row] = max(ts_update[row], query_ts[b]) (integer atomics, exact). */
PINGS_API int pings_query_feature_forward(const pings_knn_map* m, const pings_qf_tables* t, const float* queries,
                                          int64_t B, float* geo_out, float* color_out, float* w_out,
                                          int64_t* idx_out, int64_t* gidx_out, int64_t* nn_counts,
                                          float* certainty, float* certainty_accum, const int32_t* query_ts,
                                          int32_t* ts_update, float* n_out, void* stream);
/* certainties[idx[p]] += w[p] for the n_pairs = B * nn_k pairs a forward call returned (idx < 0 skipped): the training-
 * mode accumulation of :664-689 as its own O(B nn_k) launch behind the forward kernel (stream order guarantees that the
 * queried certainty, :691-695, was computed from the values before the accumulation).  Float atomics, as the
 * reference's scatter_add_. */
PINGS_API int pings_query_feature_accumulate(const int64_t* idx, const float* w, int64_t n_pairs, float* certainties,
                                             void* stream);
/* n_out [B, nn_k, 3] (optional): the neighbour vectors on their own (they are also columns F..F+2 of the rows). */

/* Backward: upstream g_geo / g_color (shapes of the forward outputs, NULL = none) and g_w [B, nn_k] ->
 * g_x [B,3] (through the neighbour vectors AND the weights; squared distances stay in the graph, :1099-1101),
 * g_geo_features [rows, Fg] / g_color_features [rows, Fc] (dense, every row written; NULL = not wanted):
 * the deterministic row scatter-add of the upstream gradient (pings_rows_scatter_add).
 * `global_points` = m->neural_points of the forward.  scratch: pings_query_feature_scratch_bytes(B, nn_k, rows). */
PINGS_API size_t pings_query_feature_scratch_bytes(int64_t B, int nn_k, int64_t rows);
PINGS_API int pings_query_feature_backward(const pings_qf_tables* t, const float* global_points,
                                           const float* queries, int64_t B, int nn_k, const int64_t* idx,
                                           const int64_t* gidx, const float* g_geo, const float* g_color,
                                           const float* g_n, const float* g_w, int64_t rows, void* scratch,
                                           float* g_x, float* g_geo_features, float* g_color_features,
                                           void* stream);
/* Split layout (per-neighbour mode): g_n [B, nn_k, 3] != NULL carries the neighbour-vector part of the upstream
 * gradient on its own (g_geo / g_color are then ignored and the feature rows are scattered separately with
 * pings_rows_plan_build / _apply) — the autograd wrapper keeps the table path and the query path in separate graph
 * nodes so that get_gradient(x, sdf) does not pay for a table scatter nobody asked for. */

/* Backward of the backward (get_gradient(..., create_graph=True), utils/tools.py:409-419; used by
 * utils/mapper.py:874-875,:1445-1448): given gg_x [B,3] (and, optionally, gg_*_features [rows, F]) — the
 * gradients w.r.t. the backward's outputs — the gradients w.r.t. its inputs: d_g_geo / d_g_color (shapes of
 * g_geo / g_color), d_g_w [B, nn_k], d_x [B,3] (optional) and, in weighted_first mode only, the feature tables
 * d_geo_features / d_color_features [rows, F] (per-neighbour mode: the backward does not depend on them). */
PINGS_API int pings_query_feature_double_backward(
    const pings_qf_tables* t, const float* global_points, const float* queries, int64_t B, int nn_k,
    const int64_t* idx, const int64_t* gidx, const float* g_geo, const float* g_color, const float* g_w,
    const float* gg_x, const float* gg_geo_features, const float* gg_color_features, int64_t rows, void* scratch,
    float* d_g_geo, float* d_g_color, float* d_g_n, float* d_g_w, float* d_x, float* d_geo_features,
    float* d_color_features, void* stream);
/* d_g_n [B, nn_k, 3] (split layout, see above): replaces d_g_geo / d_g_color. */

/* Deterministic scatter-add of rows — the backward of a row gather `table[idx]`
 * (model/neural_gaussians.py:565-579; the reference's autograd uses atomics there):
 *   out[r, 0:F] = sum over pairs p with dst_row[p] == r, in ascending p, of w[p] * src[src_row[p] * ld + 0:F]
 * and 0 for rows nothing points at (every row of out[rows, F] is written; no memset needed).
 * dst_row[p] < 0 or >= rows skips the pair; w == NULL: weight 1; src_row == NULL: pair p reads row p.
 * F <= 64.  Counting sort by destination (integer atomics only) + one pass over the table: bitwise
 * reproducible.  `scratch`: pings_rows_scatter_add_scratch_bytes(n_pairs, rows) bytes. */
PINGS_API size_t pings_rows_scatter_add_scratch_bytes(int64_t n_pairs, int64_t rows);
PINGS_API int pings_rows_scatter_add(const int64_t* dst_row, int64_t n_pairs, const float* src, int64_t ld,
                                     int32_t F, const float* w, const int64_t* src_row, int64_t rows,
                                     void* scratch, float* out, void* stream);
/* The same in two steps for several tables sharing one destination index: `plan` (caller-owned,
 * pings_rows_plan_bytes(n_pairs, rows) bytes) is built once and applied per table; pair p reads row p of src. */
PINGS_API size_t pings_rows_plan_bytes(int64_t n_pairs, int64_t rows);
PINGS_API int pings_rows_plan_build(const int64_t* dst_row, int64_t n_pairs, int64_t rows, void* plan, void* stream);
PINGS_API int pings_rows_plan_apply(const void* plan, int64_t n_pairs, int64_t rows, const float* src, int64_t ld,
                                    int32_t F, const float* w, float* out, void* stream);

typedef struct pings_sdf_decoder {
  const float* W1;   /* [hidden, F+3] layers.0.weight (decoder.py:49) */
  const float* b1;   /* [hidden]                                      */
  const float* W2;   /* [1, hidden]   lout.weight                      */
  const float* b2;   /* [1]                                            */
  int32_t hidden;    /* <= 64                                          */
  int32_t feat_dim;  /* F (<= 61)                                      */
  float sdf_scale;   /* decoder.py:55-57                               */
  int32_t weighted_first; /* config.weighted_first (neural_gaussians.py:701) */
} pings_sdf_decoder;

/* Fused inference query: sdf[B]; optional (may be NULL) grad_x[B,3] = d sdf / d query,
 * nn_counts[B] (int64), certainty[B].  `features` is [rows, F] (local or global table matching
 * the index space of the search), `points`/`orientations`/`certainties` likewise
 * ([rows,3], [rows,4] wxyz or NULL unless after_pgo, [rows] or NULL). No side effects. */
PINGS_API int pings_sdf_forward(const pings_knn_map* m, const pings_sdf_decoder* dec,
                                const float* features, const float* points,
                                const float* orientations, const float* certainties,
                                int32_t after_pgo, const float* queries, int64_t B, float* sdf,
                                float* grad_x, int64_t* nn_counts, float* certainty,
                                int64_t* idx_out, float* w_out, float* sdf_std, int64_t* gidx_out,
                                void* stream);
/* idx_out[B,nn_k] / w_out[B,nn_k] (optional): the neighbours (in the index space of `features`) and
 * their normalised inverse-distance weights, kept for pings_sdf_backward; gidx_out[B,nn_k] (optional): the same
 * neighbours as rows of m->neural_points (what the weights were measured to), kept for pings_sdf_double_backward.  sdf_std[B] (optional): spread of the
 * per-neighbour predictions sqrt(sum_m w_m (s_m - sdf)^2), the tracker's validity filter
 * (utils/tracker.py:303-313,408); 0 in weighted_first mode. */

/* Which kernel a fused query of this shape runs: out[0] = family (0 vector ALU, lane per hidden unit; 1 matrix core,
 * four queries per wave step), out[1] = the kernel's padded input width class.  `order`: 0 pings_sdf_forward,
 * 1 pings_sdf_backward, 2 pings_sdf_double_backward.  `misaligned`: the feature table (for the backward also its
 * scratch) is not 16-byte aligned.  Honours PINGS_SDF_FWD / PINGS_SDF_BWD = vector like the launches themselves, which
 * follow the same plan.  Needs no device and launches nothing. */
PINGS_API int pings_sdf_plan(int nn_k, int feat_dim, int hidden, int weighted_first, int order, int misaligned,
                             int32_t* out);

/* Fused colour query with its Jacobian (csrc/knn_color.hip): the colour head of Tracker.query_source_points
 * (utils/tracker.py:328-336) for the photometric term and the colour-consistency weight of the tracker.
 * One hidden level, ReLU, biases, sigmoid on the output (Decoder.regress_color, model/decoder.py:133). */
typedef struct pings_color_decoder {
  const float* W1;        /* [hidden, Fc+3] layers.0.weight                  */
  const float* b1;        /* [hidden]                                        */
  const float* W2;        /* [channels, hidden] lout.weight                  */
  const float* b2;        /* [channels]                                      */
  int32_t hidden;         /* <= 64                                           */
  int32_t feat_dim;       /* Fc (<= 61)                                      */
  int32_t channels;       /* 1..3                                            */
  int32_t weighted_first; /* config.weighted_first                           */
} pings_color_decoder;
/* color[B,channels] and, when `jac` is not NULL, jac[B,channels,3] = d colour / d query (through the neighbour vectors
 * and through the inverse-distance weights).  idx[B,nn_k]: rows of the tables passed (`features` [rows,Fc], `points`
 * [rows,3], `orientations` [rows,4] wxyz, read when after_pgo), -1 = no neighbour: what pings_sdf_forward(idx_out) and
 * pings_knn_search emit, so the search is not repeated.  A query without a neighbour gets colour 0 (sigmoid(mlp(0)) in
 * weighted_first mode) and a zero Jacobian.  No side effects. */
PINGS_API int pings_color_forward(const pings_color_decoder* dec, const float* features, int64_t rows,
                                  const float* points, const float* orientations, int32_t after_pgo,
                                  const float* queries, int64_t B, const int64_t* idx, int32_t nn_k, float* color,
                                  float* jac, void* stream);

/* First-order backward of the fused query w.r.t. the feature table and the decoder
 * (the training path of Mapper.sdf_mapping, utils/mapper.py:822-970: loss(sdf).backward()).
 *   dL_dfeatures[rows,F]  dense, every row written (zero where no query touched the row)
 *   dL_dW1[H,F+3], dL_db1[H], dL_dW2[H], dL_db2[1]
 * One wave per query evaluates the decoder backward on the vector ALU (lane = hidden unit, weight-gradient rows
 * in registers), the per-(query, neighbour) feature-gradient rows are grouped by destination row (counting sort,
 * pings_rows_scatter_add below) and summed in ascending pair order; decoder gradients are per-workgroup partials
 * summed in fixed order.  Bitwise reproducible.  hidden <= 64.
 * `scratch` needs pings_sdf_backward_scratch_bytes(B, nn_k, F, H, feature_rows) bytes. */
PINGS_API size_t pings_sdf_backward_scratch_bytes(int64_t B, int nn_k, int feat_dim, int hidden,
                                                  int64_t feature_rows);
/* Backward of the backward: the consistency / Eikonal losses differentiate g = dS/dx (returned by
 * pings_sdf_forward as grad_x) once more (get_gradient(create_graph=True), utils/tools.py:409-419;
 * utils/mapper.py:1445-1448).  Given v[B,3] = dL/dg (times the dL/dS the first backward was called with), the
 * gradients of  sum_b <v_b, dS_b/dx>  w.r.t. the feature table and the decoder, same outputs, scratch and
 * determinism as pings_sdf_backward.  `gidx` [B,nn_k] / `global_points`: the rows of the global point array the
 * weights were measured to (pings_sdf_forward gidx_out; == idx / points for a global query).  The gradient w.r.t.
 * the query itself (a third derivative) is not produced. */
PINGS_API int pings_sdf_double_backward(const pings_sdf_decoder* dec, const float* features,
                                        int64_t feature_rows, const float* points, const float* orientations,
                                        const float* global_points, int32_t after_pgo, const float* queries,
                                        int64_t B, int nn_k, const int64_t* idx, const int64_t* gidx,
                                        const float* w, const float* v, void* scratch, float* d_features,
                                        float* d_W1, float* d_b1, float* d_W2, float* d_b2, void* stream);
PINGS_API int pings_sdf_backward(const pings_sdf_decoder* dec, const float* features,
                                 int64_t feature_rows, const float* points,
                                 const float* orientations, int32_t after_pgo, const float* queries,
                                 int64_t B, int nn_k, const int64_t* idx, const float* w,
                                 const float* dL_dsdf, void* scratch, float* dL_dfeatures,
                                 float* dL_dW1, float* dL_db1, float* dL_dW2, float* dL_db2,
                                 void* stream);


/* ------------------------------------------------------ decoder MLP (MFMA)
 * Replaces `Decoder.mlp` / `Decoder.mlp_batch` (model/decoder.py:62-98) for the one-hidden-level
 * ReLU decoders every shipped config builds (pings.py:147-172):
 *     y[N,OUT] = relu(x[N,IN] @ W1[HID,IN]^T + b1[HID]) @ W2[OUT,HID]^T + b2[OUT]
 * fp32 in / fp32 accumulate on the matrix cores (v_mfma_f32_32x32x2_f32: bitwise an fp32 fma chain).
 * Limits: IN <= 64, HID in {32,64,96,128}, OUT <= 32.
 */
PINGS_API size_t pings_mlp_backward_scratch_bytes(int IN, int HID, int OUT);
PINGS_API int pings_mlp_forward(const float* x, int64_t N, int IN, int HID, int OUT, const float* W1,
                                const float* b1, const float* W2, const float* b2, float* y,
                                void* stream);
/* Recomputes the hidden layer (nothing is saved by the forward).  dL_dx may be NULL.  Weight
 * gradients are per-workgroup partials summed in fixed order (no atomics). */
PINGS_API int pings_mlp_backward(const float* x, const float* dL_dy, int64_t N, int IN, int HID,
                                 int OUT, const float* W1, const float* b1, const float* W2,
                                 void* scratch, float* dL_dx, float* dL_dW1, float* dL_db1,
                                 float* dL_dW2, float* dL_db2, void* stream);
/* The backward of pings_mlp_backward's dL_dx output (the graph node autograd records when the mapper differentiates
 * dS/dx once more: utils/tools.py:409-419 `get_gradient(create_graph=True)`, used at utils/mapper.py:1445-1448 and
 * utils/tracker.py:317).  ddx[N,IN] = cotangent of dL_dx; outputs: d_dy[N,OUT] (cotangent of dL_dy), d_W1[HID,IN],
 * d_W2[OUT,HID]; nothing reaches x or b1 (piecewise-constant ReLU mask).  Shapes: HID = 64, OUT = 1 (`Decoder.sdf`,
 * model/decoder.py:100-104); _supported() says so, anything else is PINGS_ERR_ARG and the host wrapper composes the
 * node from device operators instead.  scratch: pings_mlp_backward_scratch_bytes(IN, HID, OUT). */
PINGS_API int pings_mlp_double_backward_supported(int IN, int HID, int OUT);
PINGS_API int pings_mlp_double_backward(const float* x, const float* ddx, const float* dL_dy, int64_t N, int IN,
                                        int HID, int OUT, const float* W1, const float* b1, const float* W2,
                                        void* scratch, float* d_dy, float* d_W1, float* d_W2, void* stream);

/* Several decoders over the SAME N rows in one launch each way (blockIdx.y = decoder): the five spawn decoders of
 * a view (gaussian_renderer/__init__.py:605-716; hidden 128, IN <= 32 — pings.py:156-160).  Results are bitwise
 * those of pings_mlp_forward / pings_mlp_backward called per decoder.  Unused directions leave their pointers NULL
 * (dL_dx may be NULL in the backward).  scratch: pings_mlp_backward_grouped_scratch_bytes(jobs, njobs). */
typedef struct pings_mlp_job {
  const float* x;                    /* [N, IN]                                   */
  int32_t IN, OUT;                   /* IN <= 32, OUT <= 32, hidden width = 128   */
  const float *W1, *b1, *W2, *b2;    /* [128, IN], [128], [OUT, 128], [OUT]       */
  float* y;                          /* forward:  [N, OUT]                        */
  const float* dL_dy;                /* backward: [N, OUT]                        */
  float* dL_dx;                      /*           [N, IN] or NULL                 */
  float *dL_dW1, *dL_db1, *dL_dW2, *dL_db2;
} pings_mlp_job;
PINGS_API int pings_mlp_forward_grouped(const pings_mlp_job* jobs, int njobs, int64_t N, void* stream);
/* N sizes the buffers and the grid; *n_rows_dev (device int32, NULL = N) rows are decoded, the rest is not touched. */
PINGS_API int pings_mlp_forward_grouped_dyn(const pings_mlp_job* jobs, int njobs, int64_t N, const int32_t* n_rows_dev,
                                            void* stream);
PINGS_API size_t pings_mlp_backward_grouped_scratch_bytes(const pings_mlp_job* jobs, int njobs);
PINGS_API int pings_mlp_backward_grouped(const pings_mlp_job* jobs, int njobs, int64_t N, void* scratch,
                                         void* stream);

/* ------------------------------------------------------- exposure correction of the rendered image
 * gaussian_renderer/__init__.py:449-461 (affine form): out[c, p] = sum_k M[c, k] img[k, p] + b[c] for the
 * [3, H W] planes — the reference's `img.permute(1,2,0).view(-1,3) @ M^T + b`, a GEMM with K = N = 3 there.
 * Backward: g_img (may be NULL), g_M [3,3], g_b [3]; sums in fp64, fixed order (bitwise reproducible).
 * scratch: pings_exposure_backward_scratch_bytes(). */
PINGS_API int pings_exposure_forward(const float* img, const float* M, const float* b, int64_t HW, float* out,
                                     void* stream);
PINGS_API size_t pings_exposure_backward_scratch_bytes(void);
PINGS_API int pings_exposure_backward(const float* img, const float* M, const float* g_out, int64_t HW,
                                      void* scratch, float* g_img, float* g_M, float* g_b, void* stream);

/* ------------------------------------------ finite-difference SDF gradient
 * The tensor code of `Mapper.get_numerical_gradient` (utils/mapper.py:2319-2370) around the fused SDF query:
 *   pings_stencil_points            x[N,3] -> [x+ex; x-ex; x+ey; x-ey; x+ez; x-ez] ([6N,3]; one-sided: 3 blocks, [3N,3])
 *   pings_sdf_forward / _backward   on the shifted points (above)
 *   pings_stencil_gradient          S[6N] -> grad[N,3] = (S+ - S-) / (2 eps)   (one-sided: (S+ - sdf_x) / eps)
 *   pings_stencil_gradient_backward dL/dgrad[N,3] -> dL/dS[6N] (one-sided also dL/dsdf_x[N], nullable)
 * Divisions are multiplications by the fp32 reciprocal of the fp32 divisor, as torch's device kernel for
 * tensor / python-float computes them. */
PINGS_API int pings_stencil_points(const float* x, int64_t N, float eps, int two_side, float* out, void* stream);
PINGS_API int pings_stencil_gradient(const float* sdf_shifted, const float* sdf_x, int64_t N, float eps, int two_side,
                                     float* grad, void* stream);
PINGS_API int pings_stencil_gradient_backward(const float* dL_dgrad, int64_t N, float eps, int two_side,
                                              float* dL_dsdf_shifted, float* dL_dsdf_x, void* stream);

/* ------------------------------------------------------- spawn_gaussians
 * Replaces the tensor code of `spawn_gaussians` around the five decoder MLPs
 * (gaussian_splatting/gaussian_renderer/__init__.py:469-778).  Call order for one view:
 *   pings_spawn_gather   -> dense per-view inputs of the MLPs          (:551-597,:672-675,:692-699)
 *   5 x pings_mlp_forward
 *   pings_spawn_plan     -> compacted row of every kept Gaussian + count (alpha > 0, scale filter; :727-761)
 *   pings_spawn_forward  -> activations + quaternion algebra, written to the compacted rows (:605-716)
 *   pings_spawn_backward -> gradients back to the raw MLP outputs (autograd of the same lines)
 * Raw MLP outputs are [n, d*k] row-major == [n*k, d]: Gaussian g = i*k + j of neural point i owns
 * floats g*d .. g*d+d-1 (the reference's .view(N*K, -1), :632,645,665,687,716).
 */
typedef struct {
  int n;                    /* neural points after the visible & valid mask */
  int k;                    /* Gaussians per neural point (Decoder.out_k) */
  int scale_dim;            /* scale-MLP columns per Gaussian (mlp_out_dim / k): 2 or 3 */
  int surfel;               /* 1: gaussian_surfel -> [s0, s1, 1e-7] (:668-670); 0: 3d_gs -> [s0, s1, s2] */
  int color_residual;       /* 1: clamp(base + 0.1 tanh(mlp), 0, 1) (:707-711); 0: sigmoid(mlp) (:714) */
  int alpha_filter_on;      /* keep tanh(alpha mlp) > 0 (:727-740) */
  int scale_filter_on;      /* keep any(scale > scale_filter_thr) (:747-761) */
  float displacement_range; /* displacement_range_ratio * resolution (:605) */
  float unit_scale;         /* unit_scale_ratio * resolution (:661) */
  float max_scale;          /* max_scale_ratio * resolution (:655) */
  float scale_filter_thr;   /* scale_filter_ratio * resolution (:751) */
} pings_spawn_params;

/* Rows `sel[n]` (int64; NULL = rows 0..n-1) of the map tensors -> pos[n,3], quat[n,4], base_color[n,3]
 * (if `color`), free_out[n] (if `free_mask`), geo_in[n, Fg + dist_concat], col_in[n, Fc + 3*view_concat],
 * view_dist[n] (nullable).  cam_origin: DEVICE [3] or NULL (then no view features).  xy_only zeroes the
 * z-component of the view vector before the norm (:592-597); the direction is rotated into the neural
 * point's frame with R(q) (apply_quaternion_rotation(quat_inverse(q), .), :695-696). */
PINGS_API int pings_spawn_gather(int n, const int64_t* sel, const float* position, const float* orientation,
                                 const float* color, const uint8_t* free_mask, const float* geo_feature, int Fg,
                                 const float* color_feature, int Fc, const float* cam_origin, int xy_only,
                                 int view_concat, int dist_concat, float* pos, float* quat, float* base_color,
                                 uint8_t* free_out, float* geo_in, float* col_in, float* view_dist,
                                 void* stream);
/* `_dyn` forms of gather / plan / forward: `n` (p->n) is the CAPACITY the buffers and grids are sized for and
 * *n_rows_dev (device int32; NULL = n) the rows the visible & valid mask actually selected (a count `render` no longer
 * reads back before spawning, gaussian_renderer/__init__.py:563-569): rows behind it are neither read nor written,
 * never kept by the plan, and the free-mask tiling (:724) uses the device count.  nan_flag (device int32, nullable):
 * zeroed by the plan, set to 1 by the forward when a spawned rotation is NaN (the reference's assert, :305-306). */
PINGS_API int pings_spawn_gather_dyn(int n, const int32_t* n_rows_dev, const int64_t* sel, const float* position,
                                     const float* orientation, const float* color, const uint8_t* free_mask,
                                     const float* geo_feature, int Fg, const float* color_feature, int Fc,
                                     const float* cam_origin, int xy_only, int view_concat, int dist_concat,
                                     float* pos, float* quat, float* base_color, uint8_t* free_out, float* geo_in,
                                     float* col_in, float* view_dist, void* stream);
PINGS_API int pings_spawn_plan_dyn(const pings_spawn_params* p, const int32_t* n_rows_dev, const float* alpha_raw,
                                   const float* scale_raw, const float* dist_ratio, void* scratch, int32_t* dest,
                                   int32_t* count, int32_t* nan_flag, void* stream);
PINGS_API int pings_spawn_forward_dyn(const pings_spawn_params* p, const int32_t* n_rows_dev, const float* xyz_raw,
                                      const float* rot_raw, const float* scale_raw, const float* alpha_raw,
                                      const float* color_raw, const float* pos, const float* quat,
                                      const float* base_color, const float* dist_ratio, const uint8_t* free_in,
                                      const int32_t* dest, float* gaussian_xyz, float* gaussian_scale,
                                      float* gaussian_rot, float* gaussian_alpha, float* gaussian_color,
                                      float* alpha_all, uint8_t* gaussian_free_mask, int32_t* nan_flag,
                                      void* stream);
/* Scatter of the per-view feature gradients (leading dimensions ldg / ldc, first Fg / Fc columns) into
 * rows `sel` of the map-sized, PRE-ZEROED gradient tensors.  Either pair may be NULL. */
PINGS_API int pings_spawn_gather_backward(int n, const int64_t* sel, const float* dL_dgeo_in, int Fg, int ldg,
                                          const float* dL_dcol_in, int Fc, int ldc, float* dL_dgeo_feature,
                                          float* dL_dcolor_feature, void* stream);
PINGS_API size_t pings_spawn_plan_scratch_bytes(int64_t num_gaussians);
/* dest[n*k]: compacted row of every Gaussian or -1 if dropped; *count (device int32) = kept Gaussians.
 * dist_ratio[n] (nullable) = view_dist / z_far when dist_adaptive_scale (:657-659). */
PINGS_API int pings_spawn_plan(const pings_spawn_params* p, const float* alpha_raw, const float* scale_raw,
                               const float* dist_ratio, void* scratch, int32_t* dest, int32_t* count,
                               void* stream);
/* dest NULL = no compaction.  Outputs: gaussian_xyz[count,3], gaussian_scale[count, surfel ? 3 : scale_dim],
 * gaussian_rot[count,4] (wxyz), gaussian_alpha[count,1], gaussian_color[count,3], alpha_all[n*k,1]
 * (pre-filter, :721), gaussian_free_mask[count] (nullable; Gaussian g takes free_in[g % n], the reference's
 * tiling at :724). */
PINGS_API int pings_spawn_forward(const pings_spawn_params* p, const float* xyz_raw, const float* rot_raw,
                                  const float* scale_raw, const float* alpha_raw, const float* color_raw,
                                  const float* pos, const float* quat, const float* base_color,
                                  const float* dist_ratio, const uint8_t* free_in, const int32_t* dest,
                                  float* gaussian_xyz, float* gaussian_scale, float* gaussian_rot,
                                  float* gaussian_alpha, float* gaussian_color, float* alpha_all,
                                  uint8_t* gaussian_free_mask, void* stream);
/* Any dL_d<output> may be NULL (= zero).  Gradients w.r.t. the raw MLP outputs, same shapes as the inputs. */
PINGS_API int pings_spawn_backward(const pings_spawn_params* p, const float* xyz_raw, const float* rot_raw,
                                   const float* scale_raw, const float* alpha_raw, const float* color_raw,
                                   const float* quat, const float* base_color, const float* dist_ratio,
                                   const int32_t* dest, const float* dL_dxyz, const float* dL_dscale,
                                   const float* dL_drot, const float* dL_dalpha, const float* dL_dcolor,
                                   const float* dL_dalpha_all, float* dL_dxyz_raw, float* dL_drot_raw,
                                   float* dL_dscale_raw, float* dL_dalpha_raw, float* dL_dcolor_raw,
                                   void* stream);

/* ------------------------------------------------- neural-point map maintenance
 * Replaces the per-frame torch bookkeeping of `NeuralPoints`:
 *   voxel_down_sample_torch   utils/tools.py:924-967
 *   NeuralPoints.update       model/neural_gaussians.py:214-375 (everything but the feature initialisation)
 *   reset_local_map           model/neural_gaussians.py:378-478
 *   assign_local_to_global    model/neural_gaussians.py:482-494
 * Indices, masks, timestamps and table entries are bit-exact with the reference (oracle/map_cpu.py, G8 vectors).
 * Where the reference's index_put_ meets duplicate targets the LAST sample wins (its CPU semantics), here
 * deterministically.  Map arrays are caller-owned with room for the appended rows (capacity >= num_points + M).
 */
PINGS_API size_t pings_voxel_downsample_scratch_bytes(int64_t N);
/* sample_idx[<= N] (int64): index of the point closest to its voxel centre, one per occupied voxel, ordered by the
 * reference's linear voxel id; *count (HOST) = number of voxels.  Synchronises `stream` once. */
PINGS_API int pings_voxel_downsample(const float* points, int64_t N, float voxel_size, void* scratch,
                                     int64_t* sample_idx, int64_t* count, void* stream);
/* `voxel_down_sample_min_value_torch(points, voxel_size, value)` (utils/tools.py:970-1009): per occupied voxel the
 * point with the smallest `value` (1000 bins of value / max(value), ties by index); value NULL = the distance to the
 * voxel centre (pings_voxel_downsample).  Same output order, same single synchronisation. */
PINGS_API int pings_voxel_downsample_min_value(const float* points, const float* value, int64_t N, float voxel_size,
                                               void* scratch, int64_t* sample_idx, int64_t* count, void* stream);
/* Loop-closure maintenance of the map (model/neural_gaussians.py:871-1010):
 *   pings_map_prune_mask  prune[i] = |travel[cur_ts] - travel[ts_update[i]]| > diff_travel && certainty[i] < threshold
 *                         (:873-880; the caller counts, compacts the rows with pings_gather_rows and rebuilds the hash)
 *   pings_map_adjust      in place: p <- R p + t, q <- quat(R) (x) q with pose_diff[ts] (ts = create, or the mid
 *                         timestamp when use_mid_ts; :911-937); pose_diff is [num_poses, 4, 4] row-major, float64 when
 *                         pose_is_f64 (the quaternion part is then evaluated in float64 and cast, as the reference's
 *                         type promotion does) else float32
 *   pings_map_rehash      table[:] = -1; table[hash(points[v_j])] = v_j with v_j = sample_idx[j] (NULL: j) for
 *                         j < M, duplicates: the last j wins (:949-1000); slot_scratch: M int64
 * Timestamps index travel_dist[num_travel] / pose_diff[num_poses] with python semantics (negative wraps); one outside
 * [-T, T) is an IndexError in the reference: the kernels never read out of bounds — they set bit 0 of the device
 * word `out_of_range` (nullable; the caller zeroes it and reads it with its next read-back) and keep / do not move
 * that point.  cur_ts outside [0, num_travel) is PINGS_ERR_ARG. */
PINGS_API int pings_map_prune_mask(int64_t N, const float* travel_dist, int64_t num_travel, int32_t cur_ts,
                                   const int32_t* point_ts_update, const float* point_certainties,
                                   float diff_travel_dist_local, float prune_certainty_thre, uint8_t* prune_mask,
                                   int32_t* out_of_range, void* stream);
PINGS_API int pings_map_adjust(int64_t N, float* neural_points, float* point_orientations, const int32_t* point_ts_create,
                               const int32_t* point_ts_update, int32_t use_mid_ts, const void* pose_diff,
                               int32_t pose_is_f64, int64_t num_poses, int32_t* out_of_range, void* stream);
PINGS_API int pings_map_rehash(const float* neural_points, const int64_t* sample_idx, int64_t M, float resolution,
                               int64_t buffer_size, int64_t* table, int64_t* slot_scratch, void* stream);
PINGS_API size_t pings_map_update_scratch_bytes(int64_t M, int64_t num_points);
/* Inserts the M voxel representatives.  table[buffer_size] int64; travel_dist NULL = no travel-distance window
 * (temporal_local_map_on False); sample_colors / point_colors nullable together.  update_mask[M] (uint8, nullable)
 * <- 1 where the sample became a new neural point; *num_new (HOST).  Appends rows num_points .. num_points+num_new-1
 * of every map array (identity orientation, ts = cur_ts, certainty 0, free = !is_reliable, valid = 1, colour +
 * colour validity) and refreshes the colour of existing points whose colour was invalid.  Synchronises once.
 * resolution is the caller's double: the grid and the hash use it rounded to fp32, the new-point threshold is
 * fp32(3 * resolution^2) formed in double, the one rounding of the reference's `d2 > 3 * res ** 2`. */
PINGS_API int pings_map_update(const float* sample_points, const float* sample_colors, int64_t M, double resolution,
                               int64_t buffer_size, int64_t* table, int64_t num_points, const float* travel_dist,
                               int cur_ts, float diff_travel_dist_local, int is_reliable, float* neural_points,
                               float* point_orientations, int32_t* point_ts_create, int32_t* point_ts_update,
                               float* point_certainties, uint8_t* free_gs_mask, uint8_t* valid_gs_mask,
                               float* point_colors, uint8_t* valid_color_mask, void* scratch, uint8_t* update_mask,
                               int64_t* num_new, void* stream);
PINGS_API size_t pings_map_reset_local_scratch_bytes(int64_t num_points);
/* local_mask / sorrounding_mask [num_points+1] (uint8, last = 1), global2local[num_points+1] (int64: rank for local
 * points, 1 for the others — the reference's full_like(bool,-1) — and -1 for the padding entry),
 * local_idx[num_points+1] (int64: the local rows in order, followed by the padding row num_points),
 * *num_local (HOST).  sensor_position: DEVICE [3].  Synchronises once.  The radii are the caller's doubles: the
 * squared distances are compared with fp32(radius^2) formed in double (`d2 < radius ** 2` in the reference). */
PINGS_API int pings_map_reset_local(int64_t num_points, const float* neural_points, const int32_t* point_ts_create,
                                    const int32_t* point_ts_update, const float* travel_dist, int cur_ts,
                                    int use_mid_ts, int use_travel_dist, float diff_travel_dist_local,
                                    int diff_ts_local, const float* sensor_position, int range_filter_2d,
                                    double local_radius, double sorrounding_radius, void* scratch, uint8_t* local_mask,
                                    uint8_t* sorrounding_mask, int64_t* global2local, int64_t* local_idx,
                                    int64_t* num_local, void* stream);
/* `NeuralPoints.gather_local_data` (model/neural_gaussians.py:1135-1173) indexes nine per-point tensors with the
 * boolean surrounding mask, one nonzero + host synchronisation each in torch.  Here:
 *   pings_mask_rows         rows[<= n] (int64, ascending) = the indices where mask[i] != 0; count_and_last (HOST, two
 *                           int64): their number and mask[n - 1] (the feature tables carry a padding row that the
 *                           per-point tensors do not: :1159-1161).  Synchronises `stream` once (polled read-back).
 *   pings_gather_rows_multi dst_g[i] = src_g[idx[i]] for i < rows_g, all tensors g in ONE launch (any row width). */
typedef struct pings_gather_job {
  const void* src;
  void* dst;
  int64_t row_bytes;
  int64_t rows;
} pings_gather_job;
PINGS_API size_t pings_mask_rows_scratch_bytes(int64_t n);
PINGS_API int pings_mask_rows(const uint8_t* mask, int64_t n, void* scratch, int64_t* rows, int64_t* count_and_last,
                              void* stream);
PINGS_API int pings_gather_rows_multi(const pings_gather_job* jobs, int njobs, const int64_t* idx, void* stream);
/* dst[i] = src[idx[i]] / dst[idx[i]] = src[i] for rows of row_bytes bytes (any dtype). */
PINGS_API int pings_gather_rows(const void* src, int64_t row_bytes, const int64_t* idx, int64_t n, void* dst,
                                void* stream);
PINGS_API int pings_scatter_rows(const void* src, int64_t row_bytes, const int64_t* idx, int64_t n, void* dst,
                                 void* stream);

/* ------------------------------------------------------------ depth2normal
 * Replaces `depth2normal(depth, mask, camera, img_scale)` (gaussian_splatting/utils/point_utils.py:83-149) as `render`
 * uses it (gaussian_renderer/__init__.py:330-335), with the multiplication by the detached rendered alpha fused in:
 *   normal[3,H,W] = normalize(sum of the four neighbour cross products of the un-projected depth) * mask * alpha.
 * Visibility: `mask[H,W]` (uint8) if given, else `alpha > min_alpha`; `alpha` NULL = no weighting.  cx, cy, fx, fy are
 * the principal point / focal lengths in pixels of the (down-scaled) image.  Gradient flows to the depth only (mask
 * and alpha are detached in the reference). */
PINGS_API int pings_depth2normal_forward(const float* depth, const float* alpha, const uint8_t* mask, int H, int W,
                                         float cx, float cy, float fx, float fy, float min_alpha, float* normal,
                                         void* stream);
PINGS_API size_t pings_depth2normal_backward_scratch_bytes(int H, int W);
PINGS_API int pings_depth2normal_backward(const float* depth, const float* alpha, const uint8_t* mask, int H, int W,
                                          float cx, float cy, float fx, float fy, float min_alpha,
                                          const float* dL_dnormal, void* scratch, float* dL_ddepth, void* stream);

/* ------------------------------------------------------------ image-space losses
 * Replaces the photometric loss block of `Mapper.joint_gsdf_mapping` (utils/mapper.py:1197-1295; helpers
 * `l1_loss` / `sky_mask_loss`, gaussian_splatting/utils/loss_utils.py:17,178) — one fused pass per direction:
 *   losses[0] = |rgb - gt_rgb|.mean() over rows [v_min, v_max)                                   (:1224-1239)
 *   losses[1] = mean over (depth_min < gt_depth < depth_max) & (alpha > min_accu_alpha) of |gt - d|, or of
 *               |1/gt - 1/d| when inverse_depth                                                    (:1251-1267)
 *   losses[2] = mean over (|n| > 0) & (|m| > 0) of |m||n| - <n, m>, n = rendered normal, m = depth normal, both
 *               zeroed at sky pixels first; norms detached; consist_mode 1 detaches n, 2 detaches m (:1213-1216,1273-1295)
 *   losses[3] = alpha[sky].mean()                                                                  (:1198-1210)
 * All un-weighted (the lambdas stay with the caller).  Planes are [C,H,W] fp32, sky_mask [H,W] uint8; depth/gt_depth,
 * alpha, normal/depth_normal and sky_mask are optional (NULL); a mean over nothing is NaN as in torch.  `sums[8]`
 * (fp64: sum, count per loss) is kept for the backward pass, which takes dL/dlosses[4] from device memory and writes
 * whichever gradient planes are non-NULL. */
typedef struct {
  int H, W;
  int v_min, v_max;          /* rows of the colour loss, v_max exclusive (python slice already resolved) */
  float depth_min, depth_max, min_accu_alpha;
  int inverse_depth;
  int consist_mode;          /* 0 both sides learn, 1 gs_consist_normal_fixed, 2 gs_consist_depth_fixed */
} pings_image_loss_params;
PINGS_API size_t pings_image_losses_scratch_bytes(void);
PINGS_API int pings_image_losses_forward(const pings_image_loss_params* p, const float* rgb, const float* gt_rgb,
                                         const float* depth, const float* gt_depth, const float* alpha,
                                         const float* normal, const float* depth_normal, const uint8_t* sky_mask,
                                         void* scratch, double* sums, float* losses, void* stream);
PINGS_API int pings_image_losses_backward(const pings_image_loss_params* p, const float* rgb, const float* gt_rgb,
                                          const float* depth, const float* gt_depth, const float* alpha,
                                          const float* normal, const float* depth_normal, const uint8_t* sky_mask,
                                          const double* sums, const float* dL_dlosses, float* dL_drgb,
                                          float* dL_ddepth, float* dL_dalpha, float* dL_dnormal,
                                          float* dL_ddepth_normal, void* stream);

/* ------------------------------------------------------ colour / semantic heads of a kNN query
 * `Mesher.query_points` (utils/mesher.py:132-153) and the tracker's colour query (utils/tracker.py:322-331) apply an
 * activation to every neighbour's decoder output raw[B, k, C] and sum over the k neighbours with the IDW weights
 * weight[B, k] (NULL = `weighted_first`: k = 1, weight one):
 *   PINGS_HEAD_COLOR     out_value[B, C] = sum_j w_j sigmoid(raw_j)              (Decoder.regress_color, decoder.py:133-134)
 *   PINGS_HEAD_SEMANTIC  out_label[B] = argmax_c sum_j w_j log_softmax(raw_j)[c], first maximum as torch.argmax
 *                        (Decoder.sem_label_prob, decoder.py:119-122); out_value (nullable) receives the [B, C] sums
 * PINGS_HEAD_SEMANTIC needs k <= 16 (PINGS_ERR_ARG otherwise); PINGS_HEAD_COLOR takes any k >= 1.  One streaming pass instead of three to five torch passes per head. */
#define PINGS_HEAD_COLOR 0
#define PINGS_HEAD_SEMANTIC 1
PINGS_API int pings_head_reduce(const float* raw, const float* weight, int64_t B, int32_t k, int32_t C, int32_t mode,
                                float* out_value, int64_t* out_label, void* stream);

/* ------------------------------------------------------ tracker registration
 * Replaces the Jacobian assembly of `implicit_reg` (utils/tracker.py:608-689): with J_i = [p_i x g_i, g_i] (rotation
 * first, then translation),  N = sum_i w_i J_i^T J_i  (6x6)  and  g = -sum_i w_i r_i J_i  (6).
 * points[n,3], sdf_grad[n,3], sdf_residual[n], weight[n] -> out[42] = N row-major (36) followed by g (6), fp32,
 * accumulated in fp64 with a fixed-order two-stage reduction (bitwise reproducible). */
PINGS_API size_t pings_reg_normal_equations_scratch_bytes(void);
PINGS_API int pings_reg_normal_equations(const float* points, const float* sdf_grad, const float* sdf_residual,
                                         const float* weight, int64_t n, void* scratch, float* out, void* stream);
/* The rest of the step (utils/tracker.py:649-689, :774-783) from the 42 floats above: N += lm_lambda diag(N) in fp32,
 * t = N^-1 g in fp64 (Gaussian elimination with partial pivoting), T[4,4] = [expmap(t[:3]) | t[3:]] row-major fp64;
 * t_out[6] optional.  One tiny kernel instead of ~30 torch launches and the host sync of linalg.inv. */
PINGS_API int pings_reg_solve(const float* normal_eq, float lm_lambda, double* T_out, double* t_out, void* stream);
/* The same step with a conditioning report.  The reference's `torch.linalg.inv` (utils/tracker.py:668) raises on a
 * singular N; the kernel above cannot raise, so it leaves a bit mask in the device word `status_dev`:
 *   PINGS_REG_SINGULAR         a pivot of the damped matrix is exactly 0 or not finite (the case the reference raises on)
 *   PINGS_REG_ILL_CONDITIONED  smallest |pivot| < 1e-7 x largest |entry|: the step is rounding noise (N arrives in fp32)
 *   PINGS_REG_NONFINITE        t or T came out Inf / NaN
 * `status_host` (optional, host memory): the call waits for the kernel with a polled read-back and copies the word —
 * the one synchronisation the reference has at this line as well. */
#define PINGS_REG_SINGULAR 1
#define PINGS_REG_ILL_CONDITIONED 2
#define PINGS_REG_NONFINITE 4
PINGS_API int pings_reg_solve_checked(const float* normal_eq, float lm_lambda, double* T_out, double* t_out,
                                      int32_t* status_dev, int32_t* status_host, void* stream);

/* ------------------------------------------------------ device-resident odometry loop (csrc/tracker.hip)
 * One iteration of `Tracker.tracking` / `registration_step` (utils/tracker.py:43-210, 353-605) with the pose on the
 * device and one small record read back per iteration (pings_amd/tracker_ops.py: tracking).
 *   transform   cur = T p for the n source points; T is the fp64 pose in device memory, cast to fp32 and applied in
 *               fp32 as utils/tools.py:888-900
 *   assemble    validity (mask, min_grad < |g| < max_grad, std < max_std), residual (sdf - label, or sdf / |g| - label),
 *               Geman-McClure and normal weights; fp64 per-block sums of the 21 + 6 normal-equation entries, the valid
 *               count, sum w, sum |r| and sum w r^2 (invalid points weighted out, nothing compacted); optional valid[n]
 *   step        one workgroup: the per-block sums in block order; fewer than 10 valid points -> identity step and
 *               residual 0; else N, g scaled by n / (2 sum w) when `PINGS_REG_F_WEIGHTED` (the reference's w /= 2 mean w),
 *               LM damping, fp64 solve and exponential map (as pings_reg_solve_checked); T <- dT T in fp64;
 *               record[8] = valid count, status bits (PINGS_REG_*), then three doubles: residual mean in cm, rotation
 *               acos((tr dT - 1) / 2) in degrees (NaN kept), translation |dt| in metres; trace row `iter` (optional,
 *               24 doubles: count, residual, rotation, translation, status, sum w, sum w r^2, 0, dT[16])
 * The caller owns every buffer; no launch allocates, copies or waits. */
#define PINGS_REG_F_NORMALS 1      /* normals[n,3] given: w *= 0.5 + |n . g / (|g| + 1e-7)|                          */
#define PINGS_REG_F_DIV_GRAD 2     /* reg_dist_div_grad_norm: residual = sdf / |g| - label                          */
#define PINGS_REG_F_WEIGHTED 4     /* w is a tensor in the reference (any weight on): normalise by 2 mean(w)         */
typedef struct pings_reg_loop_args {
  int64_t n;                     /* source points                                                                  */
  int32_t flags, iter, trace_cap;   /* PINGS_REG_F_*; trace row of this step; rows in trace                        */
  float min_grad, max_grad, max_std;   /* validity window on |g|; bound on the SDF spread                         */
  float gm_dist, gm_grad;        /* Geman-McClure scales of residual / gradient anomaly (<= 0: off)               */
  float lm_lambda;               /* LM damping                                                                     */
  const float* src;              /* [n,3] source points (transform)                                               */
  float* cur;                    /* [n,3] transformed points (transform output, assemble input)                   */
  const float* sdf;              /* [n]                                                                            */
  const float* grad;             /* [n,3] d sdf / dx                                                               */
  const float* std;              /* [n] spread of the per-neighbour predictions                                   */
  const uint8_t* mask;           /* [n] registration mask (bool)                                                  */
  const float* label;            /* [n] SDF labels                                                                 */
  const float* normals;          /* [n,3] or NULL                                                                  */
  uint8_t* valid;                /* [n] validity out, or NULL                                                      */
  double* part;                  /* [pings_reg_partials(n) * 32] per-block sums                                    */
  double* T;                     /* [16] pose, row-major, updated in place by step                                 */
  double* delta;                 /* [16] dT of the step                                                            */
  int32_t* record;               /* [8] device record of the step                                                  */
  double* trace;                 /* [trace_cap * 24] or NULL                                                       */
} pings_reg_loop_args;
PINGS_API int pings_reg_partials(int64_t n);
PINGS_API int pings_reg_transform(const pings_reg_loop_args* a, void* stream);
PINGS_API int pings_reg_assemble(const pings_reg_loop_args* a, void* stream);
PINGS_API int pings_reg_step(const pings_reg_loop_args* a, void* stream);
/* `assemble` with the tracker's colour terms (utils/tracker.py:485-535, :692-737), for the configurations with
 * color_on and photometric_loss_on or consist_wieght_on.  Writes the same `part` layout as pings_reg_assemble, so
 * pings_reg_step runs behind it unchanged: the reference sums the geometric and the photometric system before damping.
 * Intensity I = the one channel, or 0.144 c0 + 0.299 c1 + 0.587 c2 of three (utils/tools.py:723), of source colour,
 * prediction and Jacobian rows alike.
 *   PINGS_REG_COLOR_PHOTO    N += w photo_weight J_c^T J_c, g -= w photo_weight r_c J_c with r_c = I_pred - I_src and
 *                            J_c = [p x grad I, grad I]; the weight is the geometric one
 *   PINGS_REG_COLOR_CONSIST  w *= exp(-|I_src - I_pred|); color_jac is not read
 * Validity is the SDF's alone; the colours of an invalid point are not read.  photo_part[block] = sum |I_pred - I_src|
 * over the block's valid points.  Set PINGS_REG_F_WEIGHTED in a->flags: the reference's w is a tensor on this path. */
#define PINGS_REG_COLOR_PHOTO 1
#define PINGS_REG_COLOR_CONSIST 2
typedef struct pings_reg_color_args {
  const float* src_color;        /* [n,channels] measured colours                                                  */
  const float* color_pred;       /* [n,channels] pings_color_forward                                               */
  const float* color_jac;        /* [n,channels,3] d colour / d point, or NULL (CONSIST)                           */
  int32_t channels;              /* 1 or 3                                                                         */
  int32_t mode;                  /* PINGS_REG_COLOR_*                                                              */
  float photo_weight;            /* config.photometric_loss_weight                                                 */
  double* photo_part;            /* [pings_reg_partials(n)] per-block sum |r_c|                                    */
} pings_reg_color_args;
PINGS_API int pings_reg_assemble_color(const pings_reg_loop_args* a, const pings_reg_color_args* c, void* stream);
/* The one host read of an iteration: the 8 record words behind everything queued on `stream`, by the polled
 * read-back the other checked entry points use (not a launch function: it returns when the words have arrived). */
PINGS_API int pings_reg_read_record(const int32_t* record_dev, int32_t* record_host, void* stream);

/* ------------------------------------------------------ Gaussian-space loss block (csrc/gauss_loss.hip)
 * The mapper's opacity, opacity-entropy, isotropy, area, SDF-consistency, SDF-normal-consistency and invalid-opacity
 * terms (utils/mapper.py:1331-1483) with every count on the device.  One argument block for all entry points; the
 * caller owns every buffer (pings_amd/gaussian_losses.py carves them from one allocation per direction).  Rows past
 * the device sample count S (meta[1]) exist in the capacity-sized buffers and are never read as live.
 *   select     constraint mask, opacity sums, a uniform sample of S = min(count, cap) constrained Gaussians (0 when
 *              count <= 10) as idx[0..S) in ascending index order, or the injected indices
 *   prepare    normals, the (1+R)*cap query rows (unshifted block first) and their labels
 *   (the caller runs pings_sdf_forward on the query rows into sdf / grad / nn and the neighbour lists)
 *   reduce     valid mask and the seven losses; counts[5] = #alpha_all < min_alpha, constraint count, S, valid rows,
 *              invalid samples (float64, exact integers)
 *   backward_rows     d sdf, d dS/dx and d normal per query row from the upstream g[7]
 *   (the caller runs pings_sdf_backward / pings_sdf_double_backward and pings_sdf_hvp_x into dq)
 *   backward_scatter  dense d_xyz / d_rot / d_scale / d_alpha (zeroed by the caller) and d_alpha_all
 * flags: 1 opacity, 2 opacity entropy, 4 isotropy, 8 area, 16 SDF terms. */
typedef struct pings_gauss_loss_args {
  int64_t P, Na, cap;            /* local Gaussians, alpha_all elements, sample capacity (bs * gaussian_bs_ratio) */
  int32_t R, ncols, scale_cols;  /* shift count; scale columns used (2 | 3); row stride of gaussian_scale         */
  int32_t flags;
  float min_alpha, contrib_thr, shift_range, grad_min, grad_max, inv_voxel_pow;
  int64_t n_inject;              /* -1: draw from seed; else the number of injected indices                       */
  const float* alpha_all;        /* [Na]                                                                          */
  const uint8_t* visible;        /* [P] local visibility                                                          */
  const float* contrib;          /* [P] or NULL                                                                   */
  const uint8_t* free_mask;      /* [P] or NULL                                                                   */
  const float *xyz, *rot, *scale, *alpha;   /* [P,3] [P,4] [P,scale_cols] [P]                                     */
  const int64_t* seed;           /* device word: key seed                                                         */
  const int64_t* inject_idx;     /* [n_inject] distinct indices, or NULL                                          */
  const float* randn;            /* [R, cap] standard normal draws                                                */
  uint32_t* keys;                /* [P]                                                                           */
  double* part;                  /* [256 * 4]                                                                     */
  int32_t* meta;                 /* [8]: count, S, n below min_alpha, n valid, n invalid                           */
  int32_t* idx;                  /* [cap]                                                                         */
  float *normal, *queries, *label;          /* [cap,3] [(1+R)cap,3] [(1+R)cap]                                    */
  float *sdf, *grad;             /* [(1+R)cap] [(1+R)cap,3]   (pings_sdf_forward outputs)                          */
  int64_t* nn;                   /* [(1+R)cap]                                                                    */
  uint8_t* valid;                /* [(1+R)cap]                                                                    */
  float* losses;                 /* [7]                                                                           */
  double* counts;                /* [5]                                                                           */
  const float* g;                /* [7] upstream gradient of the losses                                           */
  float *ds, *v, *dn, *dq;       /* [(1+R)cap] [(1+R)cap,3] x3                                                    */
  float *d_xyz, *d_rot, *d_scale, *d_alpha, *d_alpha_all;
} pings_gauss_loss_args;
PINGS_API int pings_gauss_loss_select(const pings_gauss_loss_args* a, void* stream);
PINGS_API int pings_gauss_loss_prepare(const pings_gauss_loss_args* a, void* stream);
PINGS_API int pings_gauss_loss_reduce(const pings_gauss_loss_args* a, void* stream);
PINGS_API int pings_gauss_loss_backward_rows(const pings_gauss_loss_args* a, void* stream);
PINGS_API int pings_gauss_loss_backward_scatter(const pings_gauss_loss_args* a, void* stream);

/* Query gradient of the fused SDF's second order: out[b] = grad_x[b] * ds[b] + H_S(x_b) v[b] for the per-neighbour
 * decoder (weighted_first = 0), with the neighbour lists of pings_sdf_forward (idx, gidx).  H_S is the Hessian of
 * S(x) = sum_m w_m(x) scale MLP([f_m, R_m^T (x - p_m)]) with relu'' = 0.  grad_x / ds may be NULL (term omitted). */
typedef struct pings_sdf_hvp_args {
  const float *W1, *b1, *W2, *b2;
  int32_t H, F;
  float scale;
  int32_t after_pgo;
  const float *features, *points, *orientations, *gpoints;
  const float* queries;
  int64_t B;
  int32_t nnk;
  const int64_t *idx, *gidx;
  const float *v, *ds, *grad_x;
  float* out;
} pings_sdf_hvp_args;
PINGS_API int pings_sdf_hvp_x(const pings_sdf_hvp_args* a, void* stream);

/* ------------------------------------------------------ SDF-sample loss block (csrc/sdf_loss.hip)
 * The mapper's BCE, Eikonal and colour terms over one SDF sample batch (utils/mapper.py:836-930, 1493-1544) with the
 * two subset counts on the device.  One argument block for all entry points; the caller owns every buffer
 * (pings_amd/sdf_losses.py).  Sizes depend on B and d only: the Eikonal rows live in a capacity cap = ceil(B/d)
 * buffer whose rows past the device count meta[0] are padding (idx -1, query = coord[0]) and get zero gradient.
 *   select     Eikonal mask |label| < eik_band, the stable rank of each masked row, rows of rank % d == 0 compacted
 *              in row order into idx / xsel; meta[0] = ceil(M/d)
 *   (the caller runs the central-difference gradient on the cap rows of xsel into g)
 *   reduce     IDW sums (unless weighted_first), sdf_pred, colour sigmoid and mask, fixed-order fp64 sums; losses[3] =
 *              BCE, Eikonal, colour (NaN for an empty subset, 0 for a disabled term); counts[2] = Eikonal rows, colour
 *              rows (float64, exact integers); meta[1] = colour rows
 *   backward   d s [B,k] (or [B]), d g [cap,3] (zero on padding), d c [B,k,C] (or [B,C]; zero off the colour mask)
 * flags: 1 Eikonal, 2 colour, 4 colour weighted by |weight|, 8 BCE weighted by |weight|, 16 weighted_first. */
typedef struct pings_sdf_loss_args {
  int64_t B, cap;                /* batch rows; Eikonal capacity ceil(B/d)                                          */
  int32_t k, C, d, flags;        /* neighbours, colour channels, gradient decimation                                */
  float sigma, eik_band, col_band;   /* sdf_scale; free_sample_end_dist_m; 0.5 * surface_sample_range_m          */
  const float* coord;            /* [B,3]                                                                         */
  const float* label;            /* [B]                                                                           */
  const float* weight;           /* [B] (read as |weight|) or NULL when no term is weighted                       */
  const float* color_label;      /* [B,C]                                                                         */
  const float* w;                /* [B,k] IDW weights                                                             */
  const float* s;                /* [B,k] decoder SDF per neighbour, [B] when weighted_first                      */
  const float* c;                /* [B,k,C] colour decoder output (pre-sigmoid), [B,C] when weighted_first        */
  const float* g;                /* [cap,3] finite-difference gradient of the xsel rows                           */
  int32_t* idx;                  /* [cap] compacted Eikonal rows, -1 on padding                                   */
  float* xsel;                   /* [cap,3]                                                                       */
  int32_t* meta;                 /* [2]: Eikonal rows, colour rows                                                */
  double* part;                  /* [pings_sdf_loss_partials(B, cap) * 4] per-block sums                          */
  float* sdf_pred;               /* [B]                                                                           */
  float* losses;                 /* [3]                                                                           */
  double* counts;                /* [2]                                                                           */
  const float* gl;               /* [3] upstream gradient of the losses                                           */
  const float* g_pred;           /* [B] upstream gradient of sdf_pred, or NULL                                    */
  float *d_s, *d_g, *d_c;        /* shapes of s, g, c                                                             */
} pings_sdf_loss_args;
PINGS_API int pings_sdf_loss_select(const pings_sdf_loss_args* a, void* stream);
PINGS_API int pings_sdf_loss_reduce(const pings_sdf_loss_args* a, void* stream);
PINGS_API int pings_sdf_loss_backward(const pings_sdf_loss_args* a, void* stream);
/* Number of per-block partials the reduce writes (part holds 4 doubles each). */
PINGS_API int pings_sdf_loss_partials(int64_t B, int64_t cap);

/* ------------------------------------------------------ semantic loss block (csrc/sem_loss.hip)
 * The mapper's semantic term over one SDF sample batch (utils/mapper.py:863-866, 929-946) with the selection on the
 * device (pings_amd/semantic_losses.py).  Row b is labelled iff label[b] > 0 (>= 0 with the free-space flag) and
 * label[b] < S; a label >= S is counted in counts[1] and never indexes memory.  r_b is the number of labelled rows in
 * front of b; the row is selected iff it is labelled and r_b % d == 0, so n = ceil(M / d) rows of M labelled ones.
 *   forward    selected[B]; loss[0] = -(1/n) sum_selected sum_j w[b,j] log_softmax(raw[b,j,:])[label[b]] (NaN when
 *              n = 0); counts[2] = n, labels >= S (float64, exact integers).  fp64 sums in a fixed order.
 *   backward   d_raw = gl[0] / n * w[b,j] * (softmax(raw[b,j,:]) - onehot(label[b])) on selected rows and exactly 0
 *              on every other row, with the selected[] and scratch of the forward call on the same inputs.
 * Limits: 1 <= S <= 32, 1 <= k <= 16, d >= 1; anything else is status 1.  Launch sizes depend on B, k, S and d only.
 * flags: 1 weighted_first (raw is [B,S], k = 1, w unused), 2 free-space labels are labelled, 4 labels are int64. */
typedef struct pings_sem_loss_args {
  int64_t B;                     /* batch rows                                                                    */
  int32_t k, S, d, flags;        /* neighbours, classes, sem_label_decimation                                     */
  const float* raw;              /* [B,k,S] semantic decoder output, [B,S] when weighted_first                    */
  const float* w;                /* [B,k] IDW weights, or NULL when weighted_first                                */
  const void* label;             /* [B] int32, or int64 with flag 4                                               */
  uint8_t* selected;             /* [B] 1 on the selected rows                                                    */
  void* scratch;                 /* pings_sem_loss_scratch_bytes(B) bytes, 8-byte aligned                         */
  float* loss;                   /* [1]                                                                           */
  double* counts;                /* [2]                                                                           */
  const float* gl;               /* [1] upstream gradient of the loss                                             */
  float* d_raw;                  /* shape of raw                                                                  */
} pings_sem_loss_args;
PINGS_API size_t pings_sem_loss_scratch_bytes(int64_t B);   /* 0 for a bad B */
PINGS_API int pings_sem_loss_forward(const pings_sem_loss_args* a, void* stream);
PINGS_API int pings_sem_loss_backward(const pings_sem_loss_args* a, void* stream);

/* ------------------------------------------------------ marching cubes (csrc/mc.hip)
 * The surface `v = level` of a C-contiguous [nx, ny, nz] fp32 volume (point (i, j, k) at (i*ny + j)*nz + k), by the
 * rules of DESIGN §2.7: cell (i, j, k) is processed iff mask[i, j, k] != 0 (mask NULL: every cell) and its 8 corners
 * are finite; vertices in index units, ascending key 4 p + slot (slot 0 the grid point p, 1..3 its +x, +y, +z edge);
 * faces int64 vertex indices in ascending cell order.  Two phases with one host read between them:
 *   count   per-block counts, scans and totals[2] (HOST): vertices, faces
 *   emit    keys[nv] (int64 workspace), verts[nv, 3], faces[nf, 3] with the nv / nf of the count call on the same
 *           inputs and the same scratch (pings_mc_scratch_bytes: O(nx*ny*nz / 256) bytes; 0 for a bad shape). */
#define PINGS_MC_ALLOW_DEGENERATE 1   /* keep faces with a repeated vertex                                           */
#define PINGS_MC_ASCENT 2             /* gradient_direction 'ascent': right-hand normals toward increasing values     */
PINGS_API size_t pings_mc_scratch_bytes(int64_t nx, int64_t ny, int64_t nz);
PINGS_API int pings_mc_count(const float* vol, const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, float level,
                             int flags, void* scratch, int64_t* totals, void* stream);
PINGS_API int pings_mc_emit(const float* vol, const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, float level,
                            int flags, const void* scratch, int64_t nv, int64_t nf, int64_t* keys, float* verts,
                            int64_t* faces, void* stream);

/* ------------------------------------------------------ mesh finishing (csrc/mesh.hip)
 * What utils/mesher.py:500-530 does with Open3D after marching cubes, by the rules of DESIGN §2.7b.  verts fp32
 * [V, 3], faces int64 [F, 3]; indices are 32-bit inside the kernels, so V >= 2^31 or 3F >= 2^31 is status 1, not a
 * launch.  Every entry takes a scratch buffer of its `_scratch_bytes` (0 for a bad shape) and no output aliases an
 * input.  A face corner outside [0, V) never indexes memory: the entries with a host read return status 1 after it.
 * Integer atomics only; every output is the same bits on every run.
 *   weld      remove_duplicated_vertices.  Two vertices are the same iff their three coordinates compare equal
 *             (-0 == +0; a vertex with a non-finite coordinate equals nothing).  The kept vertex of a group is its first
 *             occurrence, kept vertices keep their order, faces are remapped and none is removed.  verts_out [V, 3] and
 *             kept [V] (the old index of every new vertex) are filled up to *n_out (HOST, the one read);
 *             remap [V]: new index of every old vertex; faces_out [F, 3] (F may be 0).
 *   clusters  cluster_connected_triangles.  Each face has the undirected edges (min, max) of its corner pairs, (a, a)
 *             included; faces that share an edge key are connected, faces that share only a vertex are not.  A cluster's
 *             id is the rank of its smallest face index among all clusters' smallest face indices.  labels [F],
 *             counts [F] filled up to the number of clusters, which goes to *n_clusters (HOST) when that is not NULL;
 *             with NULL there is no host read and the number stays in the scratch for drop_small.
 *   drop_small  remove_triangles_by_mask: keeps face f iff counts[labels[f]] >= min_tri, in order, into faces_out
 *             [F, 3].  `scratch` is the one the clusters call on the same faces used.  totals[2] (HOST, one read):
 *             clusters, kept faces.
 *   vertex_normals  compute_vertex_normals(normalized=True): per vertex the sum, in ascending face index and then
 *             corner order, of the unnormalised (v1 - v0) x (v2 - v0) of every corner that names it, divided by its
 *             length; (0, 0, 1) where the sum is zero or not finite.  fp32, no host read; a face with a corner outside
 *             [0, V) contributes nothing.
 *   compact_vertices  drops the vertices no face names (not in the reference).  verts_out, kept as in weld;
 *             remap [V] is -1 for a dropped vertex.  *n_out (HOST, one read). */
PINGS_API size_t pings_mesh_weld_scratch_bytes(int64_t V, int64_t F);
PINGS_API int pings_mesh_weld(const float* verts, int64_t V, const int64_t* faces, int64_t F, void* scratch,
                              float* verts_out, int64_t* faces_out, int64_t* remap, int64_t* kept, int64_t* n_out,
                              void* stream);
PINGS_API size_t pings_mesh_clusters_scratch_bytes(int64_t F);
PINGS_API int pings_mesh_clusters(const int64_t* faces, int64_t F, int64_t V, void* scratch, int64_t* labels,
                                  int64_t* counts, int64_t* n_clusters, void* stream);
PINGS_API size_t pings_mesh_drop_small_scratch_bytes(int64_t F);
PINGS_API int pings_mesh_drop_small(const int64_t* faces, int64_t F, const int64_t* labels, const int64_t* counts,
                                    int64_t min_tri, void* scratch, int64_t* faces_out, int64_t* totals, void* stream);
PINGS_API size_t pings_mesh_vertex_normals_scratch_bytes(int64_t V, int64_t F);
PINGS_API int pings_mesh_vertex_normals(const float* verts, int64_t V, const int64_t* faces, int64_t F, void* scratch,
                                        float* normals, void* stream);
PINGS_API size_t pings_mesh_compact_vertices_scratch_bytes(int64_t V, int64_t F);
PINGS_API int pings_mesh_compact_vertices(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                          void* scratch, float* verts_out, int64_t* faces_out, int64_t* remap,
                                          int64_t* kept, int64_t* n_out, void* stream);

/* ------------------------------------------------------ labelled meshes (csrc/mesh_label.hip)
 * What Mesher.estimate_vertices_sem (utils/mesher.py:393-412) does with its colour dict and Open3D.
 *   label_colors     colors[v] = table[labels[v]] / 255 (fp32, table uint8 [T, 3]), drop[v] = labels[v] <= 0.  A label
 *                    outside [0, T), or one with valid[label] == 0, gets colour 0, never indexes the table, and adds one
 *                    to *bad (DEVICE int32, zeroed by the caller; an integer atomic).  No host read.
 *   remove_vertices  remove_vertices_by_mask: the vertices with drop[v] != 0 go and every face naming one goes; kept
 *                    vertices and kept faces keep their order, faces are remapped.  verts_out [V, 3], kept [V] (the old
 *                    index of every new vertex) and faces_out [F, 3] are filled up to the counts; remap [V] is -1 for a
 *                    dropped vertex.  totals[3] (HOST, the one read): kept vertices, kept faces, *bad (0 with bad NULL).
 *                    A face corner outside [0, V) never indexes memory: status 1 after the read.
 * V and 3F stay below 2^31; scratch of `_scratch_bytes` (0 for a bad shape); no output aliases an input. */
PINGS_API int pings_mesh_label_colors(const int64_t* labels, int64_t V, const uint8_t* table, const uint8_t* valid,
                                      int64_t T, float* colors, uint8_t* drop, int32_t* bad, void* stream);
PINGS_API size_t pings_mesh_remove_vertices_scratch_bytes(int64_t V, int64_t F);
PINGS_API int pings_mesh_remove_vertices(const float* verts, int64_t V, const int64_t* faces, int64_t F,
                                         const uint8_t* drop, const int32_t* bad, void* scratch, float* verts_out,
                                         int64_t* faces_out, int64_t* remap, int64_t* kept, int64_t* totals,
                                         void* stream);

/* ------------------------------------------------------ mesh surface sampling (csrc/mesh_sample.hip)
 * N points on the surface of a mesh (verts [V, 3] fp32, faces [F, 3] int64), in proportion to triangle area, with an
 * optional box crop fused in: the cloud eval/eval_mesh_utils.py:eval_mesh scores.  Restated by tests/mesh_sample_ref.py;
 * bit-equal to it and the same from run to run.  The call only enqueues on `stream`: no allocation, copy or wait.
 *   area   A_t = 0.5 |(v1 - v0) x (v2 - v0)| in fp64.  With box != NULL (DEVICE double[6]: lo xyz, hi xyz) A_t = 0
 *          unless lo <= v <= hi holds for all three vertices on every axis, both ends inclusive, compared in fp64
 *          (Open3D's crop).  A corner index outside [0, V) gives A_t = 0 and PINGS_MESH_SAMPLE_INDEX in *status, a
 *          non-finite vertex A_t = 0 and PINGS_MESH_SAMPLE_NONFINITE.
 *   q_t    = llrint(A_t * 2^PINGS_MESH_SAMPLE_UNIT_BITS), an int64 count of quanta of 2^-32 m^2; Q_t its inclusive sum.
 *          A triangle with A_t * 2^32 > floor(2^PINGS_MESH_SAMPLE_SUM_BITS / F) gets q_t = 0 and
 *          PINGS_MESH_SAMPLE_AREA_CAP, so Q cannot overflow (4 M faces: 256 m^2 per triangle).
 *   owner  point i in [0, N) belongs to the first t with llrint((double)Q_t * (double)N / (double)Q_{F-1}) > i.
 *   point  z = splitmix64(seed + (i + 1) * 0x9E3779B97F4A7C15), u1 = (z >> 32) * 2^-32, u2 = (z & 0xffffffff) * 2^-32,
 *          s = sqrt(u1), p = ((1 - s) * v0 + s * (1 - u2) * v1) + s * u2 * v2 in fp64, rounded to fp32 once.
 * points [N, 3]; tri [N] (the owner, may be NULL); *count (DEVICE int64) = N, or 0 with Q_{F-1} == 0 (then nothing else
 * is written); *status (DEVICE int32, zeroed by the caller) is OR-ed into.  The status bits leave PINGS_EVAL_EXTENT and
 * PINGS_CAMFRONT_FULL free, so one word serves a whole evaluation.  V, F and N lie in [1, 2^31 - 1]. */
#define PINGS_MESH_SAMPLE_UNIT_BITS 32
#define PINGS_MESH_SAMPLE_SUM_BITS 62
#define PINGS_MESH_SAMPLE_INDEX 16
#define PINGS_MESH_SAMPLE_NONFINITE 32
#define PINGS_MESH_SAMPLE_AREA_CAP 64
PINGS_API size_t pings_mesh_sample_scratch_bytes(int64_t F);
PINGS_API int pings_mesh_sample(const float* verts, int64_t V, const int64_t* faces, int64_t F, const double* box,
                                int64_t N, int64_t seed, void* scratch, float* points, int32_t* tri, int64_t* count,
                                int32_t* status, void* stream);

/* ------------------------------------------------------ fused AdamW (csrc/optim.hip)
 * One optimiser step of every tensor of every parameter group in ONE launch.  A job is one fp32
 * tensor; its scalars are computed by the host in double and rounded to fp32 once, as torch's single-tensor AdamW
 * rounds them when it hands Python floats to fp32 tensor ops (torch/optim/adam.py `_single_tensor_adam`), t being the
 * tensor's OWN step count after this step:
 *   decay = 1 - lr*wd, one_minus_beta1 = 1 - beta1, one_minus_beta2 = 1 - beta2 (NOT 1.0f - (float)beta: that differs
 *   in the last bits of a number near 0.01), step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t).
 * Per element, in torch's operation order, IEEE division and square root, no contraction, no atomics:
 *   p *= decay;  m += (g - m)*one_minus_beta1;  v = v*beta2 + one_minus_beta2*g*g;
 *   p -= step_size*m / (sqrt(v)/bc2_sqrt + eps)
 * The job table travels by value as a kernel argument, PINGS_ADAMW_MAX_JOBS tensors per launch; more jobs are split
 * into ceil(njobs / PINGS_ADAMW_MAX_JOBS) launches (a launch whose jobs are all empty is not made), and launches_out
 * (HOST, may be NULL) receives the number made.  A workgroup takes (tensor, chunk) items of PINGS_ADAMW_CHUNK elements;
 * a tensor whose four pointers are 16-byte aligned moves as 16-byte words, any other 4-byte aligned one as scalars.
 * n == 0 jobs do nothing.  No copy, no allocation and no synchronisation: the call only enqueues on `stream`.
 * p, m and v of one job must not overlap each other, g, or another job's tensors. */
#define PINGS_ADAMW_MAX_JOBS 48
#define PINGS_ADAMW_CHUNK 4096
typedef struct pings_adamw_job {
  float* p;                      /* [n] parameter, updated in place                                               */
  const float* g;                /* [n] gradient                                                                  */
  float* m;                      /* [n] exp_avg, updated in place                                                 */
  float* v;                      /* [n] exp_avg_sq, updated in place                                              */
  int64_t n;
  float decay;
  float beta1;
  float beta2;
  float one_minus_beta1;
  float one_minus_beta2;
  float step_size;
  float bc2_sqrt;
  float eps;
} pings_adamw_job;
PINGS_API int pings_adamw_step(const pings_adamw_job* jobs, int njobs, int* launches_out, void* stream);

/* ------------------------------------------------------ view evaluation (csrc/eval.hip)
 * What Mapper.gs_eval_offline and eval/eval_mesh_utils.py compute per evaluated view.  Every call only enqueues on
 * `stream`: no allocation, no copy, no wait; results are device records the caller reads when it wants them.  A cloud
 * is a [cap, 3] fp32 buffer whose live length is `cap`, or *x_dev (DEVICE int64, clamped into [0, cap]) when that
 * pointer is not NULL, so a length produced by one call feeds the next without passing through the host.  Sizes are
 * limited to 2^31 - 1 rows; a *_scratch_bytes query returns 0 for a size no call accepts.
 *
 * view_metrics   one pass over rgb / gt [channels, hw] (1..4 channels) and, when depth != NULL, depth / gt_depth [hw]
 *   under the mask gt > depth_min && d > depth_min && gt < depth_max && d < depth_max (&& alpha > min_alpha with
 *   use_alpha).  record[PINGS_EVAL_VIEW_RECORD] doubles: mean over channels of 20 log10(1 / sqrt(mse_c)), *ssim (a
 *   DEVICE float, NaN when NULL), mean |dd|, sqrt(mean dd^2) (both NaN on an empty mask or without depth), the mask
 *   count, mse_0..mse_3 (NaN past `channels`).
 * backproject   pixel (u, v) of depth [height, width] gives a point iff 0 < d < depth_trunc (&& alpha > min_alpha):
 *   cam_to_world * ((u - cx) d / fx, (v - cy) d / fy, d, 1), in row-major pixel order; colors = floor(rgb * 255) / 255
 *   of rgb [3, hw] when rgb != NULL.  intrinsic (HOST) = fx, fy, cx, cy; cam_to_world (HOST) = the first three rows of
 *   the 4x4, row-major.  points / colors hold height*width rows; *count (DEVICE) receives the number written.
 * voxel_centroids   Open3D voxel_down_sample: cell floor((p - (min - voxel/2)) / voxel) per axis in fp64, out = the
 *   mean of each occupied cell's points in ascending cell key (x fastest), sums in fp64 in input order (no atomics:
 *   bitwise repeatable).  out holds n rows; *count (DEVICE) receives the number of cells.
 * nn_build / nn_query   exact nearest neighbour among dst below max_dist.  build files dst by cells of size `cell`
 *   relative to its lower bound into `scratch` (O(m) bytes); query (same scratch, m and cell; any number of times)
 *   writes dist[n] and idx[n]: +inf / -1 where no dst point lies at distance < max_dist, ties in fp32 distance to the
 *   smallest index, rows past the live length of src +inf / -1.  ceil(max_dist / cell) may not exceed 64.
 * A cloud whose extent exceeds 2^21 cells on an axis cannot be filed: the extent is known on the device only, so it
 * is reported by OR-ing PINGS_EVAL_EXTENT into *status (DEVICE int32, zeroed by the caller), and a query against such
 * a grid writes NaN / -2 in every row.
 * pair_reduce   record[PINGS_EVAL_PAIR_RECORD] doubles from the two distance lists: {kept, sum d, sum d^2, d <
 *   threshold} of dist_p without its +inf rows, the same four of dist_r with +inf rows counted as truncation_com,
 *   the live lengths np and nr, *status (0 when NULL), 0. */
#define PINGS_EVAL_VIEW_RECORD 9
#define PINGS_EVAL_PAIR_RECORD 12
#define PINGS_EVAL_EXTENT 1
PINGS_API size_t pings_eval_view_metrics_scratch_bytes(int64_t hw);
PINGS_API int pings_eval_view_metrics(const float* rgb, const float* gt, int channels, int64_t hw, const float* depth,
                                      const float* gt_depth, const float* alpha, float depth_min, float depth_max,
                                      float min_alpha, int use_alpha, const float* ssim, void* scratch, double* record,
                                      void* stream);
PINGS_API size_t pings_eval_backproject_scratch_bytes(int64_t hw);
PINGS_API int pings_eval_backproject(const float* depth, const float* rgb, const float* alpha, int height, int width,
                                     const double* intrinsic, const double* cam_to_world, double depth_trunc,
                                     float min_alpha, int use_alpha, void* scratch, float* points, float* colors,
                                     int64_t* count, void* stream);
PINGS_API size_t pings_eval_voxel_scratch_bytes(int64_t n);
PINGS_API int pings_eval_voxel_centroids(const float* points, int64_t n, const int64_t* n_dev, double voxel,
                                         void* scratch, float* out, int64_t* count, int32_t* status, void* stream);
PINGS_API size_t pings_eval_nn_scratch_bytes(int64_t m);
PINGS_API int pings_eval_nn_build(const float* dst, int64_t m, const int64_t* m_dev, double cell, void* scratch,
                                  int32_t* status, void* stream);
PINGS_API int pings_eval_nn_query(const float* src, int64_t n, const int64_t* n_dev, const void* scratch, int64_t m,
                                  double cell, double max_dist, float* dist, int64_t* idx, void* stream);
PINGS_API int pings_eval_pair_reduce(const float* dist_p, int64_t np, const int64_t* np_dev, const float* dist_r,
                                     int64_t nr, const int64_t* nr_dev, double threshold, double truncation_com,
                                     const int32_t* status, double* record, void* stream);

/* ------------------------------------------------------------- camera pose on the device
 * utils/campose_utils.py:28-98 (`update_pose`, `SE3_exp`) and gaussian_splatting/utils/cameras.py:207-219
 * (`CamImage.set_pose`), each as ONE launch of one 64-lane workgroup with no host wait.  The arithmetic runs in fp64
 * from the fp32 inputs and every output is rounded to fp32 once.  Matrices are read through element strides
 * (element [r, c] of X is X[r * X_s0 + c * X_s1]), so the transposed views a `CamImage` holds need no copy.
 *
 * Both entries fill one caller-allocated block `out` of 40 fp32 words:
 *   [0,16)  world_view_transform = T_cw^T (row-major 4x4; R = out[:3,:3]^T and T = out[3,:3] are views of it)
 *   [16,32) full_proj_transform = world_view_transform(fp32) . projection_matrix
 *   [32,35) camera_center      35: unused      36: |tau| (fp32)      37: converged (uint32 0 / 1)      38,39: unused
 *
 * pings_camera_update_pose: tau = [cam_trans_delta, cam_rot_delta]; T_cw' = SE3_exp(tau) . [R T; 0 1], both
 *   `angle < 1e-5` series branches of the reference included; camera_center = -R'^T t'; converged = |tau| <
 *   converged_threshold; the two delta vectors are set to zero.  |tau| == 0 (pose optimisation off: the reference
 *   returns True and touches nothing): the current world_view_transform, full_proj_transform and camera_center are
 *   copied into the block bit for bit, converged = 1, the deltas are left alone.  `out` must not overlap an input.
 * pings_camera_set_pose: T_wc [4,4] (fp64 if is_f64, else fp32) camera -> world; T_cw is its GENERAL inverse
 *   (cofactors and determinant in fp64, no rigid shortcut); camera_center = T_wc[:3, 3]; words 35..37 are zero.
 *   A singular T_wc gives non-finite outputs (no status: that would need a host wait). */
typedef struct pings_camera_pose_args {
  const float* R;                    /* [3,3] rotation of T_cw */
  const float* T;                    /* [3] translation of T_cw */
  const float* projection_matrix;    /* [4,4] */
  const float* world_view_transform; /* [4,4] current values, read only when |tau| == 0 */
  const float* full_proj_transform;  /* [4,4] */
  const float* camera_center;        /* [3] */
  float* cam_trans_delta;            /* [3] rho, contiguous */
  float* cam_rot_delta;              /* [3] theta, contiguous */
  float* out;                        /* [40] */
  int64_t R_s0, R_s1, T_s, proj_s0, proj_s1, wvt_s0, wvt_s1, fpt_s0, fpt_s1, center_s;
  double converged_threshold;
} pings_camera_pose_args;
PINGS_API int pings_camera_update_pose(const pings_camera_pose_args* args, void* stream);
PINGS_API int pings_camera_set_pose(const void* T_wc, int is_f64, int64_t s0, int64_t s1,
                                    const float* projection_matrix, int64_t proj_s0, int64_t proj_s1, float* out,
                                    void* stream);

/* ------------------------------------------------------------- SDF training-sample pool
 * The reference's torch code around the mapper's sample pool, on the caller's own tensors (no state is kept here).
 * Every kernel is bitwise deterministic: no float atomics, no hand-offs between waves.
 *
 * pings_pool_sample: `DataSampler.sample` (utils/data_sampler.py:18-264) with the three noise tensors passed in, one
 *   thread per output row.  row = p * S + s, S = surface_sample_n + free_front_n + free_behind_n + 1; s = 0 is the
 *   measured point, then the surface samples, the front samples, the behind samples (the reference's ray-wise order).
 *   Replicate j of a section reads its noise at j * P + p.  fp32 op for op with IEEE division and square root; the
 *   python-side scalar products (2 * range, 1 + 0.5 * scale, end - 0.2 * end) are formed in double from the fields
 *   below and rounded to fp32 once.  sdf_label = -displacement; weight < 0 marks free space; out_sem (int32) is the
 *   label for s <= surface_sample_n and 0 elsewhere, out_color the colour there and -1 elsewhere.  normal / sem /
 *   color and their outputs are nullable together.  A point at the origin gives the reference's inf / NaN pattern.
 * pings_pool_draw: the indexing of `Mapper.get_batch` (utils/mapper.py:704-771) and its row gathers in one launch.
 *   Output row b < bs_history takes i = local_idx ? local_idx[r_hist[b]] : r_hist[b], the others
 *   i = new_idx[r_new[b - bs_history]]; dst_g[b] = src_g[i] for every job g (rows = bs_history + bs_new in each job;
 *   any row width).  An r outside its index list or an i outside [0, pool_rows) is never dereferenced: bit 0 of the
 *   device word `out_of_range` (nullable; the caller zeroes it) is set and the row is zero-filled.
 * pings_pool_ts_range: min_max[0] = min(ts), min_max[1] = max(ts) (device int64; INT64_MAX / INT64_MIN for N == 0).
 * pings_pool_transform: `Mapper.transform_data_pool` (utils/mapper.py:774-778, utils/tools.py:903-921) in place:
 *   p <- R[ts] p + t[ts] on points[N,3] fp32, pose_diff [num_poses,4,4] row-major (fp64 when pose_is_f64, rounded to
 *   fp32 first as `transformation.to(points)` does), ts int32 or int64 with python index semantics; a ts outside
 *   [-T, T) sets bit 0 of `out_of_range` (nullable) and leaves the row alone.
 * pings_pool_window_count / pings_pool_window: the sample window of `process_frame` (utils/mapper.py:429-438):
 *   rows (int64, ascending) with sqrt(dx^2 + dy^2 [+ dz^2]) < radius in fp32, d = p - origin (origin: DEVICE [3]).
 *   _count fills `scratch` (pings_pool_window_scratch_bytes(n)) and returns the number of rows in *count (HOST; one
 *   polled read-back); pings_pool_window then writes them, never past `capacity`.  No per-row temporary. */
typedef struct pings_pool_sample_args {
  int64_t P;
  int32_t surface_sample_n, free_front_n, free_behind_n, color_channels;
  int32_t dist_weight_on, behind_dropoff_on, sem_is_i64, reserved;
  double surface_sample_range, free_sample_begin_ratio, free_sample_end_dist, dist_weight_scale, max_range;
  const float* points;        /* [P,3] */
  const float* normal;        /* [P,3] or NULL */
  const void* sem;            /* [P] int32 / int64 or NULL */
  const float* color;         /* [P,color_channels] or NULL */
  const float* noise_surface; /* [surface_sample_n * P] standard normal */
  const float* noise_front;   /* [free_front_n * P] uniform [0,1) */
  const float* noise_behind;  /* [free_behind_n * P] uniform [0,1) */
  float* coord;               /* [P*S,3] */
  float* sdf_label;           /* [P*S] */
  float* weight;              /* [P*S] */
  float* out_normal;          /* [P*S,3] or NULL */
  int32_t* out_sem;           /* [P*S] or NULL */
  float* out_color;           /* [P*S,color_channels] or NULL */
} pings_pool_sample_args;
PINGS_API int pings_pool_sample(const pings_pool_sample_args* args, void* stream);
PINGS_API int pings_pool_draw(const pings_gather_job* jobs, int njobs, const int64_t* r_hist, int64_t bs_history,
                              const int64_t* r_new, int64_t bs_new, const int64_t* local_idx, int64_t n_local,
                              const int64_t* new_idx, int64_t n_new, int64_t pool_rows, int32_t* out_of_range,
                              void* stream);
PINGS_API int pings_pool_ts_range(const void* ts, int32_t ts_is_i64, int64_t N, int64_t* min_max, void* stream);
PINGS_API int pings_pool_transform(int64_t N, float* points, const void* ts, int32_t ts_is_i64, const void* pose_diff,
                                   int32_t pose_is_f64, int64_t num_poses, int32_t* out_of_range, void* stream);
PINGS_API size_t pings_pool_window_scratch_bytes(int64_t n);
PINGS_API int pings_pool_window_count(const float* points, int64_t n, const float* origin, float radius,
                                      int32_t range_filter_2d, void* scratch, int64_t* count, void* stream);
PINGS_API int pings_pool_window(const float* points, int64_t n, const float* origin, float radius,
                                int32_t range_filter_2d, const void* scratch, int64_t* rows, int64_t capacity,
                                void* stream);

/* ------------------------------------------------------------- the pool part of `Mapper.process_frame`
 * What utils/mapper.py:270-284 and :340-426 do once per mapped frame, on the caller's own buffers (no state is kept
 * here).  Plain stores, no float atomics, no LDS: every result is bitwise reproducible.  A pose is a DEVICE [4,4]
 * row-major matrix, fp32 or fp64 (rounded to fp32 first, as `transformation.to(points)` does); a transformed row is
 * ((R_i0 x + R_i1 y) + R_i2 z) + t_i, the order of pings_pool_transform.
 *
 * pings_pool_append: rows [n, n + m) of every pool tensor in one launch (:340-366): global_coord = R coord + t,
 *   time = frame_id, sdf_label / weight / sem / color / normal copied.  sem, color and normal are nullable together
 *   with their pools; `capacity` is the number of rows every pool buffer holds (n + m <= capacity is checked).
 * pings_pool_discard_mark: keep[r[j]] = 0 for j < discard_count (:395-399; `keep` is n bytes the caller has set to 1,
 *   `r` the int64 draw, duplicates expected).  An r[j] outside [0, n) is not dereferenced and sets bit 0 of the device
 *   word `status` (nullable; the caller zeroes it).
 * pings_pool_compact_count / pings_pool_compact: the boolean-mask indexing of :404-423 for every pool tensor, stable,
 *   OUT OF PLACE.  A wave owns 2048 consecutive rows; _count writes the per-wave numbers of kept rows to `scratch`
 *   (pings_pool_compact_scratch_bytes(n): 16 B per 2048 rows), one wave scans them, and counts2 (HOST, two int64; one
 *   polled read-back) receives the number of kept rows and the number of kept rows among the last `tail`.
 *   pings_pool_compact then moves the rows: dst_g[rank] = src_g[row] for every job g in one launch (blockIdx.y = g,
 *   any row width); jobs[g].rows is the number of rows dst_g holds, never written past.  src and dst must not overlap.
 * pings_pool_select_count / pings_pool_select_update: the update points of :262-284.  Selected: the rows with
 *   |sdf_label| < fp32(thr), or every row with `select_all` (then no count is needed: rank = row).  _count fills
 *   `scratch` (pings_pool_select_scratch_bytes(n)) and returns their number in *count (HOST; one polled read-back).
 *   pings_pool_select_update writes, in ascending row order and never past `capacity` rows: out_points = R coord + t,
 *   out_color = the colour row, out_normal = R normal (no translation); color / normal are nullable with their
 *   outputs. */
typedef struct pings_pool_append_args {
  int64_t n, m, capacity;
  int32_t frame_id, color_channels, pose_is_f64, reserved;
  const void* pose;            /* DEVICE [4,4] */
  const float* coord;          /* [m,3], sensor frame */
  const float* sdf_label;      /* [m] */
  const float* weight;         /* [m] */
  const int32_t* sem;          /* [m] or NULL */
  const float* color;          /* [m,color_channels] or NULL */
  const float* normal;         /* [m,3] or NULL */
  float* global_coord_pool;    /* [capacity,3] */
  float* sdf_label_pool;       /* [capacity] */
  float* weight_pool;          /* [capacity] */
  int32_t* time_pool;          /* [capacity] */
  int32_t* sem_label_pool;     /* [capacity] or NULL */
  float* color_pool;           /* [capacity,color_channels] or NULL */
  float* normal_label_pool;    /* [capacity,3] or NULL */
} pings_pool_append_args;
typedef struct pings_pool_select_args {
  int64_t n, capacity;
  int32_t color_channels, pose_is_f64, select_all, reserved;
  double thr;
  const void* pose;            /* DEVICE [4,4] */
  const float* coord;          /* [n,3] */
  const float* sdf_label;      /* [n]; NULL with select_all */
  const float* color;          /* [n,color_channels] or NULL */
  const float* normal;         /* [n,3] or NULL */
  const void* scratch;         /* filled by pings_pool_select_count; NULL with select_all */
  float* out_points;           /* [capacity,3] */
  float* out_color;            /* [capacity,color_channels] or NULL */
  float* out_normal;           /* [capacity,3] or NULL */
} pings_pool_select_args;
PINGS_API int pings_pool_append(const pings_pool_append_args* args, void* stream);
PINGS_API int pings_pool_discard_mark(const int64_t* r, int64_t discard_count, int64_t n, uint8_t* keep,
                                      int32_t* status, void* stream);
PINGS_API size_t pings_pool_compact_scratch_bytes(int64_t n);
PINGS_API int pings_pool_compact_count(const uint8_t* keep, int64_t n, int64_t tail, void* scratch, int64_t* counts2,
                                       void* stream);
PINGS_API int pings_pool_compact(const pings_gather_job* jobs, int njobs, const uint8_t* keep, int64_t n,
                                 const void* scratch, void* stream);
PINGS_API size_t pings_pool_select_scratch_bytes(int64_t n);
PINGS_API int pings_pool_select_count(const float* sdf_label, int64_t n, double thr, void* scratch, int64_t* count,
                                      void* stream);
PINGS_API int pings_pool_select_update(const pings_pool_select_args* args, void* stream);

/* ------------------------------------------------------------- frame-time point tests
 * Three per-frame query steps of the reference's `Mapper`, on the caller's own tensors (no state is kept here).  Every
 * threshold is the double the reference forms between python scalars; it is rounded to fp32 once, as torch does with a
 * python scalar against an fp32 tensor.  Bitwise deterministic: no LDS, no float atomics, no hand-offs between waves.
 *
 * pings_frame_new_count / pings_frame_new_rows: the new-sample test of `process_frame` (utils/mapper.py:447-513).  Row r
 *   of coord[n,3] / sdf_label[n] looks up its OWN cell in the map's table (`m`: table or compact, buffer_size,
 *   neural_points, resolution; no neighbourhood, no time window: `query_certainty`, model/neural_gaussians.py:1117-1133,
 *   under `set_search_neighborhood(1, 0.0)`), drops the point when its squared distance is above `max_valid_dist2` (the
 *   one-cell 3 * ((1 + 1) * resolution)^2, an argument: the map is not touched) and takes
 *   certainty = point_certainties[idx], 0 without a point.  The row is kept iff certainty < new_certainty_thre and
 *   |sdf_label| < label_thre (= 3 * surface_sample_range_m).  _count fills `scratch`
 *   (pings_frame_new_scratch_bytes(n): a bit per row and 12 B per 512 rows) and returns the number of kept rows in
 *   *count (HOST; one polled read-back); _rows then writes r + pool_offset for the kept rows in ascending order (int64),
 *   never past `capacity`.  A table entry >= num_points is treated as an empty cell.
 * pings_frame_static_mask: `Mapper.dynamic_filter` / `dynamic_filter_neural_points` (utils/mapper.py:554-564) from the
 *   fused query's outputs: mask[i] = certainty[i] < certainty_thre || sdf[i] < sdf_thre, and with grad[n,3] != NULL
 *   also && (sqrt(gx^2 + gy^2 + gz^2) > min_grad_norm || certainty[i] < certainty_thre).  *dynamic_count (DEVICE int64;
 *   cleared by the call) receives the number of zeros, one integer atomic per wave.
 * pings_frame_valid_scatter: `Mapper.check_invalid_neural_points` (utils/mapper.py:1647-1655) for the stable rows
 *   rows[n] (distinct local rows) with their sdf[n] and nn_count[n]: v = |sdf[i]| < sdf_thre && nn_count[i] >= min_nn_count
 *   is stored to local_valid[rows[i]] and valid[local_idx[rows[i]]].  A row outside [0, n_local) or a global row outside
 *   [0, n_global) is skipped. */
PINGS_API size_t pings_frame_new_scratch_bytes(int64_t n);
PINGS_API int pings_frame_new_count(const pings_knn_map* m, const float* point_certainties, int64_t num_points,
                                    const float* coord, const float* sdf_label, int64_t n, double max_valid_dist2,
                                    double new_certainty_thre, double label_thre, void* scratch, int64_t* count,
                                    void* stream);
PINGS_API int pings_frame_new_rows(const void* scratch, int64_t n, int64_t pool_offset, int64_t* rows,
                                   int64_t capacity, void* stream);
PINGS_API int pings_frame_static_mask(const float* sdf, const float* certainty, const float* grad, int64_t n,
                                      double certainty_thre, double sdf_thre, double min_grad_norm, uint8_t* mask,
                                      int64_t* dynamic_count, void* stream);
PINGS_API int pings_frame_valid_scatter(const int64_t* rows, int64_t n, const float* sdf, const int64_t* nn_count,
                                        double sdf_thre, int64_t min_nn_count, const int64_t* local_idx,
                                        int64_t n_local, int64_t n_global, uint8_t* local_valid, uint8_t* valid,
                                        void* stream);

/* ------------------------------------------------------------- loop-closure context
 * The scan-context descriptors and the global loop search of utils/loop_detector.py (`ptcloud2sc_torch`, `sc2rk`,
 * `set_virtual_node`, `detect_loop`, `distance_sc_torch`, `distance_sc_feature_torch`) on caller-owned buffers.  A
 * descriptor is sc[R,S] (largest z per ring / sector bin, 0.0 for a bin no point reached) and, with D-wide point
 * features, sc_feat[R,S,D] (mean feature row per bin); a ring key is the mean over the sectors, [R] or [R,D].
 * Limits: R <= PINGS_LOOP_MAX_R, S <= PINGS_LOOP_MAX_S, D <= PINGS_LOOP_MAX_D, poses / queries <= PINGS_LOOP_MAX_Q,
 * candidates <= PINGS_LOOP_MAX_C; outside them (and for a null pointer) an entry returns PINGS_ERR_ARG.  No float
 * atomics: maxima by integer atomics on an order-preserving key, feature sums by the deterministic row scatter in
 * ascending point index, every other sum in a fixed order.  Two runs on the same input agree bit for bit.
 *
 * pings_loop_context_build: descriptors of M poses from one pass over points[n_points,3] (features[n_points,D] with
 *   D > 0).  transforms[M,12] are row-major 3x4 fp32 (rounded once from fp64 by the caller; identity for a cloud in
 *   its sensor frame).  Per (pose, point), in fp32: p' = T p, r = |p'|, kept iff r < max_length (false for NaN / inf
 *   rows), theta = atan2(y', x') * 180 / pi + 180, ring = floor(r / (max_length / R)), sector = floor(theta / (360 / S)),
 *   both clamped to the shape.  Outputs sc[M,R,S], ringkey[M,R] and, with D > 0, sc_feat[M,R,S,D], ringkey_feat[M,R,D].
 *   use_stored[M] (DEVICE, nullable): a pose with a non-zero flag takes stored_sc[R,S], stored_ringkey[R]
 *   (stored_sc_feat, stored_ringkey_feat) instead of what was built: the reference's centre pose (:135-139).
 *   scratch: pings_loop_context_scratch_bytes(n_points, M, R, S, D) bytes (0 for arguments outside the limits).
 * pings_loop_ring_key: `sc2rk` of one descriptor, sc[R,S] (D = 0) or sc[R,S,D].
 * pings_loop_virtual_poses: the M = 2 * side_count + 1 lateral virtual poses of `set_virtual_node` (:84-133) from
 *   frame_pose[4,4] and last_frame_pose[4,4] (nullable: lateral direction (0,1,0)), both DEVICE fp64 row-major with
 *   last row (0,0,0,1): lat_tran[M,3] (fp32, as the reference forms it), tran_from_frame[M,4,4] (fp64),
 *   transforms[M,12] = inv(frame_pose @ inv(T_k)) in fp64 rounded once, use_stored[k] = (|lat_tran[k]| == 0 in fp32).
 *   Two identical consecutive poses give NaN everywhere, as in the reference.
 * pings_loop_search: `detect_loop` (:250-295) in two launches.  bank_context[capacity, R*S*(use_feature ? D : 1)] and
 *   bank_ringkey[capacity, R*(use_feature ? D : 1)] hold the nodes by slot; cand[C] are slots in the caller's order (a
 *   slot outside [0, capacity) is skipped); the Q queries are query_context / query_ringkey in the same layouts.  Phase
 *   one: ring-key distance of every (query, candidate) pair, L1 (plain) or 1 - cosine (features); the winner is the
 *   smallest distance, then the earliest query, then the first candidate in cand order.  Phase two (a second launch that
 *   reads the winner from `record`; skipped on the device when the distance exceeds ringkey_thre): for the shifts
 *   i = 1..S the candidate is rolled by i sectors and the mean over the S (S*D) columns of the cosine similarity over
 *   the R rings is taken (a zero column contributes 0; eps 1e-8); the largest mean wins, ties to the smallest shift.
 *   record[8] (DEVICE int32): 0 position in cand (-1: none), 1 query, 2 ring-key distance (fp32 bits), 3 cosine distance
 *   (fp32 bits), 4 shift in 1..S (S = no rotation), 5 gate (1 = phase two ran), 6-7 spare.  Fields 3 and 4 are written
 *   only when the gate is open.  query_tran[Q,3] / win_tran[3] (nullable): the winner's row is copied to win_tran.
 * pings_loop_context_distance: phase two alone on two descriptors (sc1 is the one rolled): record[3], record[4].
 * pings_loop_read_record: one polled read of 8 words into record_host (HOST): record[0..7], or with win_tran_dev
 *   record[0..4] followed by win_tran[0..2]. */
#define PINGS_LOOP_MAX_R 32
#define PINGS_LOOP_MAX_S 128
#define PINGS_LOOP_MAX_D 16
#define PINGS_LOOP_MAX_Q 16
#define PINGS_LOOP_MAX_C 65536
PINGS_API size_t pings_loop_context_scratch_bytes(int64_t n_points, int32_t M, int32_t R, int32_t S, int32_t D);
PINGS_API int pings_loop_context_build(const float* points, int64_t n_points, const float* features, int32_t D,
                                       const float* transforms, int32_t M, int32_t R, int32_t S, double max_length,
                                       const int32_t* use_stored, const float* stored_sc, const float* stored_ringkey,
                                       const float* stored_sc_feat, const float* stored_ringkey_feat, void* scratch,
                                       float* sc, float* ringkey, float* sc_feat, float* ringkey_feat, void* stream);
PINGS_API int pings_loop_ring_key(const float* sc, int32_t R, int32_t S, int32_t D, float* ringkey, void* stream);
PINGS_API int pings_loop_virtual_poses(const double* frame_pose, const double* last_frame_pose, int32_t side_count,
                                       double step_m, float* transforms, double* tran_from_frame, float* lat_tran,
                                       int32_t* use_stored, void* stream);
PINGS_API int pings_loop_search(const float* bank_context, const float* bank_ringkey, int64_t capacity,
                                const int32_t* cand, int32_t C, const float* query_context, const float* query_ringkey,
                                int32_t Q, int32_t R, int32_t S, int32_t D, int32_t use_feature, double ringkey_thre,
                                const float* query_tran, int32_t* record, float* win_tran, void* stream);
PINGS_API int pings_loop_context_distance(const float* sc1, const float* sc2, int32_t R, int32_t S, int32_t D,
                                          int32_t* record, void* stream);
PINGS_API int pings_loop_read_record(const int32_t* record_dev, const float* win_tran_dev, int32_t* record_host,
                                     void* stream);

/* ------------------------------------------------------------- LiDAR frame front-end
 * What dataset/slam_dataset.py:584-621 (`filter_and_correct`), utils/tools.py:1088-1177 (`deskewing`, `slerp_pose`),
 * :1242-1351 (`project_points_to_cam_torch`) and gaussian_splatting/utils/cameras.py:233-243 (`set_depth_img`) compute,
 * on caller-owned buffers (no state is kept here).  A point cloud is fp32 rows of `stride` floats whose first three are
 * x, y, z.  Bitwise deterministic: the only atomic is an integer maximum.  No entry waits for the device.
 *
 * pings_lidar_crop: mask[i] = min_range < dist < max_range && min_z < z < max_z, all strict, in fp32 with the four
 *   thresholds rounded to fp32 once; dist = sqrt(x^2 + y^2 [+ z^2 unless on_xy_plane]).  A NaN row gives 0.
 * pings_lidar_deskew: in place on x, y, z.  s_i = (ts_i - min ts) / (max ts - min ts) - ts_ref_pose in fp64, rounded to
 *   fp32 (ts [n] fp32 or fp64; max == min gives NaN coordinates).  pose: DEVICE [4,4] row-major (fp32 or fp64),
 *   T_last<-cur = (R, t); with (a, theta) the axis and angle of R, theta in [0, pi], R(s) is the rotation by s theta about
 *   a (the shortest-arc slerp from the identity, any real s; theta == 0 gives the identity exactly) and
 *   p_i <- R(s_i) p_i + s_i t.  Axis and angle are formed in fp64 by the first wave of each workgroup, the per-point
 *   Rodrigues formula runs in fp32.  num_other > 0 is the multi-LiDAR branch: lidar_idx[n] (int32 or int64) names the
 *   LiDAR of a row; 0 takes the formula above, k in [1, num_other] takes T = T_l_lm[k-1] (HOST [num_other,16] row-major
 *   fp64, last row 0 0 0 1), pose_k = T pose T^-1, s = s_i + ts_diff[k-1] (HOST, nullable) and
 *   p <- T^-1 (R_k(s) (T p) + s t_k); any other index leaves the row alone.  num_other <= PINGS_LIDAR_MAX_LIDARS.
 *   Two launches: per-workgroup (min, max) partials into `scratch` (pings_lidar_deskew_scratch_bytes()), then the apply
 *   launch, which reduces them.  n == 0 is an argument error (the reference's torch.min raises).
 * pings_lidar_slerp_pose: out[4,4] = [R(s), s t; 0 1] of pose (s = ts - ts_ref_pose, formed by the caller), its rigid
 *   inverse with `invert`, and left-multiplied by `left` (DEVICE [4,4], nullable) after that; fp64 arithmetic, rounded
 *   once to out's type.  One 64-lane launch.
 * pings_lidar_project: every point into every camera in one launch.  Per camera c (K: DEVICE [3,3], T: DEVICE >= 12
 *   floats, rows 0..2 of T_c_l, both fp32 row-major): P = R p + t, q = K P, d = q_z (d == 0 becomes -1e-6),
 *   u = rint(q_x / |d|), v = rint(q_y / |d|) (half to even; -0 is pixel 0); the point is visible iff 0 <= u < W,
 *   0 <= v < H, d > min_depth, d < max_depth (false for non-finite values).  A visible point raises keys[v W + u]
 *   (uint32; the caller zero-fills it once per frame, all cameras in one buffer) to ~bits(d): since d > min_depth >= 0
 *   the largest key is the smallest depth and 0 means no hit.  The point takes image[:, v, u] of the LAST camera that
 *   sees it: rgb[i rgb_stride + 0..2], 0 to indicator[i indicator_stride] (nullable).  A point no camera sees gets -1 in
 *   all of them with `init`, and is left alone without.  visible[i] (nullable) = seen by any camera.  rgb may point into
 *   the cloud's own colour columns.  ncam <= PINGS_LIDAR_MAX_CAMS; l0..l3 and src are not read.
 * pings_lidar_depth_pyramid: per camera, level 0 = keys decoded (0 for no hit), or `src` [H,W] when keys is NULL; level
 *   k = 1..3 [H >> k, W >> k] takes level-0 pixel (2^k i + 2^k - 1, 2^k j + 2^k - 1), which is three chained
 *   F.interpolate(scale_factor=0.5, mode='nearest-exact').  Each of l0..l3 is nullable.  One launch for all cameras. */
#define PINGS_LIDAR_MAX_CAMS 8
#define PINGS_LIDAR_MAX_LIDARS 8
typedef struct pings_lidar_cam {
  const float* image;          /* [3,H,W] */
  const float* K;              /* DEVICE [3,3] */
  const float* T;              /* DEVICE [4,4] T_c_l (12 floats read) */
  uint32_t* keys;              /* [H*W] depth keys */
  const float* src;            /* [H,W]: the pyramid's source when keys is NULL */
  float *l0, *l1, *l2, *l3;    /* pyramid levels */
  int32_t H, W;
} pings_lidar_cam;
PINGS_API int pings_lidar_crop(const float* points, int64_t n, int64_t stride, double min_z, double max_z,
                               double min_range, double max_range, int32_t on_xy_plane, uint8_t* mask, void* stream);
PINGS_API size_t pings_lidar_deskew_scratch_bytes(void);
PINGS_API int pings_lidar_deskew(float* points, int64_t n, int64_t stride, const void* ts, int32_t ts_is_f64,
                                 const void* pose, int32_t pose_is_f64, double ts_ref_pose, const void* lidar_idx,
                                 int32_t lidar_idx_is_i64, int32_t num_other, const double* T_l_lm,
                                 const double* ts_diff, void* scratch, void* stream);
PINGS_API int pings_lidar_slerp_pose(const void* pose, int32_t pose_is_f64, double s, const void* left,
                                     int32_t left_is_f64, int32_t invert, void* out, int32_t out_is_f64, void* stream);
PINGS_API int pings_lidar_project(const float* points, int64_t n, int64_t stride, const pings_lidar_cam* cams,
                                  int32_t ncam, double min_depth, double max_depth, float* rgb, int64_t rgb_stride,
                                  float* indicator, int64_t indicator_stride, uint8_t* visible, int32_t init,
                                  void* stream);
PINGS_API int pings_lidar_depth_pyramid(const pings_lidar_cam* cams, int32_t ncam, void* stream);

/* ------------------------------------------------------------- camera frame front-end (csrc/camfront.hip)
 * The image pyramids of CamImage.__init__ (gaussian_splatting/utils/cameras.py:39, :116-182) on caller-owned buffers.
 * No entry allocates, copies or waits; every output is bitwise the same from run to run (plain stores only).
 *
 * pings_camfront_pyramid: up to PINGS_CAMFRONT_MAX_MAPS maps (8 cameras x RGB, depth, sky mask, normal) in ONE launch;
 *   the table travels in the kernel arguments and launches_out (HOST, may be NULL) receives the number of launches made.
 *   Level k = 0..3 of a map is a contiguous [C, H >> k, W >> k] buffer (a trailing odd row or column is dropped at each
 *   level); each of l0..l3 is nullable, a NULL level is not written, and no level is read back: levels 1..3 are formed
 *   from the level-0 tile in registers and cross-lane moves.  By kind:
 *     PINGS_CAMFRONT_RGB_U8   src uint8 [H, W, 3] contiguous (strides ignored); level 0 = float(u) / 255.0f, IEEE division
 *     PINGS_CAMFRONT_RGB_F32  src fp32 [3, H, W] with element strides stride_c / stride_y / stride_x (any view); level 0 =
 *                             the value clamped to [0, 1] as torch.clamp does (a NaN stays a NaN)
 *     PINGS_CAMFRONT_NORMAL   src fp32 [3, H, W] with strides; level 0 = the value (pass l0 = NULL to keep the input)
 *       these three, levels 1..3: 0.5 (0.5 a + 0.5 b) + 0.5 (0.5 c + 0.5 d) of the 2 x 2 block of the level above
 *       (a, b the upper pair), rounded to fp32 at every level: F.interpolate(scale_factor=0.5, mode='bilinear')
 *     PINGS_CAMFRONT_DEPTH    src fp32 [1, H, W] with strides; level k takes level-0 pixel (2^k y + 2^k - 1,
 *                             2^k x + 2^k - 1): chained mode='nearest-exact'.  l0 is not written.
 *     PINGS_CAMFRONT_SKY      src bytes [1, H, W] with strides; level k takes level-0 pixel (2^k y, 2^k x): chained
 *                             mode='nearest' of a bool image.  l0 is not written.
 *   A workgroup takes a PINGS_CAMFRONT_TILE_W x PINGS_CAMFRONT_TILE_H tile of one map and checks bounds per level.  A map
 *   with W % 16 == 0, unit stride_x, stride_y and stride_c multiples of 16 and 16-byte aligned pointers moves 8- and
 *   16-byte words per lane, any other map single elements; the values are the same. */
#define PINGS_CAMFRONT_MAX_MAPS 32
#define PINGS_CAMFRONT_TILE_W 128
#define PINGS_CAMFRONT_TILE_H 32
#define PINGS_CAMFRONT_RGB_U8 0
#define PINGS_CAMFRONT_RGB_F32 1
#define PINGS_CAMFRONT_NORMAL 2
#define PINGS_CAMFRONT_DEPTH 3
#define PINGS_CAMFRONT_SKY 4
typedef struct pings_camfront_map {
  const void* src;
  void *l0, *l1, *l2, *l3;     /* levels, each nullable */
  int64_t stride_c, stride_y, stride_x;
  int32_t H, W, kind, reserved;
} pings_camfront_map;
PINGS_API int pings_camfront_pyramid(const pings_camfront_map* maps, int32_t nmaps, int32_t* launches_out, void* stream);

/* The mono-depth cloud of dataset/slam_dataset.py:366-477, per camera, with every count on the device.
 *
 * pings_camfront_align: pred, lidar_depth [n] fp32.  Over the pixels with lidar > min_range && pred > min_range &&
 *   lidar < 0.8 max_range (strict; both thresholds rounded to fp32 once, as numpy rounds a Python scalar) the line
 *   lidar = k pred + b by least squares, from fp64 sums.  record (DEVICE, PINGS_CAMFRONT_FIT_RECORD doubles) = count, k,
 *   b, rmse before (sqrt of the mean of (pred - lidar)^2, NaN at count 0), rmse after.  count <= PINGS_CAMFRONT_MIN_FIT
 *   gives k = 1, b = 0 and rmse after = NaN.  Two launches: per-workgroup partial sums into `scratch`
 *   (pings_camfront_align_scratch_bytes()) in a fixed order, then one workgroup that adds them in index order.
 * pings_camfront_mono_cloud: pred [H, W] fp32, image [H, W, 3] uint8.  Per pixel, in this order:
 *   d = fp32(k pred + b) evaluated in fp64 (k, b = record[1], record[2]; record NULL: 1, 0);
 *   sky = d > 1.2 max_range, and d = 0 there; with high_z: d > 0.8 max_range -> 0, then d < 2 min_range -> 0; without:
 *   d < 0.2 max_range -> 0 (every threshold rounded to fp32 once, every comparison strict).  sky [H, W] bytes and gated
 *   (nullable) [H, W] fp32 receive sky and d.  A pixel gives a row iff 0 < d < depth_trunc: rows[o] = xyz, rgb with
 *   xyz = cam_to_lidar ((u - cx) d / fx, (v - cy) d / fy, d) in fp64 rounded once (intrinsic HOST = fx, fy, cx, cy;
 *   cam_to_lidar HOST = the first three rows of T_c_l^-1, row-major) and rgb = byte / 255 in fp64 rounded once, in
 *   row-major pixel order; rows holds H W rows of 6 floats, *count (DEVICE) receives how many were written.  Three
 *   launches (flag, scan, scatter); scratch of pings_camfront_cloud_scratch_bytes(H W).
 * pings_camfront_voxel_average: Open3D's voxel_down_sample over rows of 6 floats (position, colour), with the contract
 *   of pings_eval_voxel_centroids: cells from the first three columns in fp64 on a grid anchored at min - voxel / 2,
 *   output in ascending cell key, sums in fp64 in input order over all six columns, PINGS_EVAL_EXTENT in *status.  The
 *   input has n rows of capacity and *n_dev (nullable) live rows.  The cells are appended to out [out_cap, 6] behind
 *   *offset rows (DEVICE, nullable = 0) and *count (DEVICE, another word than offset) receives offset + cells, so that
 *   cameras chain without the host; cells that find no room are dropped and PINGS_CAMFRONT_FULL is or-ed into *status.
 *   scratch of pings_camfront_voxel_scratch_bytes(n). */
#define PINGS_CAMFRONT_FIT_RECORD 5
#define PINGS_CAMFRONT_MIN_FIT 100
#define PINGS_CAMFRONT_FULL 2
PINGS_API size_t pings_camfront_align_scratch_bytes(void);
PINGS_API int pings_camfront_align(const float* pred, const float* lidar_depth, int64_t n, double min_range,
                                   double max_range, void* scratch, double* record, void* stream);
PINGS_API size_t pings_camfront_cloud_scratch_bytes(int64_t hw);
PINGS_API int pings_camfront_mono_cloud(const float* pred, const uint8_t* image, int32_t H, int32_t W,
                                        const double* record, const double* intrinsic, const double* cam_to_lidar,
                                        double min_range, double max_range, double depth_trunc, int32_t high_z,
                                        void* scratch, uint8_t* sky, float* gated, float* rows, int64_t* count,
                                        void* stream);
PINGS_API size_t pings_camfront_voxel_scratch_bytes(int64_t n);
PINGS_API int pings_camfront_voxel_average(const float* rows, int64_t n, const int64_t* n_dev, double voxel,
                                           void* scratch, float* out, int64_t out_cap, const int64_t* offset,
                                           int64_t* count, int32_t* status, void* stream);

/* ------------------------------------------------------ sparse TSDF fusion (csrc/tsdf.hip)
 * Depth views fused into blocks of PINGS_TSDF_BLOCK^3 voxels, the route of SLAMDataset.o3d_tsdf_fusion.  Grid point g
 * lies at origin + voxel_length * g, block b = floor(g / 8) has the key (bx + 2^20) << 42 | (by + 2^20) << 21 |
 * (bz + 2^20).  The caller owns everything:
 *   table   tkeys [tsize] int64 (-1 = free), tslots [tsize] int32 (-1 = no slot yet), tstamps [tsize] int32 (0 = never
 *           touched); tsize a power of two in [64, 2^31), at least twice the blocks it will ever hold
 *   store   block_keys [capacity] int64, tsdf / weight [capacity, 512] fp32, color [capacity, 3, 512] fp32 or NULL;
 *           voxel (lx, ly, lz) of a block at (lx*8 + ly)*8 + lz.  A block's slot never changes.
 * intrinsic (HOST) = fx, fy, cx, cy; extrinsic / cam_to_world (HOST) = the first three rows of the world -> camera 4x4
 * and of its inverse, row-major; origin (HOST) 3 doubles.  All are rounded to fp32 once.  A depth d is valid iff it is
 * finite and depth_min < d < depth_trunc.  2 sdf_trunc <= 8 voxel_length, else status 1.
 *   touch    every valid pixel with u % stride == v % stride == 0 names the blocks whose index lies per axis in
 *            [floor((q - trunc - origin) / (8 voxel)), floor((q + trunc - origin) / (8 voxel))], q its world point;
 *            absent keys are inserted (slot -1).  touched [list_cap] int32 receives the table entry of every block
 *            named in this frame once (`frame` >= 1, larger in every call), new_keys [list_cap] the keys without a
 *            slot, both in no particular order; list_cap >= 8 ceil(width / stride) ceil(height / stride).  counters [4]
 *            int32 DEVICE workspace; totals[3] (HOST, the frame's one read): touched, new, status bits
 *            (PINGS_TSDF_EXTENT: a block index outside [-2^20, 2^20) was dropped; PINGS_TSDF_TABLE_FULL).
 *   assign   sorts new_keys ascending and gives key r the slot base_slot + r: table, block_keys, and the block's
 *            fields set to tsdf 1, weight 0, colour 0.  scratch of pings_tsdf_assign_scratch_bytes(n_new).
 *   update   one workgroup per entry of touched: for each voxel p_c = R p + t, skipped unless z > 0;
 *            iu = floor(fx x / z + cx + 0.5), iv likewise, skipped outside the image or on an invalid depth d;
 *            sdf = (d - z) sqrt(1 + ((iu - cx) / fx)^2 + ((iv - cy) / fy)^2), skipped unless sdf > -sdf_trunc;
 *            tsdf <- (tsdf w + min(1, sdf / sdf_trunc)) / (w + 1), colour likewise from image [3, H, W], w <- w + 1.
 *   table_insert  files block_keys[0 .. nb) with their slots in a cleared table (after the table has grown).
 *   densify  the box lo + [0, nx) x [0, ny) x [0, nz) of grid points (lo HOST, 3 int64) as out_tsdf, out_weight
 *            (nullable) [nx, ny, nz] and out_color (nullable) [nx, ny, nz, 3]; a voxel of an absent block reads
 *            tsdf 1, weight 0, colour 0; out_tsdf is +inf where weight < min_weight (min_weight <= 0: nowhere).
 *   vertices  keys[nv] of pings_mc_emit on such a box -> verts [nv, 3] = origin + voxel_length (g0 + t axis) with
 *            t = v0 / (v0 - v1) of the edge's two values (slot 0: the point g0), in fp64 and rounded once; colors
 *            [nv, 3] = c0 + t (c1 - c0) of col [nx, ny, nz, 3] clamped to [0, 1] (both NULL without colour). */
#define PINGS_TSDF_BLOCK 8
#define PINGS_TSDF_EXTENT 1
#define PINGS_TSDF_TABLE_FULL 2
PINGS_API int pings_tsdf_table_insert(const int64_t* block_keys, int64_t nb, int64_t* tkeys, int32_t* tslots,
                                      int64_t tsize, int32_t* status, void* stream);
PINGS_API int pings_tsdf_touch(const float* depth, int height, int width, const double* intrinsic,
                               const double* cam_to_world, const double* origin, double voxel_length, double sdf_trunc,
                               float depth_min, float depth_trunc, int stride, int frame, int64_t* tkeys,
                               const int32_t* tslots, int32_t* tstamps, int64_t tsize, int64_t list_cap,
                               int32_t* touched, int64_t* new_keys, int32_t* counters, int64_t* totals, void* stream);
PINGS_API size_t pings_tsdf_assign_scratch_bytes(int64_t n_new);
PINGS_API int pings_tsdf_assign(const int64_t* new_keys, int64_t n_new, int64_t base_slot, int64_t capacity,
                                void* scratch, const int64_t* tkeys, int32_t* tslots, int64_t tsize,
                                int64_t* block_keys, float* tsdf, float* weight, float* color, void* stream);
PINGS_API int pings_tsdf_update(const float* depth, const float* image, int height, int width, const double* intrinsic,
                                const double* extrinsic, const double* origin, double voxel_length, double sdf_trunc,
                                float depth_min, float depth_trunc, const int32_t* touched, int64_t n_touched,
                                const int64_t* tkeys, const int32_t* tslots, int64_t tsize, int64_t capacity, float* tsdf,
                                float* weight, float* color, void* stream);
PINGS_API int pings_tsdf_densify(const int64_t* tkeys, const int32_t* tslots, int64_t tsize, int64_t capacity,
                                 const float* tsdf, const float* weight, const float* color, const int64_t* lo,
                                 int64_t nx, int64_t ny, int64_t nz, float min_weight, float* out_tsdf,
                                 float* out_weight, float* out_color, void* stream);
PINGS_API int pings_tsdf_vertices(const int64_t* keys, int64_t nv, const float* vol, const float* col, const int64_t* lo,
                                  int64_t nx, int64_t ny, int64_t nz, const double* origin, double voxel_length,
                                  float* verts, float* colors, void* stream);

/* ------------------------------------------------------ LiDAR scans into the TSDF volume (csrc/tsdf_points.hip, §2.9b)
 * points [n, 3] fp32 world frame, colors [n, 3] fp32 in [0, 1] or NULL, sensor [3] fp32 DEVICE; n <=
 * PINGS_TSDF_POINTS_MAX.  Table, store, key and origin as above; tindex [tsize] int32 DEVICE workspace (the place of
 * an entry in `touched`, valid for entries stamped with this `frame`).  A point is valid iff it is finite and
 * min_range < r < max_range, r = |p - sensor|.  Grid point g owns the half-open cube of edge voxel_length around it;
 * the ray sensor + s d, d = (p - sensor) / r, samples every cube it crosses with a positive chord for s in [s0, s1],
 * s1 = r + sdf_trunc, s0 = max(0, r - sdf_trunc), or 0 with space_carving (which needs a finite max_range).
 *   touch       files the blocks floor(g / 8) of the samples exactly as pings_tsdf_touch does (same lists, counters,
 *               totals and status bits); list_cap >= 8 n without carving, else the caller's bound on the blocks of a
 *               call.  totals[3] (HOST) is the call's one read.
 *   (pings_tsdf_assign, unchanged, gives the new blocks their slots.)
 *   accumulate  per sample with centre c: sdf = sign((c - o).(p - c)) |p - c| (PINGS_TSDF_SDF_POINT, sign(0) = +1) or
 *               r - (c - o).d (PINGS_TSDF_SDF_RAY); it counts iff sdf > -sdf_trunc, with t = min(1, sdf / sdf_trunc)
 *               quantised once, q = rint(t 2^PINGS_TSDF_POINTS_SCALE_BITS), colours likewise.  acc [n_touched, P, 512]
 *               uint64, P = 4 with colors and 1 without, ZEROED by the caller: plane 0 receives
 *               1 << PINGS_TSDF_POINTS_COUNT_SHIFT | (q + 2^PINGS_TSDF_POINTS_SCALE_BITS) per sample, planes 1..3 the
 *               colour q, all by 64-bit integer atomic adds.
 *   apply       per voxel with count n > 0 and exact sum S = sum q / 2^SCALE_BITS: tsdf <- fl32((tsdf w + S) / (w + n))
 *               in fp64, colour likewise, w <- min(w + n, max_weight) (INFINITY: no cap); n = 0 leaves every bit. */
#define PINGS_TSDF_POINTS_SCALE_BITS 22
#define PINGS_TSDF_POINTS_COUNT_SHIFT 44
#define PINGS_TSDF_POINTS_MAX 1048575
#define PINGS_TSDF_SDF_POINT 0
#define PINGS_TSDF_SDF_RAY 1
PINGS_API int pings_tsdf_points_touch(const float* points, int64_t n, const float* sensor, const double* origin,
                                      double voxel_length, double sdf_trunc, float min_range, float max_range,
                                      int space_carving, int frame, int64_t* tkeys, const int32_t* tslots,
                                      int32_t* tstamps, int32_t* tindex, int64_t tsize, int64_t list_cap,
                                      int32_t* touched, int64_t* new_keys, int32_t* counters, int64_t* totals,
                                      void* stream);
PINGS_API int pings_tsdf_points_accumulate(const float* points, const float* colors, int64_t n, const float* sensor,
                                           const double* origin, double voxel_length, double sdf_trunc,
                                           float min_range, float max_range, int space_carving, int sdf_mode,
                                           int frame, const int64_t* tkeys, const int32_t* tslots,
                                           const int32_t* tstamps, const int32_t* tindex, int64_t tsize,
                                           int64_t n_touched, uint64_t* acc, void* stream);
PINGS_API int pings_tsdf_points_apply(const int32_t* touched, int64_t n_touched, const int32_t* tslots, int64_t tsize,
                                      int64_t capacity, const uint64_t* acc, int with_color, float max_weight,
                                      float* tsdf, float* weight, float* color, void* stream);

/* ------------------------------------------------------ pose-graph optimisation (csrc/pgo.hip)
 * Poses X [n_nodes, 4, 4] fp64 (T_world<-frame, row-major).  Factor f: fi[f], fj[f] (-1: a prior), Z [f, 4, 4],
 * W [f, 6, 6] the square-root information, rotation first.  r = W Log(Z^-1 X_i^-1 X_j) (prior: W Log(Z^-1 X_i)),
 * cost = 1/2 sum |r|^2, update X <- X Exp(delta).  The caller classifies the factors once per graph change:
 *   kind[f]   PINGS_PGO_PRIOR, PINGS_PGO_CHAIN (|i - j| = 1) or PINGS_PGO_LOOP; lcol[f] the loop's number 0 .. n_loops-1
 *   loop_f [n_loops]: the factor of every loop, the inverse of lcol
 *   node_off [n_nodes + 1], node_ent [n_entries]: per node the list of 2 f + slot (slot 0: the node is fi, 1: fj),
 *   in the order the contributions are summed.
 * The normal matrix is block tridiagonal plus U U^T with 6 columns per loop.  pings_pgo_iteration queues ONE
 * Levenberg-Marquardt trial: linearise, assemble, damp with lambda diag(H), block Cholesky, sweeps for 1 + 6 n_loops
 * right-hand sides in chunks of `chunk` columns (a multiple of 64), the dense capacitance system, the last sweep, the
 * retraction into a candidate, its cost, and the decision, all on the device.
 *   state  [8] fp64 DEVICE: 0 lambda (set by the caller before the first trial), 1 cost before, 2 cost after, rest
 *          workspace.   status [1] int32 DEVICE, sticky bits PINGS_PGO_ST_*; the caller clears it.
 *   record [8] fp64 DEVICE: cost before, cost after, lambda of this trial, accepted, status, iteration, 0, 0.
 * A trial is accepted iff cost after <= cost before (lambda / 10, X <- candidate), else lambda * 10.
 * PINGS_PGO_ST_CONVERGED: accepted with before - after <= rel_tol * before; PINGS_PGO_ST_LAMBDA_MAX: lambda passed
 * 1e5.  pings_pgo_read_record is the one host read of a trial.  pings_pgo_cost: out_cost[0] = the cost at `poses`
 * (status bits OR-ed into args->status).  pings_pgo_pose_diff: out64 / out32 (each nullable) [n, 4, 4] =
 * after[n] before[n]^-1, rigid inverse.  scratch: pings_pgo_scratch_bytes(n_nodes, n_factors, n_loops, chunk). */
#define PINGS_PGO_PRIOR 0
#define PINGS_PGO_CHAIN 1
#define PINGS_PGO_LOOP 2
#define PINGS_PGO_ST_NEAR_PI 1
#define PINGS_PGO_ST_NOT_POSDEF 2
#define PINGS_PGO_ST_NONFINITE 4
#define PINGS_PGO_ST_CONVERGED 8
#define PINGS_PGO_ST_LAMBDA_MAX 16
#define PINGS_PGO_RECORD 8
typedef struct {
  int64_t n_nodes, n_factors, n_loops, n_entries;
  int32_t chunk, iteration;
  double rel_tol;
  const int32_t *fi, *fj, *kind, *lcol, *loop_f, *node_off, *node_ent;
  const double *Z, *W;
  double *X, *state, *record;
  int32_t* status;
  void* scratch;
} pings_pgo_args;
PINGS_API size_t pings_pgo_scratch_bytes(int64_t n_nodes, int64_t n_factors, int64_t n_loops, int32_t chunk);
PINGS_API int pings_pgo_cost(const pings_pgo_args* args, const double* poses, double* out_cost, void* stream);
PINGS_API int pings_pgo_iteration(const pings_pgo_args* args, void* stream);
PINGS_API int pings_pgo_read_record(const double* record_dev, double* record_host, void* stream);
PINGS_API int pings_pgo_pose_diff(const double* after, const double* before, int64_t n, double* out64, float* out32,
                                  void* stream);

#endif /* PINGS_HIP_H_ */
