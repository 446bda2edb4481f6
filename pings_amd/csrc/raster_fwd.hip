// Gaussian(-surfel) rasteriser, forward pass, for gfx950.
//
// Pipeline (one HIP stream, no host round trip except the 8-byte instance count):
//   preprocess_kernel   per Gaussian: camera transform, EWA projection, cull, tile rect,
//                       64-B blend record, fp32 depth key                     [HBM: 56 B in, 96 B out]
//   radix sort (P)      Gaussians by depth key (hipcub / rocPRIM)
//   gather + scan       tiles-per-Gaussian in depth order -> instance offsets
//   duplicate_kernel    emits (tile id, Gaussian id) instances in depth order  [8 B per instance]
//   radix sort (I)      STABLE sort by tile id only (ceil(log2(tiles)) bits): tile_sort.hip  [the only
//                       multi-pass traffic over the instance list; 16-bit keys instead of 64-bit]
//   tile_ranges_kernel  [start,end) of every tile in the sorted list
//   (a frame whose kept instances all lie in a short front of depth ranks skips the three steps above and gathers its
//   tile lists from those ranks: plan_gather below, raster_gather.hip)
//   blend + sums        raster_blend_fwd.hip (launch_blend_fwd); blob layout, environment knobs and the
//                       choice of blend kernels: raster_layout.hip
//
// The arithmetic of preprocess_kernel follows oracle/raster_cpu.py:preprocess op for op
// (this TU is compiled with -ffp-contract=off; IEEE divide / sqrt), so radii, tile
// rectangles and the sort order match the fp32 oracle bit for bit.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <type_traits>

#include "raster_common.hpp"

namespace pings {
namespace raster {

// ---------------------------------------------------------------- kernels
__device__ inline void to_camera(const float* __restrict__ V, float x, float y, float z, float& px,
                                 float& py, float& pz) {
  px = ((V[0] * x + V[4] * y) + V[8] * z) + V[12];
  py = ((V[1] * x + V[5] * y) + V[9] * z) + V[13];
  pz = ((V[2] * x + V[6] * y) + V[10] * z) + V[14];
}

__global__ __launch_bounds__(256) void mark_visible_kernel(const float* __restrict__ pos, int N,
                                                            const float* __restrict__ V,
                                                            const float* __restrict__ Pm,
                                                            uint8_t* __restrict__ present, int depth_only) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float px, py, pz;
  to_camera(V, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], px, py, pz);
  const float hx = ((Pm[0] * px + Pm[4] * py) + Pm[8] * pz) + Pm[12];
  const float hy = ((Pm[1] * px + Pm[5] * py) + Pm[9] * pz) + Pm[13];
  const float hw = ((Pm[3] * px + Pm[7] * py) + Pm[11] * pz) + Pm[15];
  const float pw = 1.0f / (hw + 1e-7f);
  const float nx = hx * pw, ny = hy * pw;
  present[i] = (pz > NEAR_Z) && (depth_only || ((nx >= -1.3f) && (nx <= 1.3f) && (ny >= -1.3f) && (ny <= 1.3f)));
}

// One Gaussian of preprocess_kernel; returns its depth key (CULLED_KEY if it was culled) and the tiles of its rectangle.
template <int MODE>
__device__ inline uint32_t preprocess_gaussian(
    const KParams& p, int g, const float* __restrict__ means3D, const float* __restrict__ colors,
    const float* __restrict__ opacities, const float* __restrict__ scales,
    const float* __restrict__ rotations, float4* __restrict__ rec, uint4* __restrict__ rect,
    uint32_t* __restrict__ depth_key, uint32_t* __restrict__ gidx, int32_t* __restrict__ radii,
    uint32_t& tiles_out) {   // tiles_out: tiles of its rectangle, 0 if it was culled
  const float* V = p.view;
  const float* Pm = p.proj_raw;

  gidx[g] = (uint32_t)g;
  // defaults for a culled Gaussian
  uint32_t key = CULLED_KEY;
  uint4 rc = make_uint4(0u, 0u, 0u, 0u);
  int rad = 0;

  float px, py, pz;
  to_camera(V, means3D[3 * g], means3D[3 * g + 1], means3D[3 * g + 2], px, py, pz);
  bool ok = pz > NEAR_Z;
  // rows of a worst-case sized buffer behind the count the producer left on the device: culled (their contents are
  // never interpreted: every use below is guarded by `ok`)
  if (p.live && g < p.dyn_rows && g >= *p.live) ok = false;

  const float hx = ((Pm[0] * px + Pm[4] * py) + Pm[8] * pz) + Pm[12];
  const float hy = ((Pm[1] * px + Pm[5] * py) + Pm[9] * pz) + Pm[13];
  const float hw = ((Pm[3] * px + Pm[7] * py) + Pm[11] * pz) + Pm[15];
  const float pw = 1.0f / (hw + 1e-7f);
  const float ndx = hx * pw, ndy = hy * pw;
  const float mx = ((ndx + 1.0f) * (float)p.W - 1.0f) * 0.5f;
  const float my = ((ndy + 1.0f) * (float)p.H - 1.0f) * 0.5f;

  const float qr = rotations[4 * g], qx = rotations[4 * g + 1], qy = rotations[4 * g + 2],
              qz = rotations[4 * g + 3];
  const float R00 = 1.0f - 2.0f * (qy * qy + qz * qz), R01 = 2.0f * (qx * qy - qr * qz),
              R02 = 2.0f * (qx * qz + qr * qy);
  const float R10 = 2.0f * (qx * qy + qr * qz), R11 = 1.0f - 2.0f * (qx * qx + qz * qz),
              R12 = 2.0f * (qy * qz - qr * qx);
  const float R20 = 2.0f * (qx * qz - qr * qy), R21 = 2.0f * (qy * qz + qr * qx),
              R22 = 1.0f - 2.0f * (qx * qx + qy * qy);
  const float S0 = p.scale_mod * scales[3 * g], S1 = p.scale_mod * scales[3 * g + 1],
              S2 = p.scale_mod * scales[3 * g + 2];
  const float RS[3][3] = {{R00 * S0, R01 * S1, R02 * S2},
                          {R10 * S0, R11 * S1, R12 * S2},
                          {R20 * S0, R21 * S1, R22 * S2}};
  // Wc[a][b] = V[b][a] = V[4*b + a]
  float Mc[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      Mc[a][k] = (V[a] * RS[0][k] + V[4 + a] * RS[1][k]) + V[8 + a] * RS[2][k];

  const float tx = fminf(p.limx, fmaxf(-p.limx, px / pz)) * pz;
  const float ty = fminf(p.limy, fmaxf(-p.limy, py / pz)) * pz;
  const float J00 = p.fx / pz;
  const float J02 = -(p.fx * tx) / (pz * pz);
  const float J11 = p.fy / pz;
  const float J12 = -(p.fy * ty) / (pz * pz);
  float T0[3], T1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    T0[k] = J00 * Mc[0][k] + J02 * Mc[2][k];
    T1[k] = J11 * Mc[1][k] + J12 * Mc[2][k];
  }
  const float cxx = ((T0[0] * T0[0] + T0[1] * T0[1]) + T0[2] * T0[2]) + LOWPASS;
  const float cxy = (T0[0] * T1[0] + T0[1] * T1[1]) + T0[2] * T1[2];
  const float cyy = ((T1[0] * T1[0] + T1[1] * T1[1]) + T1[2] * T1[2]) + LOWPASS;
  const float det = cxx * cyy - cxy * cxy;
  ok = ok && (det != 0.0f);
  const float det_inv = 1.0f / (det != 0.0f ? det : 1.0f);
  const float conic_x = cyy * det_inv, conic_y = -cxy * det_inv, conic_z = cxx * det_inv;
  const float mid = 0.5f * (cxx + cyy);
  const float lam = mid + sqrtf(fmaxf(mid * mid - det, 0.1f));
  const float radius = ceilf(3.0f * sqrtf(lam));
  ok = ok && isfinite(mx) && isfinite(my) && isfinite(radius);

  float nx = 0.f, ny = 0.f, nz = 0.f, q = 0.f, rz = 0.f;
  if (MODE == MODE_SURFEL) {
    nx = (V[0] * R02 + V[4] * R12) + V[8] * R22;
    ny = (V[1] * R02 + V[5] * R12) + V[9] * R22;
    nz = (V[2] * R02 + V[6] * R12) + V[10] * R22;
    q = (nx * px + ny * py) + nz * pz;
    if (p.front_only) {
      ok = ok && !(q >= 0.0f);
    } else if (q > 0.0f) {
      nx = -nx; ny = -ny; nz = -nz; q = -q;
    }
    rz = 3.0f * fmaxf(S0, S1);
  }

  // Tile rectangle.  Three rules (KParams::rect_rule, PINGS_RASTER_RECT):
  //   RECT_3SIGMA   the published 3DGS getRect(): the square of half-width ceil(3 sqrt(lambda_max)) around the centre,
  //                 upper bound (m + r + TILE - 1) / TILE.
  //   RECT_TIGHT    (default) that square INTERSECTED with the bounding box of the region in which the blend kernels'
  //                 own fp32 evaluation of alpha can reach 1/255.  A tile outside that box holds no pixel that passes
  //                 the alpha test, so dropping it changes no output bit: images, per-Gaussian sums and gradients equal
  //                 RECT_3SIGMA's (tests/test_raster.py::test_default_rectangle_is_lossless).  `radii` is the published
  //                 one: a Gaussian whose square touches the image keeps radius > 0 even if no tile is left.
  //   RECT_ELLIPSE  rounds 1-3: bounding box of the ellipse cut at min(3 sigma, alpha = 1/255) — drops the
  //                 alpha < ~0.011 tail the published rule blends (images differ by up to 3.4e-3); opt-in only.
  // Box of RECT_TIGHT: with the conic (cx, cy, cz) the kernels read, q(d) = cx dx^2 + 2 cy dx dy + cz dy^2 >= sx dx^2,
  // sx = cx - cy^2 / cz (Schur complement; = 1 / cov_xx in exact arithmetic), and the kernels' evaluation q^ of q is
  // off by at most 1e-6 S, S = cx dx^2 + 2 |cy dx dy| + cz dy^2 <= 4 (cx / sx) q (seven roundings of relative 6e-8 on
  // each term; 1e-6 leaves a factor two).  A pixel passes only if q^ <= thr = 2 ln(255 o) (+ 2e-3 for the fast exp /
  // log), hence only if dx^2 <= thr / (sx (1 - 4e-6 cx / sx)).  sx is taken 2e-6 cx low (its own three roundings); a
  // footprint so thin that cx / sx > 1e5 (or a non-finite / non-positive sx) keeps the whole square on that axis.
  const float opac = opacities[g];
  const float k2 = fminf(2.0f * logf(255.0f * opac), 9.0f);
  const bool want = ok;                 // survives culling: `radii` of the published rule depends on the square only
  ok = ok && (k2 > 0.0f || p.rect_rule == RECT_3SIGMA);
  if (want) {
    const bool square = p.rect_rule != RECT_ELLIPSE;
    const float ex = square ? radius : sqrtf(k2 * cxx), ey = square ? radius : sqrtf(k2 * cyy);
    const float up = square ? (float)(TILE - 1) : (float)TILE;
    const float fgx = (float)p.gx, fgy = (float)p.gy;
    int xmin = (int)fminf(fmaxf(floorf((mx - ex) / (float)TILE), 0.0f), fgx);
    int xmax = (int)fminf(fmaxf(floorf(((mx + ex) + up) / (float)TILE), 0.0f), fgx);
    int ymin = (int)fminf(fmaxf(floorf((my - ey) / (float)TILE), 0.0f), fgy);
    int ymax = (int)fminf(fmaxf(floorf(((my + ey) + up) / (float)TILE), 0.0f), fgy);
    const bool sq_tiles = (xmax - xmin) * (ymax - ymin) > 0;
    if (p.rect_rule == RECT_TIGHT) {
      if (sq_tiles) rad = (int)radius;
      if (ok) {
        const float thr = 2.0f * logf(255.0f * opac) + 2e-3f;
        const float sx = (conic_x - (conic_y * conic_y) / conic_z) - 2e-6f * conic_x;
        const float sy = (conic_z - (conic_y * conic_y) / conic_x) - 2e-6f * conic_z;
        const float kx = conic_x / sx, ky = conic_z / sy;
        if (sx > 0.0f && kx <= 1e5f) {   // NaN -> keep the square
          const float bx = sqrtf(thr / (sx * (1.0f - 4e-6f * kx))) * 1.000001f + 1e-3f;
          xmin = max(xmin, (int)fminf(fmaxf(floorf((mx - bx) / (float)TILE), 0.0f), fgx));
          xmax = min(xmax, (int)fminf(fmaxf(floorf(((mx + bx) + (float)TILE) / (float)TILE), 0.0f), fgx));
        }
        if (sy > 0.0f && ky <= 1e5f) {
          const float by = sqrtf(thr / (sy * (1.0f - 4e-6f * ky))) * 1.000001f + 1e-3f;
          ymin = max(ymin, (int)fminf(fmaxf(floorf((my - by) / (float)TILE), 0.0f), fgy));
          ymax = min(ymax, (int)fminf(fmaxf(floorf(((my + by) + (float)TILE) / (float)TILE), 0.0f), fgy));
        }
        xmax = max(xmax, xmin);
        ymax = max(ymax, ymin);
      }
    }
    if (ok) {
      const int tiles = (xmax - xmin) * (ymax - ymin);
      if (tiles > 0) {
        key = __float_as_uint(pz);
        // rect.x: the INNER rectangle of the occlusion-budget pass, as four 8-bit margins inside the tile rectangle
        // (left, right, top, bottom; margins that meet = empty).  A tile adds to the budget only if all of its pixels
        // pass the alpha test (tile_min_alpha > 0), i.e. its four corners lie inside the alpha >= 1/255 ellipse, hence
        // inside that ellipse's bounding box [m - e', m + e'], e' = sqrt(thr cov) with the UNCAPPED thr = 2 ln(255 o)
        // (the tile rectangle itself is cut at 3 sigma).  Typically the rectangle shrinks by a tile on every side —
        // half the pairs of a 7 x 7 rectangle.  The bounds are widened by 0.02 tile against rounding; a Gaussian whose
        // minor semi-axis sqrt(thr lambda_min) is below 7.5 px (threshold 50 = 7.07^2: slack again) cannot hold the
        // 15 x 15 pixel square of a tile at all.
        const float thr_u = 2.0f * logf(opac / p.occ_amin);
        const float lam_min = mid - sqrtf(fmaxf(mid * mid - det, 0.0f));
        uint32_t inner = 0xFFFFFFFFu;   // empty
        if (thr_u * lam_min >= 50.0f) {
          const float exu = sqrtf(thr_u * cxx), eyu = sqrtf(thr_u * cyy);
          const int ix0 = max(xmin, (int)ceilf((mx - exu) / (float)TILE - 0.02f));
          const int ix1 = min(xmax, (int)floorf((mx + exu - 15.0f) / (float)TILE + 0.02f) + 1);
          const int iy0 = max(ymin, (int)ceilf((my - eyu) / (float)TILE - 0.02f));
          const int iy1 = min(ymax, (int)floorf((my + eyu - 15.0f) / (float)TILE + 0.02f) + 1);
          if (ix1 > ix0 && iy1 > iy0)
            inner = (uint32_t)min(ix0 - xmin, 255) | ((uint32_t)min(xmax - ix1, 255) << 8) |
                    ((uint32_t)min(iy0 - ymin, 255) << 16) | ((uint32_t)min(ymax - iy1, 255) << 24);
        }
        const uint32_t covers = inner;
        rc = make_uint4(covers, (uint32_t)xmin | ((uint32_t)ymin << 16),
                        (uint32_t)xmax | ((uint32_t)ymax << 16), (uint32_t)tiles);
        rad = (int)radius;
      }
    }
  }
  depth_key[g] = key;
  rect[g] = rc;
  radii[g] = rad;
  tiles_out = rc.w;
  if (key != CULLED_KEY) {  // nobody reads the record of a culled Gaussian (two thirds of Metric-1's cloud)
    rec[4 * g + 0] = make_float4(mx, my, opac, pz);
    rec[4 * g + 1] = make_float4(conic_x, conic_y, conic_z, rz);
    rec[4 * g + 2] = make_float4(colors[3 * g], colors[3 * g + 1], colors[3 * g + 2], q);
    rec[4 * g + 3] = make_float4(nx, ny, nz, 0.0f);
  }
  return key;
}

// the shard of the frame statistics (STAT_*: raster_common.hpp) this wave adds to
__device__ inline int stat_shard() {
  return (int)((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (STAT_SHARDS - 1));
}

// `ds_head` (bucket depth sort only, else null): the key range of the survivors, as the largest key and the largest
// ~key of every workgroup, each into one of DS_SHARDS words — the keys are in registers here; a pass of its own would
// read them back from HBM.  The header must have been cleared before this launch.
// `stats`: the footprint statistic behind the blend kernels' pixels-per-lane choice, all (Gaussian, tile) pairs before
// occlusion culling and the Gaussians that own one — the rectangle is in registers here, and the sums do not depend
// on the depth order.  Cleared before this launch.
template <int MODE>
__global__ __launch_bounds__(256) void preprocess_kernel(
    KParams p, const float* __restrict__ means3D, const float* __restrict__ colors,
    const float* __restrict__ opacities, const float* __restrict__ scales,
    const float* __restrict__ rotations, float4* __restrict__ rec, uint4* __restrict__ rect,
    uint32_t* __restrict__ depth_key, uint32_t* __restrict__ gidx, int32_t* __restrict__ radii,
    uint32_t* __restrict__ ds_head, unsigned long long* __restrict__ stats) {
  __shared__ uint32_t sm[8];
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t key = CULLED_KEY, tiles = 0u;
  if (g < p.P)
    key = preprocess_gaussian<MODE>(p, g, means3D, colors, opacities, scales, rotations, rec, rect, depth_key, gidx, radii,
                                    tiles);
  {
    const unsigned long long vis = __ballot(tiles != 0u);
    uint32_t tot = tiles;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += (uint32_t)__shfl_xor((int)tot, o, 64);
    if ((threadIdx.x & 63) == 0 && tot) {
      const int shard = stat_shard();
      atomicAdd(stats + STAT_PAIRS + shard, (unsigned long long)tot);
      atomicAdd(stats + STAT_VISIBLE + shard, (unsigned long long)__popcll(vis));
    }
  }
  if (!ds_head) return;
  uint32_t mx = key != CULLED_KEY ? key : 0u, mn = key != CULLED_KEY ? ~key : 0u;  // max key, max ~key over valid entries
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    mn = max(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[wave] = mx; sm[4 + wave] = mn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
    mn = max(max(sm[4], sm[5]), max(sm[6], sm[7]));
    if (mx | mn) {
      atomicMax(&ds_head[blockIdx.x % DS_SHARDS], mx);
      atomicMax(&ds_head[DS_SHARDS + blockIdx.x % DS_SHARDS], mn);
    }
  }
}

constexpr int SMALL_RECT = 8;

// Walks the tile rectangles of the depth-ranked Gaussians: one lane per rank; rectangles of more than SMALL_RECT
// tiles are walked by the whole wave, 64 tiles per step (`coop(src_lane, k, active)` runs in every lane with its
// own tile number k of the source lane's rectangle), the others serially by their lane (`serial(tile)`).
struct RectLane {
  uint32_t g, n;
  int xmin, ymin, wdt, hgt;
};
template <typename Serial, typename CoopBegin, typename Coop>
__device__ inline void walk_rects(const RectLane& me, int gx, Serial serial, CoopBegin coop_begin, Coop coop) {
  const int lane = threadIdx.x & 63;
  if (me.n != 0u && me.n <= (uint32_t)SMALL_RECT) {
    int x = 0, y = 0;
    for (uint32_t k = 0; k < me.n; ++k) {
      serial(me.xmin + x, me.ymin + y);
      if (++x == me.wdt) { x = 0; ++y; }
    }
  }
  unsigned long long m = __ballot(me.n > (uint32_t)SMALL_RECT);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const uint32_t n = lane_value(me.n, src);
    const int x0 = lane_value(me.xmin, src), y0 = lane_value(me.ymin, src), wdt = lane_value(me.wdt, src);
    const float inv_w = 1.0f / (float)wdt;
    coop_begin(src);
    for (uint32_t k0 = 0; k0 < n; k0 += 64) {
      const uint32_t k = k0 + (uint32_t)lane;
      const bool act = k < n;
      // k / wdt without an integer division (k < 2^24: the float quotient is off by at most one)
      int yy = (int)((float)k * inv_w);
      int xx = (int)k - yy * wdt;
      if (xx < 0) { --yy; xx += wdt; }
      if (xx >= wdt) { ++yy; xx -= wdt; }
      coop(src, act ? x0 + xx : 0, act ? y0 + yy : 0, act);
    }
  }
}

// ranks from nvalid on are the culled Gaussians (no tiles): their index and rectangle are not even loaded
__device__ inline RectLane rect_lane(int r, const uint32_t* __restrict__ gidx_sorted, const uint4* __restrict__ rect,
                                     uint32_t nvalid) {
  RectLane me{0u, 0u, 0, 0, 1, 1};
  if (r >= 0 && (uint32_t)r < nvalid) {
    me.g = gidx_sorted[r];
    const uint4 rc = rect[me.g];
    me.n = rc.w;
    me.xmin = (int)(rc.y & 0xFFFF);
    me.ymin = (int)(rc.y >> 16);
    me.wdt = max((int)(rc.z & 0xFFFF) - me.xmin, 1);
    me.hgt = max((int)(rc.z >> 16) - me.ymin, 1);
  }
  return me;
}

// ---------------------------------------------------------------- kept tiles of a rectangle, from the tile bitmasks
// Whether a (Gaussian, tile) pair is kept depends on the Gaussian's rank bucket and the tile alone, and a footprint is
// a full rectangle: occl_scan_kernel writes, for every bucket, the set of tiles that still need it as a bitmask over
// tile ids (GeomState::occ_mask), and the kept tiles of a rectangle row are a bit range of the bucket's mask.  The
// unit of work is an ITEM: up to 64 consecutive tiles of one row (a row wider than 64 tiles is several items), read
// as two neighbouring 8-byte words — one popcount counts them, a walk over the set bits emits them.  Items in
// ascending order, bits in ascending order inside an item: row-major over the rectangle, x ascending — the slot order.
constexpr int SMALL_ITEMS = 16;   // up to this many items a lane walks its rectangle itself, four loads in flight
constexpr uint32_t SMALL_KEPT = 16u;  // duplicate_kernel: up to this many kept tiles the lane also emits them itself

// kept_bits (a bit range of a bucket's mask row): raster_common.hpp

struct RowItems {
  int s0, gx, wdt, cpr;   // first tile id of the rectangle, tiles per image row, rectangle width, items per row
  float inv_cpr;
  __device__ RowItems(int xmin, int ymin, int wdt_, int gx_)
      : s0(ymin * gx_ + xmin), gx(gx_), wdt(wdt_), cpr((wdt_ + 63) >> 6), inv_cpr(1.0f / (float)((wdt_ + 63) >> 6)) {}
  // first tile id and width of item k
  __device__ void at(uint32_t k, int& s, int& w) const {
    int y = (int)k, c = 0;
    if (cpr > 1) {   // k / cpr without an integer division (k < 2^24: the float quotient is off by at most one)
      y = (int)((float)k * inv_cpr);
      c = (int)k - y * cpr;
      if (c < 0) { --y; c += cpr; }
      if (c >= cpr) { ++y; c -= cpr; }
    }
    s = s0 + y * gx + 64 * c;
    w = min(64, wdt - 64 * c);
  }
};

__device__ inline uint32_t rect_items(const RectLane& me) {
  return me.n != 0u ? (uint32_t)(me.hgt * ((me.wdt + 63) >> 6)) : 0u;
}

// `serial(s, bits)` for every item of this lane's own rectangle, in order
template <typename Serial>
__device__ inline void walk_items_serial(const RectLane& me, uint32_t items, int gx,
                                         const unsigned long long* __restrict__ mrow, Serial serial) {
  const RowItems ri(me.xmin, me.ymin, me.wdt, gx);
  for (uint32_t k0 = 0; k0 < items; k0 += 4) {
    int s[4];
    unsigned long long b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int w;
      ri.at(min(k0 + (uint32_t)u, items - 1u), s[u], w);
      b[u] = kept_bits(mrow, s[u], w);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k0 + (uint32_t)u < items) serial(s[u], b[u]);
  }
}

// The rectangles of the lanes in `big`, one after the other, by the whole wave: lane l takes items l, l + 64, ... of
// the source lane's rectangle.  `begin(src)` once per rectangle, then `step(s, bits)` in every lane for every 64
// items (bits = 0 in a lane without an item).
template <typename Begin, typename Step>
__device__ inline void walk_items_coop(unsigned long long big, const RectLane& me, uint32_t items, int gx, uint32_t bk,
                                       const unsigned long long* __restrict__ mask, int words, Begin begin, Step step) {
  const int lane = threadIdx.x & 63;
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    const uint32_t n = lane_value(items, src);
    const RowItems ri(lane_value(me.xmin, src), lane_value(me.ymin, src), lane_value(me.wdt, src), gx);
    const unsigned long long* mrow = mask + (size_t)lane_value(bk, src) * words;
    begin(src);
    for (uint32_t k0 = 0; k0 < n; k0 += 64) {
      const uint32_t k = k0 + (uint32_t)lane;
      int sk = 0, w = 1;
      unsigned long long bits = 0ull;
      if (k < n) {
        ri.at(k, sk, w);
        bits = kept_bits(mrow, sk, w);
      }
      step(sk, bits);
    }
  }
}

// ---------------------------------------------------------------- occlusion culling of instances
// A tile whose every pixel has stopped (transmittance test, T_EPS) ignores the rest of its list.  Before any
// instance is created, a CONSERVATIVE per-tile bound finds a depth rank beyond which that is certain:
//   * for a (Gaussian, tile) pair, a_min = lower bound of the alpha the blend kernel gives ANY pixel of the tile
//     (largest q at the tile corners, fp32 error margins included; 0 if some pixel might be rejected by the
//     alpha >= 1/255 or power <= 0 tests, in particular for the tile that holds the centre);
//   * -ln(1 - a_min) is added (fixed point, integer atomics: order independent, hence reproducible) to the budget
//     of (tile, rank bucket); ranks are the depth order, OCC buckets per tile;
//   * the first bucket at which the running budget reaches OCC_THR > -ln(T_EPS) is the last one the tile needs:
//     whatever alphas the other Gaussians add, every pixel has met T (1 - alpha) < T_EPS by then.
// Instances of later buckets are never created: the sort, the per-instance arrays and the staging of the blend
// kernels shrink to the lists that can matter (Metric-1: 16.9 M -> 1.8 M), and every output stays bit-identical,
// because a culled instance would never have been blended.  The kept list of a tile is a prefix of its full list.
// tile_min_alpha itself: raster_common.hpp (the blend kernels' interior test rests on it as well).

// ---------------------------------------------------------------- depth order of the preprocessed Gaussians
// A library radix / merge sort of P = 1M (key, index) pairs costs 20 launches and 150 us, more than the preprocess
// pass itself, although only the ~30 % that survive culling need an order.  Here: the key range of the survivors
// (two atomics per wave) -> 2^18 equal-width buckets of the KEY BITS (monotone in depth; positive floats order as
// integers) -> histogram -> exclusive scan -> scatter in arrival order -> every element ranks itself among its
// bucket mates by (key, index), which is the stable order of a full sort, whatever the arrival order was: the result
// is bit-identical to the library sort.  Culled Gaussians fill ranks [nvalid, P) in any order (they own no tiles; the
// per-rank kernels only need a permutation).  Buckets average a handful of elements; one beyond DS_LIMIT (many
// Gaussians at exactly one depth) raises a flag the host reads at its one synchronisation point and the library
// sort redoes the frame.
struct DsRange { uint32_t kmin, shift; };

// what ds_hist_kernel published (ds_scatter_kernel, ds_rank_kernel)
__device__ inline DsRange ds_range(const uint32_t* __restrict__ head) { return DsRange{head[DS_KMIN], head[DS_SHIFT]}; }

// The range from preprocess_kernel's shards: every workgroup of ds_hist_kernel folds the 2 x DS_SHARDS words itself
// (L2-resident; a one-wave kernel in between cost a launch) — its first wave, the others get the result through LDS.
__device__ inline DsRange ds_range_from_shards(const uint32_t* __restrict__ head, uint32_t (&sr)[2]) {
  if (threadIdx.x < 64) {
    uint32_t mx = head[threadIdx.x], mn = head[DS_SHARDS + threadIdx.x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
      mn = max(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
    }
    if (threadIdx.x == 0) {
      const uint32_t kmin = ~mn;
      uint32_t shift = 0u;
      if (mx > kmin)
        while (((mx - kmin) >> shift) >= (uint32_t)DS_NB) ++shift;
      sr[0] = kmin;
      sr[1] = shift;
    }
  }
  __syncthreads();
  return DsRange{sr[0], sr[1]};
}

// bucket histogram of the survivors; culled Gaussians are counted per workgroup (cnt[DS_NB + block]) so that the one
// exclusive scan over [bucket counts | per-block culled counts] also yields each block's first culled rank.
// The histogram atomics are aggregated per wave: lanes that fall into the same bucket elect a leader (pure ALU
// rounds: ballot of the lanes equal to the first unassigned one), the leaders issue ONE returning atomic per distinct
// bucket, all in flight together, and every lane derives its arrival slot inside the bucket (`pos`) from the leader's
// return value.  A wall of surfels at one depth — a quarter of a million Gaussians in one bucket — would otherwise
// serialise on one address (~12 ns per atomic: 3 ms); the scatter pass needs no atomics at all.
// Workgroup 0 also publishes the key range (head[DS_KMIN], head[DS_SHIFT]) for the two passes that follow.
__global__ __launch_bounds__(256) void ds_hist_kernel(int P, const uint32_t* __restrict__ key, uint32_t* __restrict__ head,
                                                       uint32_t* __restrict__ cnt, uint32_t* __restrict__ pos) {
  __shared__ uint32_t sc[4];
  __shared__ uint32_t sr[2];
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t k = g < P ? key[g] : 0u;
  const bool culled = g < P && k == CULLED_KEY;
  const bool active = g < P && !culled;
  const DsRange r = ds_range_from_shards(head, sr);
  if (blockIdx.x == 0 && threadIdx.x == 0) { head[DS_KMIN] = r.kmin; head[DS_SHIFT] = r.shift; }
  const uint32_t b = active ? (k - r.kmin) >> r.shift : 0xFFFFFFFFu;
  unsigned long long todo = __ballot(active);
  const unsigned long long below = (1ull << lane) - 1ull;
  int my_leader = lane;
  uint32_t my_rank = 0u, group = 0u;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)b, leader);
    const unsigned long long m = __ballot(b == lb) & todo;
    if (b == lb) {
      my_leader = leader;
      my_rank = (uint32_t)__popcll(m & below);
      group = (uint32_t)__popcll(m);
    }
    todo &= ~m;
  }
  uint32_t base = 0u;
  if (active && my_leader == lane) base = atomicAdd(&cnt[b], group);
  base = (uint32_t)__shfl((int)base, my_leader, 64);
  if (active) pos[g] = base + my_rank;
  const unsigned long long bal = __ballot(culled);
  if (lane == 0) sc[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) cnt[DS_NB + blockIdx.x] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
}

__global__ __launch_bounds__(256) void ds_scatter_kernel(int P, const uint32_t* __restrict__ key, const uint32_t* __restrict__ head,
                                                          const uint32_t* __restrict__ off, const uint32_t* __restrict__ pos,
                                                          uint32_t* __restrict__ tmp_key, uint32_t* __restrict__ tmp_idx,
                                                          uint32_t* __restrict__ gidx_sorted) {
  __shared__ uint32_t sc[4];
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t k = g < P ? key[g] : 0u;
  const bool culled = g < P && k == CULLED_KEY;
  if (g < P && !culled) {
    const DsRange r = ds_range(head);
    const uint32_t b = (k - r.kmin) >> r.shift;
    const uint32_t slot = off[b] + pos[g];
    tmp_key[slot] = k;
    tmp_idx[slot] = (uint32_t)g;
  }
  // culled Gaussians take ranks [nvalid, P) in index order
  const unsigned long long bal = __ballot(culled);
  if (lane == 0) sc[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  if (culled) {
    uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += sc[w];
    gidx_sorted[off[DS_NB + blockIdx.x] + before] = (uint32_t)g;
  }
}

__global__ __launch_bounds__(256) void ds_rank_kernel(const uint32_t* __restrict__ tmp_key, const uint32_t* __restrict__ tmp_idx,
                                                       uint32_t* __restrict__ head, const uint32_t* __restrict__ off,
                                                       uint32_t* __restrict__ gidx_sorted, uint32_t* __restrict__ rank_of,
                                                       uint32_t* __restrict__ nvalid) {
  const uint32_t n = off[DS_NB];
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s == 0u) *nvalid = n;
  if (s >= n) return;
  const uint32_t k = tmp_key[s], id = tmp_idx[s];
  const DsRange r = ds_range(head);
  const uint32_t b = (k - r.kmin) >> r.shift;
  const uint32_t lo = off[b], hi = off[b + 1];
  if (hi - lo > DS_LIMIT) {  // degenerate depth distribution: keep a valid permutation, let the host redo the sort
    gidx_sorted[s] = id;
    rank_of[id] = s;
    if (s == lo) head[DS_FLAG] = 1u;
    return;
  }
  uint32_t rank = 0u;
  uint32_t t = lo;
  // eight bucket mates per round trip: a crowded bucket (a wall of surfels at one depth: hundreds of mates) made this
  // loop one dependent load latency per mate
  for (; t + 8u <= hi; t += 8u) {
    uint32_t kt[8], it[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { kt[u] = tmp_key[t + u]; it[u] = tmp_idx[t + u]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) rank += (kt[u] < k || (kt[u] == k && it[u] < id)) ? 1u : 0u;
  }
  for (; t < hi; ++t) {
    const uint32_t kt = tmp_key[t], it = tmp_idx[t];
    rank += (kt < k || (kt == k && it < id)) ? 1u : 0u;
  }
  gidx_sorted[lo + rank] = id;
  rank_of[id] = lo + rank;
}

__global__ __launch_bounds__(256) void invert_perm_kernel(int P, const uint32_t* __restrict__ gidx_sorted,
                                                           uint32_t* __restrict__ rank_of) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < P) rank_of[gidx_sorted[r]] = (uint32_t)r;
}

// ranks [0, nvalid) hold the Gaussians with a real depth key (culled ones sort last): first culled rank,
// found by one wave with a 64-ary search (4 dependent rounds for any P < 2^24, instead of 20+)
__global__ __launch_bounds__(64) void count_valid_kernel(int P, const uint32_t* __restrict__ depth_key_sorted,
                                                         uint32_t* __restrict__ nvalid) {
  const int lane = threadIdx.x;
  long long lo = 0, hi = P;  // invariant: keys below lo are valid, keys from hi on are culled
  while (lo < hi) {
    const long long span = hi - lo;
    const long long step = (span + 63) / 64;
    const long long pos = lo + (long long)lane * step;
    const bool valid = pos < hi && depth_key_sorted[pos] < CULLED_KEY;
    const int nv = __popcll(__ballot(valid));  // probes are ascending: the valid ones form a prefix
    if (nv == 0) { hi = lo; break; }
    const long long last_valid = lo + (long long)(nv - 1) * step;
    lo = last_valid + 1;
    hi = min(hi, last_valid + step);
  }
  if (lane == 0) *nvalid = (uint32_t)lo;
}

// rank_bucket (the rank bucket of a depth rank): raster_common.hpp

// The budget pass.  A lane owns one depth rank: its inner rectangle, the six record values tile_min_alpha reads and its
// rank bucket.  DENSE (the product): the (rank, tile) pairs of the workgroup's 256 ranks are numbered through — one
// exclusive sum of the inner-tile counts, inside the wave and then over the four wave totals in LDS, one barrier — and
// thread t takes pairs t, t + 256, ...: every lane of every step has a pair until the workgroup's last step, whatever
// the rectangle sizes.  The owner of pair p is the last rank whose offset is <= p: its wave from three compares with
// the wave bases, then three 16-byte probes in LDS (the offsets of every 16th, every 4th and every rank of that wave,
// four at a time: half the dependent round trips of a binary search); what a pair needs of its owner is nine words of
// LDS (corner and width packed, the reciprocal width — one correctly rounded divide per rank instead of one per pair
// — the bucket and the six record values).  A workgroup without a pair (most of those behind nvalid) ends after the
// barrier.  !DENSE (PINGS_OCC_WALK=l): the dealing of walk_rects — a lane walks a rectangle of up to SMALL_RECT tiles
// itself, the wave walks the larger ones one after the other.  The same pairs, the same arithmetic per pair and
// integer atomics: the budget table is the same words either way.
template <bool DENSE>
__global__ __launch_bounds__(256) void occl_budget_kernel(int P, int gx, int nb,
                                                          const uint32_t* __restrict__ gidx_sorted,
                                                          const uint4* __restrict__ rect,
                                                          const float4* __restrict__ rec,
                                                          const uint32_t* __restrict__ nvalid, int num_tiles,
                                                          uint32_t* __restrict__ bucket) {
  const int r = strided_rank(P);
  const uint32_t nv = *nvalid;
  RectLane me = rect_lane(r, gidx_sorted, rect, nv);
  if (me.n != 0u) {   // walk only the inner rectangle (preprocess_kernel): tiles outside it cannot be covered
    const uint4 rc = rect[me.g];
    const int x0 = me.xmin + (int)(rc.x & 255u), x1 = (int)(rc.z & 0xFFFF) - (int)((rc.x >> 8) & 255u);
    const int y0 = me.ymin + (int)((rc.x >> 16) & 255u), y1 = (int)(rc.z >> 16) - (int)(rc.x >> 24);
    if (x1 > x0 && y1 > y0) {
      me.xmin = x0; me.ymin = y0; me.wdt = x1 - x0; me.hgt = y1 - y0; me.n = (uint32_t)((x1 - x0) * (y1 - y0));
    } else {
      me.n = 0u;
    }
  }
  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
  if (me.n != 0u) {
    ra = rec[4 * (size_t)me.g + 0];
    rb = rec[4 * (size_t)me.g + 1];
  }
  const uint32_t bk = rank_bucket(r, nb, nv);
  // bucket-major layout: the 64 tiles a wave handles in one step are neighbours in a tile row, so its atomics
  // hit contiguous words (scattered 4-byte atomics run an order of magnitude slower)
  auto add = [&](int tx, int ty, float mx, float my, float o, float cx, float cy, float cz, uint32_t b) {
    const float a = tile_min_alpha(mx, my, o, cx, cy, cz, (float)(tx * TILE), (float)(ty * TILE));
    if (a > 0.f)
      atomicAdd(&bucket[(size_t)b * num_tiles + (ty * gx + tx)], (uint32_t)(-__logf(1.f - a) * OCC_FIX));
  };
  if constexpr (!DENSE) {
    float smx = 0, smy = 0, so = 0, scx = 0, scy = 0, scz = 0;
    uint32_t sb = 0;
    walk_rects(
        me, gx, [&](int tx, int ty) { add(tx, ty, ra.x, ra.y, ra.z, rb.x, rb.y, rb.z, bk); },
        [&](int src) {
          smx = lane_value(ra.x, src); smy = lane_value(ra.y, src); so = lane_value(ra.z, src);
          scx = lane_value(rb.x, src); scy = lane_value(rb.y, src); scz = lane_value(rb.z, src);
          sb = lane_value(bk, src);
        },
        [&](int, int tx, int ty, bool act) { if (act) add(tx, ty, smx, smy, so, scx, scy, scz, sb); });
  } else {
    // first pair of a rank, counted from its wave's first pair: of every 16th rank, of every 4th and of every rank
    __shared__ alignas(16) uint32_t sOff16[16], sOff4[64], sOff[256];
    __shared__ uint32_t sTot[4];     // pairs per wave
    __shared__ uint4 sGeo[256];      // xmin | ymin << 16, wdt | bucket << 16, 1 / wdt, conic z
    __shared__ float4 sRec[256];     // mean x, mean y, opacity, conic x
    __shared__ float sCy[256];       // conic y
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t incl = wave_inclusive_sum_dpp(me.n);
    sOff[t] = incl - me.n;
    if ((t & 3) == 0) sOff4[t >> 2] = incl - me.n;
    if ((t & 15) == 0) sOff16[t >> 4] = incl - me.n;
    if (lane == 63) sTot[wave] = incl;
    if (me.n != 0u) {
      sGeo[t] = make_uint4((uint32_t)me.xmin | ((uint32_t)me.ymin << 16), (uint32_t)me.wdt | (bk << 16),
                           __float_as_uint(1.0f / (float)me.wdt), __float_as_uint(rb.z));
      sRec[t] = make_float4(ra.x, ra.y, ra.z, rb.x);
      sCy[t] = rb.y;
    }
    __syncthreads();
    const uint32_t b1 = sTot[0], b2 = b1 + sTot[1], b3 = b2 + sTot[2], total = b3 + sTot[3];
    for (uint32_t p = (uint32_t)t; p < total; p += 256u) {
      // equal bases (a wave without a pair) and equal offsets (a rank without one) resolve to the last of them
      const int w = (int)(p >= b1) + (int)(p >= b2) + (int)(p >= b3);
      const uint32_t q = p - (w == 0 ? 0u : w == 1 ? b1 : w == 2 ? b2 : b3);
      // three 16-byte probes, four offsets each: the first of a group is <= q, so the count of those <= q, less one,
      // is the last of them
      auto last4 = [q](uint4 o) { return (int)(o.y <= q) + (int)(o.z <= q) + (int)(o.w <= q); };
      int own = 4 * w + last4(reinterpret_cast<const uint4*>(sOff16)[w]);
      own = 4 * own + last4(reinterpret_cast<const uint4*>(sOff4)[own]);
      const uint4 o1 = reinterpret_cast<const uint4*>(sOff)[own];
      const int j = last4(o1);
      own = 4 * own + j;
      const uint32_t k = q - (j == 0 ? o1.x : j == 1 ? o1.y : j == 2 ? o1.z : o1.w);
      const uint4 ge = sGeo[own];
      const float4 re = sRec[own];
      const float cy = sCy[own];
      const int wdt = (int)(ge.y & 0xFFFFu);
      // k / wdt without an integer division (k < 2^24: the float quotient is off by at most one)
      int yy = (int)((float)k * __uint_as_float(ge.z));
      int xx = (int)k - yy * wdt;
      if (xx < 0) { --yy; xx += wdt; }
      if (xx >= wdt) { ++yy; xx -= wdt; }
      add((int)(ge.x & 0xFFFFu) + xx, (int)(ge.x >> 16) + yy, re.x, re.y, re.z, re.w, cy, __uint_as_float(ge.w),
          ge.y >> 16);
    }
  }
}

// Running budget over the rank buckets -> last bucket a tile needs.  A 512-thread workgroup takes 64 tiles x 8
// bucket groups: thread (tile, g) loads its group's buckets (coalesced across the 64 tiles, all loads independent),
// the group sums meet in LDS, and the group in which the running sum crosses the threshold finds the bucket.
// Epilogue: the tile bitmasks of the row walks.  The workgroup's 64 tiles are one word of every bucket's mask
// (word blockIdx.x of `words` = gridDim.x): wave g ballots `bucket <= bsat` for each bucket of its group and lane u
// stores the word of the group's bucket u.  Bits of tiles from num_tiles on are 0.  With the budget all zero (the
// occlusion bound switched off) every tile comes out as OCC_ALL and every mask as all ones.  `bmax` (zero before the
// launch) receives the largest last needed bucket over the tiles, nb - 1 as soon as one tile never saturates.
__global__ __launch_bounds__(512) void occl_scan_kernel(int num_tiles, int nb, const uint32_t* __restrict__ bucket,
                                                        uint16_t* __restrict__ bsat,
                                                        unsigned long long* __restrict__ mask,
                                                        uint32_t* __restrict__ bmax) {
  __shared__ uint32_t sSum[8][64];
  __shared__ uint32_t sSat[64];
  const int t = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int tile = blockIdx.x * 64 + t;
  const int per = nb / 8;  // nb is a power of two >= 32
  const uint32_t thr = (uint32_t)(OCC_THR * OCC_FIX);
  uint32_t v[32];
  uint32_t sum = 0;
#pragma unroll
  for (int u = 0; u < 32; ++u) {
    v[u] = (u < per && tile < num_tiles) ? min(bucket[(size_t)(g * per + u) * num_tiles + tile], thr) : 0u;
    sum += v[u];
  }
  sSum[g][t] = min(sum, thr);
  __syncthreads();
  uint32_t before = 0;
  for (int k = 0; k < g; ++k) before += sSum[k][t];
  const uint32_t total = before + sSum[g][t];
  if (tile < num_tiles) {
    if (g == 7 && total < thr) {  // never saturates: the last group sees the full sum
      bsat[tile] = OCC_ALL;
      sSat[t] = OCC_ALL;
    }
    if (before < thr && total >= thr) {               // exactly one group crosses the threshold
      uint32_t run = before;
      int res = -1;
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        run += v[u];
        if (res < 0 && run >= thr) res = u;
      }
      bsat[tile] = (uint16_t)(g * per + res);
      sSat[t] = (uint32_t)(g * per + res);
    }
  }
  __syncthreads();
  const uint32_t sat = tile < num_tiles ? sSat[t] : 0u;
  if (g == 0) {   // the last bucket any tile needs (count_kept_kernel): an integer maximum, order independent
    uint32_t m = min(sat, (uint32_t)nb - 1u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if (t == 0) atomicMax(bmax, m);
  }
  unsigned long long word = 0ull;
  for (int u = 0; u < per; ++u) {
    const unsigned long long w = __ballot(tile < num_tiles && (uint32_t)(g * per + u) <= sat);
    if (t == u) word = w;
  }
  if (t < per) mask[(size_t)(g * per + t) * gridDim.x + blockIdx.x] = word;
}

// kept tiles per depth rank (the Gaussian's rank bucket must not exceed the tile's last needed bucket).  A rank whose
// bucket lies behind the last one ANY tile needs (occl_scan_kernel's bmax) keeps nothing and walks nothing: where every
// tile saturates (the headline, closed rooms) that is most of the visible Gaussians; where one tile sees sky bmax is
// nb - 1 and nothing changes.  Such a rank loads neither its Gaussian's index nor its rectangle: it stores its zero and
// is done (the footprint statistics, which count every pair, are preprocess_kernel's).
__global__ __launch_bounds__(256) void count_kept_kernel(int P, int gx, int nb, int words,
                                                         const uint32_t* __restrict__ gidx_sorted,
                                                         const uint4* __restrict__ rect,
                                                         const unsigned long long* __restrict__ mask,
                                                         const uint32_t* __restrict__ nvalid,
                                                         const uint32_t* __restrict__ bmax,
                                                         uint32_t* __restrict__ tiles_sorted,
                                                         unsigned long long* __restrict__ stats) {
  const int r = strided_rank(P);
  const int lane = threadIdx.x & 63;
  const uint32_t nv = *nvalid;
  const uint32_t bk = rank_bucket(r, nb, nv);
  const RectLane me = rect_lane(bk <= *bmax ? r : -1, gidx_sorted, rect, nv);
  const uint32_t items = rect_items(me);
  uint32_t kept = 0, acc = 0;
  if (items != 0u && items <= (uint32_t)SMALL_ITEMS)
    walk_items_serial(me, items, gx, mask + (size_t)bk * words,
                      [&](int, unsigned long long bits) { kept += (uint32_t)__popcll(bits); });
  int cur = -1;
  auto flush = [&]() {   // the finished rectangle's count, summed over the wave, to its lane
    if (cur < 0) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += (uint32_t)__shfl_xor((int)acc, off, 64);
    if (lane == cur) kept = acc;
  };
  walk_items_coop(
      __ballot(items > (uint32_t)SMALL_ITEMS), me, items, gx, bk, mask, words,
      [&](int src) { flush(); cur = src; acc = 0; },
      [&](int, unsigned long long bits) { acc += (uint32_t)__popcll(bits); });
  flush();
  if (r >= 0) tiles_sorted[r] = kept;
  // the kept total once more in 64 bits: the instance offsets are a 32-bit scan, which a degenerate frame (huge
  // footprints with the occlusion bound off) could wrap without anyone noticing
  uint32_t kept_w = r >= 0 ? kept : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kept_w += (uint32_t)__shfl_xor((int)kept_w, off, 64);
  if (lane == 0 && kept_w) atomicAdd(stats + STAT_KEPT + stat_shard(), (unsigned long long)kept_w);
}

// Emits the kept (tile id, slot) instances in depth order; gval[slot] = Gaussian id.  A Gaussian that keeps nothing
// (count_kept_kernel's count) is not walked at all; one that keeps more than SMALL_KEPT tiles, or has more than
// SMALL_ITEMS items, is emitted by the whole wave: the items' bits in parallel, then one store step per non-empty
// item, lane i taking bit i (consecutive slots: the stores of a step are contiguous).
template <typename KeyT>
__global__ __launch_bounds__(256) void duplicate_kernel(int P, int gx, int nb, int words,
                                                         const uint32_t* __restrict__ gidx_sorted,
                                                         const uint32_t* __restrict__ offsets_sorted,
                                                         const uint32_t* __restrict__ tiles_sorted,
                                                         const uint4* __restrict__ rect,
                                                         const unsigned long long* __restrict__ mask,
                                                         const uint32_t* __restrict__ nvalid,
                                                         KeyT* __restrict__ tile_key,
                                                         uint32_t* __restrict__ gval,
                                                         uint32_t* __restrict__ per_gaussian) {
  // the zeros of the per-Gaussian sums (per_gaussian_sum_kernel stores only where a Gaussian kept a tile): one
  // coalesced word per thread, in Gaussian order — the launch has one thread per Gaussian anyway
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P) per_gaussian[i] = 0u;
  const int r = strided_rank(P);
  const int lane = threadIdx.x & 63;
  // the kept count first (one coalesced word): the ranks that keep nothing — on the headline all but one in a
  // hundred of the survivors — load neither index, rectangle nor offset
  const uint32_t kept = r >= 0 ? tiles_sorted[r] : 0u;
  const uint32_t nv = *nvalid;
  const RectLane me = rect_lane(kept != 0u ? r : -1, gidx_sorted, rect, nv);
  const uint32_t bk = kept != 0u ? rank_bucket(r, nb, nv) : 0u;
  uint32_t o = kept != 0u ? offsets_sorted[r] - kept : 0u;  // first slot of this Gaussian
  const uint32_t items = rect_items(me);
  const bool coop = items > (uint32_t)SMALL_ITEMS || kept > SMALL_KEPT;
  if (items != 0u && !coop)
    walk_items_serial(me, items, gx, mask + (size_t)bk * words, [&](int s, unsigned long long bits) {
      while (bits) {
        tile_key[o] = (KeyT)(s + __builtin_ctzll(bits));
        gval[o] = me.g;
        ++o;
        bits &= bits - 1;
      }
    });
  uint32_t so = 0, sg = 0;
  walk_items_coop(
      __ballot(items != 0u && coop), me, items, gx, bk, mask, words,
      [&](int src) {
        so = lane_value(o, src);
        sg = lane_value(me.g, src);
      },
      [&](int s, unsigned long long bits) {
        unsigned long long todo = __ballot(bits != 0ull);
        while (todo) {
          const int j = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const uint32_t blo = lane_value((uint32_t)bits, j), bhi = lane_value((uint32_t)(bits >> 32), j);
          const int sj = lane_value(s, j);
          if (((lane < 32 ? blo : bhi) >> (lane & 31)) & 1u) {
            const uint32_t pos = so + __builtin_amdgcn_mbcnt_hi(bhi, __builtin_amdgcn_mbcnt_lo(blo, 0u));
            tile_key[pos] = (KeyT)(sj + lane);
            gval[pos] = sg;
          }
          so += (uint32_t)(__popc(blo) + __popc(bhi));
        }
      });
}

// ---------------------------------------------------------------- longest-processing-time-first tile dispatch
// tile_order_body: raster_common.hpp
template <bool FROM_RANGES>
__global__ __launch_bounds__(1024) void tile_order_kernel(const uint32_t* __restrict__ work_in,
                                                          const uint2* __restrict__ ranges, int num_tiles,
                                                          uint32_t* __restrict__ order, uint32_t* __restrict__ n_long,
                                                          uint32_t long_thr, uint32_t long_max) {
  tile_order_body<FROM_RANGES>(work_in, ranges, num_tiles, order, n_long, long_thr, long_max);
}

int launch_tile_order(const uint32_t* work, int num_tiles, uint32_t* order, hipStream_t st, uint32_t* n_long,
                      uint32_t long_thr, uint32_t long_max) {
  hipLaunchKernelGGL(tile_order_kernel<false>, dim3(1), dim3(1024), 0, st, work, (const uint2*)nullptr, num_tiles, order,
                     n_long, long_thr, long_max);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

template <typename KeyT>
__global__ __launch_bounds__(256) void tile_ranges_kernel(int64_t I, const KeyT* __restrict__ key,
                                                           uint2* __restrict__ ranges) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const uint32_t t = (uint32_t)key[i];
  if (i == 0 || key[i - 1] != t) ranges[t].x = (uint32_t)i;
  if (i == I - 1 || key[i + 1] != t) ranges[t].y = (uint32_t)(i + 1);
}

// One wave folds everything the host reads at the frame's one synchronisation into a 64-byte record: depth-sort
// overflow flag, the three sharded statistics and up to 8 caller words (counts other kernels of the frame
// left on the device: pings_raster_preprocess_dyn).
constexpr int FRONT_SCAN_STEPS = 16;   // frame_summary_kernel: steps of 256 ranks it looks back for the last keeper
enum { FRONT_NEVER = 0, FRONT_CLASS2 = 1, FRONT_ALWAYS = 2 };   // when frame_summary_kernel looks for the front depth
struct AuxPtrs {
  const int32_t* p[8];
};
__global__ __launch_bounds__(64) void frame_summary_kernel(const uint32_t* __restrict__ overflow,
                                                           const unsigned long long* __restrict__ shards, AuxPtrs aux,
                                                           int aux_words, FrameSummary* __restrict__ out, uint32_t seq,
                                                           int nb, const uint32_t* __restrict__ nvalid,
                                                           const uint32_t* __restrict__ bmax,
                                                           const uint32_t* __restrict__ tiles_sorted,
                                                           uint32_t* __restrict__ front, int front_mode) {
  __shared__ unsigned long long part[3][64];
  __shared__ unsigned long long tot[3];
  const int lane = threadIdx.x;
  unsigned long long a0 = 0, a1 = 0, a2 = 0;
  for (int i = lane; i < STAT_SHARDS; i += 64) {
    a0 += shards[STAT_PAIRS + i]; a1 += shards[STAT_VISIBLE + i]; a2 += shards[STAT_KEPT + i];
  }
  part[0][lane] = a0; part[1][lane] = a1; part[2][lane] = a2;
  __syncthreads();
  if (lane < 3) {
    unsigned long long t = 0;
    for (int i = 0; i < 64; ++i) t += part[lane][i];
    out->stats[lane] = t;
    tot[lane] = t;
  }
  __syncthreads();
  if (lane == 4) out->overflow = overflow ? *overflow : 0u;
  // Only for a frame whose render may gather (front_mode FRONT_NEVER: PINGS_BIN=s; FRONT_CLASS2: the default rule, which
  // gathers footprint class 2 alone — the host's own test on the same two sums; FRONT_ALWAYS: PINGS_BIN=g).  Every
  // other frame (C2, C3: class 1) stores FRONT_UNKNOWN, which no plan accepts, and this wave, which the host is waiting
  // for, does what it did before there was a front depth.
  const bool want_front = front_mode == FRONT_ALWAYS || (front_mode == FRONT_CLASS2 && tot[1] > 0ull && tot[0] > 16ull * tot[1]);
  if (!want_front) {
    if (lane == 5) { out->front = FRONT_UNKNOWN; *front = FRONT_UNKNOWN; }
  } else {
    // The front depth of the frame: 1 + the last depth rank that keeps a tile.  No rank in a bucket behind occ_bmax
    // keeps one, so the ranks of the buckets up to it bound the front (the bucket map is monotone: a search);
    // from there the kept counts are read backwards, 256 ranks a step, until one is non-zero — the first step where
    // tiles saturate, since the last needed bucket is a few hundred ranks wide.  After FRONT_SCAN_STEPS empty steps the
    // bound itself stands: every use of the front depth (raster_gather.hip) only needs no keeper at or behind it.
    const uint32_t nv = *nvalid, bm = *bmax;
    // smallest rank whose bucket lies behind bm (nv if there is none), by a 64-ary search as in count_valid_kernel:
    // ranks below lo have a bucket up to bm, ranks from hi on one behind it
    uint32_t lo = 0u, hi = nv;
    if (bm + 1u >= (uint32_t)nb) lo = nv;   // a tile never saturates: every bucket is needed, nothing to search
    while (lo < hi) {
      const uint32_t step = (hi - lo + 63u) / 64u;
      const uint32_t pos = lo + (uint32_t)lane * step;
      const bool le = pos < hi && rank_bucket((int)pos, nb, nv) <= bm;
      const int nle = __popcll(__ballot(le));   // probes ascend and the map is monotone: these form a prefix
      if (nle == 0) { hi = lo; break; }
      const uint32_t last_le = lo + (uint32_t)(nle - 1) * step;
      lo = last_le + 1u;
      hi = min(hi, last_le + step);
    }
    uint32_t fr = lo;
    for (int step = 0; step < FRONT_SCAN_STEPS && fr > 0u; ++step) {
      const uint32_t base = fr > 256u ? fr - 256u : 0u;
      uint32_t last = 0u;   // 1 + the last keeper among this lane's ranks base + lane, + 64, ..
#pragma unroll
      for (uint32_t u = 0u; u < 4u; ++u) {
        const uint32_t r = base + 64u * u + (uint32_t)lane;
        if (r < fr && tiles_sorted[r] != 0u) last = r + 1u;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) last = max(last, (uint32_t)__shfl_xor((int)last, o, 64));
      if (last != 0u) { fr = last; break; }
      if (base == 0u) { fr = 0u; break; }
      if (step + 1 < FRONT_SCAN_STEPS) fr = base;
      else fr = lo;
    }
    if (lane == 5) { out->front = fr; *front = fr; }
  }
  if (lane >= 8 && lane < 16) out->aux[lane - 8] = (lane - 8 < aux_words && aux.p[lane - 8]) ? *aux.p[lane - 8] : 0;
  // `out` is pinned HOST memory: every field first, then the sequence number with system-scope release semantics
  __threadfence_system();
  __syncthreads();
  if (lane == 0) __hip_atomic_store(&out->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

static int make_params(const pings_raster_settings* s, int P, const RasterKnobs& knobs, KParams& kp) {
  if (int e = fill_camera(s, P, kp)) return e;
  kp.occ_amin = knobs.occ_amin;
  kp.rect_rule = knobs.rect_rule;
  kp.live = nullptr;
  kp.dyn_rows = 0;
  return PINGS_OK;
}

// What the thread's last geometry call read back, for the binning plan of the render call that follows it: the blob it
// filled, the frame's size and its front depth.  A render of anything else (another blob, an older frame, another
// thread's frame) finds no match and sorts.  Like every other field of the geometry blob the record assumes what the
// two-call interface assumes anyway: nobody refills this blob between the geometry call and its render (a frame of
// another thread written into it in between would hand either plan that frame's ranks, rectangles and offsets under
// this frame's instance count).
struct FrontRecord {
  const void* geom = nullptr;
  int P = 0, num_tiles = 0;
  int64_t I = 0;
  uint32_t front = 0;
};
static thread_local FrontRecord t_front;
static thread_local int t_bin_plan = 0;   // what the thread's last render took: 0 = sort (or no instance), 1 = gather

// Gather the tile lists from the front ranks?  The host value of the front depth only chooses the plan and sizes
// grids and tables; the kernels read the device word.
static bool plan_gather(const RasterKnobs& knobs, const void* geom_blob, int P, int64_t I, int footprint_class,
                        const KParams& kp) {
  const FrontRecord& fr = t_front;
  const int num_tiles = kp.gx * kp.gy;
  if (knobs.bin == RasterKnobs::BIN_SORT || I <= 0) return false;
  if (fr.geom != geom_blob || fr.P != P || fr.I != I || fr.num_tiles != num_tiles) return false;
  if (!gather_fits(fr.front, kp.gx, kp.gy, occlusion_buckets(num_tiles), I)) return false;
  if (knobs.bin == RasterKnobs::BIN_GATHER) return true;
  return footprint_class == 2 && (uint64_t)fr.front * (uint64_t)num_tiles <= GATHER_COST * (uint64_t)I;
}

static int tile_bits(int num_tiles) {
  int b = 1;
  while ((1 << b) < num_tiles) ++b;
  return b;
}

}  // namespace raster
}  // namespace pings

using namespace pings::raster;

PINGS_API int pings_raster_mark_visible(const float* positions, int N,
                                        const pings_raster_settings* s, uint8_t* present,
                                        void* stream) {
  PINGS_ARG_CHECK(s && s->viewmatrix && s->projmatrix_raw, "null settings / matrices");
  if (N == 0) return PINGS_OK;
  PINGS_ARG_CHECK(N > 0 && positions && present, "null pointer");
  const int depth_only = read_knobs().mark_depth_only;
  hipLaunchKernelGGL(mark_visible_kernel, dim3(pings::ceil_div(N, 256)), dim3(256), 0,
                     pings::as_stream(stream), positions, N, s->viewmatrix, s->projmatrix_raw,
                     present, depth_only);
  PINGS_LAUNCH_CHECK();
  return PINGS_OK;
}

PINGS_API int pings_raster_rank_bucket(const int32_t* ranks, int64_t n, int occ_nb, uint32_t nvalid,
                                       uint32_t* buckets) {
  PINGS_ARG_CHECK(n >= 0 && occ_nb > 0 && (n == 0 || (ranks && buckets)), "null pointer / non-positive bucket count");
  for (int64_t i = 0; i < n; ++i) buckets[i] = rank_bucket(ranks[i], occ_nb, nvalid);
  return PINGS_OK;
}

PINGS_API int pings_raster_debug_bin_plan(int32_t* plan, uint32_t* front) {
  PINGS_ARG_CHECK(plan && front, "null pointer");
  *plan = t_bin_plan;
  *front = t_front.front;
  return PINGS_OK;
}

PINGS_API int pings_raster_debug_interior(const float* records, const float* tile_origins, int64_t n, float cxp,
                                          float cyp, float fx, float fy, uint8_t* flags) {
  PINGS_ARG_CHECK(n >= 0 && (n == 0 || (records && tile_origins && flags)), "null pointer / negative count");
  PINGS_ARG_CHECK(fx > 0.f && fy > 0.f, "non-positive focal length");
  for (int64_t i = 0; i < n; ++i) {
    const float* r = records + 16 * i;
    const float X0 = tile_origins[2 * i], Y0 = tile_origins[2 * i + 1];
    flags[i] = blend_interior(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[11], r[12], r[13], r[14], X0, Y0,
                              tile_rays(X0, Y0, cxp, cyp, fx, fy)) ? 1 : 0;
  }
  return PINGS_OK;
}

PINGS_API int pings_raster_preprocess(const pings_raster_settings* s, int P, const float* means3D,
                                      const float* colors, const float* opacities,
                                      const float* scales, const float* rotations,
                                      void* geom_blob, int32_t* radii, int64_t* num_instances,
                                      int32_t* footprint_class, void* stream) {
  return pings_raster_preprocess_dyn(s, P, means3D, colors, opacities, scales, rotations, geom_blob, radii, nullptr, 0,
                                     nullptr, 0, nullptr, num_instances, footprint_class, stream);
}

PINGS_API int pings_raster_preprocess_dyn(const pings_raster_settings* s, int P, const float* means3D,
                                          const float* colors, const float* opacities, const float* scales,
                                          const float* rotations, void* geom_blob, int32_t* radii,
                                          const int32_t* live_rows_dev, int dyn_rows,
                                          const int32_t* const* aux_dev, int aux_words, int32_t* aux_host,
                                          int64_t* num_instances, int32_t* footprint_class, void* stream) {
  const RasterKnobs knobs = read_knobs();
  KParams kp;
  if (int e = make_params(s, P, knobs, kp)) return e;
  PINGS_ARG_CHECK(num_instances != nullptr && footprint_class != nullptr, "null output");
  *num_instances = 0;
  *footprint_class = 1;
  t_front = FrontRecord{};
  PINGS_ARG_CHECK(aux_words >= 0 && aux_words <= 8 && (aux_words == 0 || (aux_dev && aux_host)), "0..8 aux words");
  PINGS_ARG_CHECK(!live_rows_dev || (dyn_rows >= 0 && dyn_rows <= P), "dyn_rows must lie in 0..P");
  PINGS_ARG_CHECK(P > 0 || aux_words == 0, "aux words need a non-empty frame");
  if (P == 0) return PINGS_OK;
  kp.live = live_rows_dev;
  kp.dyn_rows = live_rows_dev ? dyn_rows : 0;
  PINGS_ARG_CHECK(P > 0 && means3D && colors && opacities && scales && rotations && geom_blob && radii,
                  "null pointer");
  hipStream_t st = pings::as_stream(stream);
  const int num_tiles = kp.gx * kp.gy;
  GeomState gs = carve_geom(geom_blob, P, num_tiles);
  const dim3 grid(pings::ceil_div(P, 256)), block(256);
  const bool occlusion = knobs.occlusion;
  bool library_sort = knobs.library_sort;   // also the retry path of a depth-bucket overflow
  // the occlusion budget, the frame statistics and the depth-sort header in one clear (adjacent in the blob), ahead of
  // the preprocess pass, which leaves the key range in the header; a retry (depth-bucket overflow) clears again what it
  // reuses
  PINGS_HIP_CHECK(hipMemsetAsync(gs.zero_begin, 0, gs.zero_bytes, st));
  {
    pings::prof::Scope ps("preprocess", st);
    with_mode(s->mode, [&](auto m) {
      hipLaunchKernelGGL(preprocess_kernel<m()>, grid, block, 0, st, kp, means3D, colors,
                         opacities, scales, rotations, gs.rec, gs.rect, gs.depth_key, gs.gidx, radii,
                         library_sort ? (uint32_t*)nullptr : gs.ds_head, gs.stats);
    });
    PINGS_LAUNCH_CHECK();
  }
  // The record of the frame's one read-back is written by the summary kernel straight into pinned, device-mapped host
  // memory and the host POLLS its sequence number: no copy, and no blocking wait inside the runtime.  (Three pageable
  // copies, each a wait of its own, in round 2.  A blocking hipStreamSynchronize wakes through an interrupt; on one box
  // of this pool every wait that outlasted the runtime's spin phase — any frame of a million Gaussians — returned only
  // on a 60 Hz tick: 16 ms per frame, 1.15 -> 11.7 ms per headline step.  Polling a host word does not depend on it.)
  static thread_local FrameSummary* host_sum = nullptr;
  static thread_local FrameSummary* host_sum_dev = nullptr;
  static thread_local uint32_t frame_seq = 0;
  if (!host_sum) {
    PINGS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&host_sum), sizeof(FrameSummary), hipHostMallocMapped | hipHostMallocPortable));
    PINGS_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&host_sum_dev), host_sum, 0));
    host_sum->seq = 0;
  }
  AuxPtrs aux;
  for (int i = 0; i < 8; ++i) aux.p[i] = i < aux_words ? aux_dev[i] : nullptr;
  for (int attempt = 0;; ++attempt) {
    size_t tb = gs.temp_bytes;
    if (library_sort) {
      pings::prof::Scope ps("depth_sort", st);
      PINGS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(gs.temp, tb, gs.depth_key, gs.depth_key_sorted,
                                                         gs.gidx, gs.gidx_sorted, P, 0, 32, st));
      hipLaunchKernelGGL(count_valid_kernel, dim3(1), dim3(64), 0, st, P, gs.depth_key_sorted, gs.nvalid);
      PINGS_LAUNCH_CHECK();
      hipLaunchKernelGGL(invert_perm_kernel, grid, block, 0, st, P, gs.gidx_sorted, gs.rank_of);
      PINGS_LAUNCH_CHECK();
    } else {
      // first attempt only (a retry is the library sort): the header holds what preprocess_kernel left in it
      pings::prof::Scope ps("depth_sort", st);
      // arrival slots of the survivors live in rank_of until ds_rank_kernel overwrites it with the final ranks
      hipLaunchKernelGGL(ds_hist_kernel, grid, block, 0, st, P, gs.depth_key, gs.ds_head, gs.ds_cnt, gs.rank_of);
      PINGS_LAUNCH_CHECK();
      if (int e = raster_scan_u32(gs.ds_cnt, DS_NB + (int64_t)grid.x + 1, false, gs.ds_off, gs.temp, gs.temp_bytes,
                                  knobs.library_scan, st))
        return e;
      hipLaunchKernelGGL(ds_scatter_kernel, grid, block, 0, st, P, gs.depth_key, gs.ds_head, gs.ds_off, gs.rank_of,
                         gs.depth_key_sorted, gs.ds_idx, gs.gidx_sorted);
      PINGS_LAUNCH_CHECK();
      hipLaunchKernelGGL(ds_rank_kernel, grid, block, 0, st, gs.depth_key_sorted, gs.ds_idx, gs.ds_head, gs.ds_off,
                         gs.gidx_sorted, gs.rank_of, gs.nvalid);
      PINGS_LAUNCH_CHECK();
    }
    if (occlusion) {
      {
        pings::prof::Scope ps("occl_setup", st);
        if (attempt > 0)
          PINGS_HIP_CHECK(hipMemsetAsync(gs.occ_bucket, 0, sizeof(uint32_t) * (size_t)num_tiles * gs.occ_nb, st));
      }
      {
        pings::prof::Scope ps("occl_budget", st);
        hipLaunchKernelGGL(knobs.occ_walk_lanes ? occl_budget_kernel<false> : occl_budget_kernel<true>, grid, block, 0,
                           st, P, kp.gx, gs.occ_nb, gs.gidx_sorted, gs.rect, gs.rec, gs.nvalid, num_tiles, gs.occ_bucket);
        PINGS_LAUNCH_CHECK();
      }
    }
    {
      // with the bound off the budget is still all zero: every tile keeps every rank bucket (OCC_ALL, masks all ones);
      // nvalid stays: rect_lane skips the culled ranks with it
      pings::prof::Scope ps("occl_scan", st);
      // a retry clears again what the first attempt's count_kept_kernel and occl_scan_kernel left: the kept pairs and,
      // behind them, occ_bmax.  The footprint statistics stay: preprocess_kernel does not run again.
      if (attempt > 0)
        PINGS_HIP_CHECK(hipMemsetAsync(gs.stats + STAT_KEPT, 0, STAT_RETRY_WORDS * sizeof(unsigned long long), st));
      hipLaunchKernelGGL(occl_scan_kernel, dim3(gs.occ_words), dim3(512), 0, st, num_tiles, gs.occ_nb, gs.occ_bucket,
                         gs.occ_bsat, gs.occ_mask, gs.occ_bmax);
      PINGS_LAUNCH_CHECK();
    }
    {
      pings::prof::Scope ps("tile_count_scan", st);
      hipLaunchKernelGGL(count_kept_kernel, grid, block, 0, st, P, kp.gx, gs.occ_nb, gs.occ_words, gs.gidx_sorted,
                         gs.rect, gs.occ_mask, gs.nvalid, gs.occ_bmax, gs.tiles_sorted, gs.stats);
      PINGS_LAUNCH_CHECK();
    }
    // The summary needs nothing of the instance scan (the kept total is one of count_kept_kernel's 64-bit statistics),
    // so it goes first and the scan runs while the host wakes up, sizes the binning blob and issues the render.  After
    // a depth-bucket overflow the frame is redone and this scan was for nothing.
    const uint32_t seq = ++frame_seq ? frame_seq : ++frame_seq;   // never 0
    hipLaunchKernelGGL(frame_summary_kernel, dim3(1), dim3(64), 0, st,
                       library_sort ? (const uint32_t*)nullptr : gs.ds_head + DS_FLAG, gs.stats, aux, aux_words,
                       host_sum_dev, seq, gs.occ_nb, gs.nvalid, gs.occ_bmax, gs.tiles_sorted, gs.occ_front,
                       knobs.bin == RasterKnobs::BIN_SORT ? FRONT_NEVER : knobs.bin == RasterKnobs::BIN_GATHER ? FRONT_ALWAYS : FRONT_CLASS2);
    PINGS_LAUNCH_CHECK();
    {
      pings::prof::Scope ps("tile_count_scan", st);
      if (int e = raster_scan_u32(gs.tiles_sorted, P, true, gs.offsets_sorted, gs.temp, gs.temp_bytes, knobs.library_scan, st))
        return e;
    }
    {
      const auto t_start = std::chrono::steady_clock::now();
      unsigned spins = 0;
      while (__atomic_load_n(&host_sum->seq, __ATOMIC_ACQUIRE) != seq) {
        if ((++spins & 0x3FFu) == 0) {
          // every 1024 polls: has the stream failed, or has this taken absurdly long?  Then let the runtime decide.
          const hipError_t q = hipStreamQuery(st);
          if (q == hipErrorNotReady) (void)hipGetLastError();   // "not ready" must not linger as the thread's last error
          else if (q != hipSuccess) PINGS_HIP_CHECK(q);
          if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(20)) {
            PINGS_HIP_CHECK(hipStreamSynchronize(st));
            PINGS_ARG_CHECK(__atomic_load_n(&host_sum->seq, __ATOMIC_ACQUIRE) == seq, "frame summary never arrived");
          }
        }
        __builtin_ia32_pause();
      }
    }
    if (host_sum->overflow == 0) break;
    library_sort = true;  // a depth bucket overflowed: redo the frame with the library sort
  }
  const unsigned long long stats[3] = {host_sum->stats[0], host_sum->stats[1], host_sum->stats[2]};
  for (int i = 0; i < aux_words; ++i) aux_host[i] = host_sum->aux[i];
  // stats[2] is the 64-bit sum of the per-rank counts the 32-bit scan runs over: below 2^31 the scan cannot have
  // wrapped, and its last entry is this number
  PINGS_ARG_CHECK(stats[2] < 0x7FFFFFFFull, "more than 2^31 - 1 (Gaussian, tile) instances in this frame");
  *num_instances = (int64_t)stats[2];
  t_front.geom = geom_blob;
  t_front.P = P;
  t_front.num_tiles = num_tiles;
  t_front.I = (int64_t)stats[2];
  t_front.front = host_sum->front;
  // Class 2 = more than 16 (Gaussian, tile) pairs per visible Gaussian.  Footprints of many tiles reach nearly every
  // pixel of a tile: blend_plan gives such a view one wave per tile with four pixels per lane, forward and backward
  // (blend_fwd_tile_kernel, blend_bwd_tile_kernel), which amortises the per-record work.  Small footprints (class 1)
  // would leave most of those lanes idle: one wave per 8x8 quadrant with its own culled list forward
  // (blend_fwd_wave_kernel) and the Gaussian-per-lane scan backward (blend_bwd_scan_kernel).
  *footprint_class = (stats[1] > 0 && stats[0] > 16ull * stats[1]) ? 2 : 1;
  return PINGS_OK;
}

PINGS_API int pings_raster_render(const pings_raster_settings* s, int P, int64_t I,
                                  void* geom_blob, void* binning_blob, void* image_blob,
                                  float* out_color, float* out_normal,
                                  float* out_depth, float* out_alpha, void* per_gaussian,
                                  int footprint_class, void* stream) {
  const RasterKnobs knobs = read_knobs();
  KParams kp;
  if (int e = make_params(s, P, knobs, kp)) return e;
  PINGS_ARG_CHECK(out_color && out_depth && out_alpha && image_blob && binning_blob, "null pointer");
  PINGS_ARG_CHECK(s->mode == PINGS_RASTER_3DGS || out_normal, "surfel mode needs out_normal");
  PINGS_ARG_CHECK(I >= 0 && I < (int64_t)0x7FFFFFFF, "instance count out of range");
  PINGS_ARG_CHECK(P == 0 || (geom_blob && per_gaussian), "null pointer");
  hipStream_t st = pings::as_stream(stream);
  const int num_tiles = kp.gx * kp.gy;
  GeomState gs = carve_geom(geom_blob, P, num_tiles);
  BinState bs = carve_binning(binning_blob, I, num_tiles, knobs.blend_seg);
  ImageState im = carve_image(image_blob, kp.W, kp.H);

  {
    // tile ranges, per-instance weights and quadrant masks (3DGS: contributor counts too) in one clear, up to the
    // 256-byte boundary at which the next field starts (one fill launch; an odd size costs a second one for the tail)
    const char* z0 = reinterpret_cast<const char*>(bs.ranges);
    const char* z1 = I > 0 ? (s->mode == PINGS_RASTER_3DGS ? reinterpret_cast<const char*>(bs.inst_cnt + I)
                                                             : reinterpret_cast<const char*>(bs.inst_qmask + I + 1))
                           : reinterpret_cast<const char*>(bs.ranges + num_tiles);
    PINGS_HIP_CHECK(hipMemsetAsync(bs.ranges, 0, pings::align_up((size_t)(z1 - z0)), st));
  }
  const bool gather = plan_gather(knobs, geom_blob, P, I, footprint_class, kp);
  t_bin_plan = gather ? 1 : 0;
  if (gather) {
    // every kept instance lies in the first t_front.front depth ranks: each tile reads its list off those ranks
    if (int e = launch_tile_gather(kp, P, I, t_front.front, gs, bs, per_gaussian, st)) return e;
  } else if (I > 0) {
    // tile ids fit 16 bits for every image up to 4096x4096: a 2-byte key cuts the sort traffic by a quarter
    auto bin = [&](auto* key, auto* key_sorted) -> int {
      using KeyT = std::remove_pointer_t<decltype(key)>;
      {
        pings::prof::Scope ps("duplicate", st);
        hipLaunchKernelGGL(duplicate_kernel<KeyT>, dim3(pings::ceil_div(P, 256)), dim3(256), 0, st, P,
                           kp.gx, gs.occ_nb, gs.occ_words, gs.gidx_sorted, gs.offsets_sorted, gs.tiles_sorted,
                           gs.rect, gs.occ_mask, gs.nvalid, key, bs.gval, reinterpret_cast<uint32_t*>(per_gaussian));
        PINGS_LAUNCH_CHECK();
      }
      const int bits = tile_bits(num_tiles);
      const KeyT* sorted = key_sorted;
      {
        pings::prof::Scope ps("tile_sort", st);
        if (knobs.library_tile_sort || bits > 16) {
          if (int e = tile_sort_library<KeyT>(key, I, bits, key_sorted, bs.point_list, bs.temp, bs.temp_bytes, st)) return e;
        } else {
          // two passes: through key_sorted / slot_val and back into `key`; one pass: straight to key_sorted
          if (bits > 8) sorted = key;
          if (int e = tile_sort<KeyT>(key, I, bits, key_sorted, bs.slot_val, bits > 8 ? key : key_sorted, bs.point_list,
                                      reinterpret_cast<uint32_t*>(bs.temp), st))
            return e;
        }
      }
      {
        pings::prof::Scope ps("tile_ranges", st);
        hipLaunchKernelGGL(tile_ranges_kernel<KeyT>, dim3((unsigned)pings::ceil_div<int64_t>(I, 256)), dim3(256), 0,
                           st, I, sorted, bs.ranges);
        PINGS_LAUNCH_CHECK();
      }
      return PINGS_OK;
    };
    const int e = num_tiles <= 65536 ? bin(reinterpret_cast<uint16_t*>(bs.tile_key), reinterpret_cast<uint16_t*>(bs.tile_key_sorted))
                                     : bin(bs.tile_key, bs.tile_key_sorted);
    if (e) return e;
  }
  if (!gather) {
    // forward dispatch order: tiles by descending list length
    pings::prof::Scope ps_o("tile_order", st);
    hipLaunchKernelGGL(tile_order_kernel<true>, dim3(1), dim3(1024), 0, st, (const uint32_t*)nullptr, bs.ranges, num_tiles,
                       bs.tile_order, (uint32_t*)nullptr, 0u, 0u);
    PINGS_LAUNCH_CHECK();
  }
  return launch_blend_fwd(s->mode, kp, blend_plan(knobs, footprint_class, I, num_tiles), P, I, gs, bs, im, out_color,
                          out_normal, out_depth, out_alpha, per_gaussian, st);
}
